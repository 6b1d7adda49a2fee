"""Vocabulary, fixtures and model of the call-sequence tests (test_engine_model.py on the mock library, test_gpu_engine_sequences.py on
the MI355X): what the engine (csrc/engine.hip) carries from one call to the next, driven through the C ABI in any order.

  * FIXTURES: small planes -- pixels, chunks, cparams -- made once per session by the oracle (tests/_oracle.py), never by the engine;
    each stands for a geometry that sends the engine down another path.
  * ops: one small class per entry point of include/cimg_hip.h that does work.  run(eng) -> (rc, outputs); expected() -> the same
    from the oracle and numpy alone, computed once per (op kind, fixture).  Every output lies between guard bytes.
  * PendingModel: the header's protocol over the three kinds of pending work (which call voids which _begin, what a _fetch refers
    to), restated in plain Python with the header's line beside each rule.
  * Runner: keeps a PendingModel beside an engine and checks return code, outputs and guards after every op.

The library under test is given as a ctypes handle: libcimg_hip.so on the GPU, tests/emu/libcimg_hip_mock_full.so without one (device
memory is host memory there); an op whose entry point the library lacks reports itself unavailable.
"""
import ctypes as C
import os

import numpy as np

import _oracle as O
import _special_chunks as SC
import _trunc as T
import _window_writes as WW
import _window_writes_masked as WWM
import _window_writes_strided as WWS
import _window_writes_typed as WWT
import _windows as W
import _windows_strided as WS
import _windows_typed as WT
from cimg import hip as H          # the structs of the C ABI only; nothing is loaded by importing it
from cimg import synth

HERE = os.path.dirname(os.path.abspath(__file__))
MOCK_LIB = os.path.join(HERE, "emu", "libcimg_hip_mock_full.so")
ERR_READ_BUFFER, ERR_CODEC_SUPPORT, ERR_INVALID_PARAM = -5, -7, -12
CANARY = 0x5A                      # guard bytes of every output of a _fetch; an int32 of them is WORD
WORD = 0x5A5A5A5A
GUARD = 64                         # (a multiple of 16: the interleave calls want 16-byte aligned buffers)
ROW = 64                           # elements per row of the planes as the window ops see them
ROOM = 280000                      # bytes a _fetch that the model calls void offers per chunk: more than any fixture's chunk

# ---- the library ------------------------------------------------------------------------------------------------------------------
_P, _I, _L, _F = C.c_void_p, C.c_int32, C.c_int64, H._ALLOC_FN
_UPD_DEV = [_P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P]
_UPD_HOST = [_P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _F, _P, _P, _P, _P]
_WIN_DEV = [_P, _I, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P]
_WIN_HOST = [_P, _I, _P, _P, _P, _I, _P, _P, _P]
SIGNATURES = {      # include/cimg_hip.h; set on a library that has no argtypes yet (cimg.hip.load() sets its own)
    "cimg_engine_create": [C.c_int, _P], "cimg_engine_destroy": [_P], "cimg_engine_synchronize": [_P], "cimg_last_error": [_P],
    "cimg_device_malloc": [_P, C.c_size_t], "cimg_device_free": [_P, _P], "cimg_memcpy_h2d": [_P, _P, _P, C.c_size_t],
    "cimg_memcpy_d2h": [_P, _P, _P, C.c_size_t],
    "cimg_compress_batch_device": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    "cimg_compress_batch_device_begin": [_P, _P, _I, _P, _P, _P, _P, _P, _P], "cimg_compress_batch_device_fetch": [_P, _I, _P],
    "cimg_decompress_batch_device": [_P, _I, _P, _P, _P, _P, _P, _P, _P],
    "cimg_decompress_batch_device_sized": [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P],
    "cimg_decompress_batch_device_begin": [_P, _I, _P, _P, _P, _P, _P, _P],
    "cimg_decompress_batch_device_begin_sized": [_P, _I, _P, _P, _P, _P, _P, _P, _P], "cimg_decompress_batch_device_fetch": [_P, _P],
    "cimg_compress_batch_host": [_P, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    "cimg_compress_batch_host_begin": [_P, _P, _I, _P, _P, _P, _P, _P], "cimg_compress_batch_host_fetch": [_P, _I, _P, _P],
    "cimg_compress_batch_host_packed": [_P, _P, _I, _P, _P, _P, _P, _P, _F, _P, _P],
    "cimg_compress_batch_host_interleaved_begin": [_P, _P, _I, _L, _P, _I, _P, _P, _P, _P],
    "cimg_decompress_batch_host": [_P, _I, _P, _P, _P, _P, _P, _P], "cimg_decompress_batch_host_sized": [_P, _I, _P, _P, _P, _P, _P, _P, _P],
    "cimg_deinterleave_device": [_P, _P, _I, _I, _L, _P, _L], "cimg_interleave_device": [_P, _P, _L, _I, _I, _L, _P],
    "cimg_pack_chunks_device": [_P, _I, _P, _P, _P, _P],
    "cimg_compress_batch_device_packed_begin": [_P, _P, _I, _P, _P, _P, _P, _P], "cimg_compress_batch_device_packed_fetch": [_P, _I, _P, _P],
    "cimg_decompress_windows_device": _WIN_DEV, "cimg_decompress_windows_strided_device": _WIN_DEV,
    "cimg_decompress_windows_grouped_device": _WIN_DEV, "cimg_decompress_windows_typed_device": _WIN_DEV,
    "cimg_decompress_windows_host": _WIN_HOST, "cimg_decompress_windows_strided_host": _WIN_HOST, "cimg_decompress_windows_grouped_host": _WIN_HOST,
    "cimg_update_windows_device": _UPD_DEV, "cimg_update_windows_strided_device": _UPD_DEV, "cimg_update_windows_typed_device": _UPD_DEV,
    "cimg_update_windows_masked_device": _UPD_DEV + [_P],
    "cimg_update_windows_host": _UPD_HOST, "cimg_update_windows_strided_host": _UPD_HOST,
    "cimg_update_windows_masked_host": [_P, _P, _I, _P, _P, _P, _P, _I, _P, _P, _P, _F, _P, _P, _P, _P],
    "cimg_engine_wait_stream": [_P, _P], "cimg_engine_enable_timing": [_P, C.c_int], "cimg_engine_reset_timing": [_P],
    "cimg_engine_debug_stamps": [_P, C.c_int],
}


def bind(lib):
    for name, sig in SIGNATURES.items():
        if hasattr(lib, name) and getattr(lib, name).argtypes is None:
            getattr(lib, name).argtypes = sig
    lib.cimg_device_malloc.restype = C.c_void_p
    lib.cimg_last_error.restype = C.c_char_p
    for name in ("cimg_engine_destroy", "cimg_device_free", "cimg_engine_enable_timing", "cimg_engine_reset_timing", "cimg_engine_debug_stamps"):
        if hasattr(lib, name):
            getattr(lib, name).restype = None
    return lib


def mock_library():
    """tests/emu/libcimg_hip_mock_full.so (tests/emu/Makefile; build() makes it), bound"""
    if not os.path.exists(MOCK_LIB):
        raise OSError(f"{MOCK_LIB} is missing: run `make -C tests/emu`")
    return bind(C.CDLL(MOCK_LIB))


def _p(a):
    return None if a is None else a.ctypes.data


def _i32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


class Area:
    """device memory between two guard bands (canary-filled, like the area itself unless data is given)"""

    def __init__(self, eng, nbytes, data=None, canary=CANARY):
        self.eng, self.n, self.canary = eng, int(nbytes), canary
        host = np.full(self.n + 2 * GUARD, canary, np.uint8)
        if data is not None:
            d = np.ascontiguousarray(data).view(np.uint8).ravel()
            host[GUARD:GUARD + d.size] = d
        self.base = eng.L.cimg_device_malloc(eng.h, host.size)
        assert self.base, "device allocation failed"
        eng.areas.append(self)
        assert eng.L.cimg_memcpy_h2d(eng.h, self.base, _p(host), host.size) == 0
        self.ptr = self.base + GUARD

    def read(self):
        host = np.empty(self.n + 2 * GUARD, np.uint8)
        assert self.eng.L.cimg_memcpy_d2h(self.eng.h, _p(host), self.base, host.size) == 0
        assert (host[:GUARD] == self.canary).all() and (host[GUARD + self.n:] == self.canary).all(), "a call wrote outside its device output"
        return host[GUARD:GUARD + self.n]


class HostArea:
    """host memory between two guard bands"""

    def __init__(self, nbytes, canary=CANARY):
        self.full = np.full(int(nbytes) + 2 * GUARD, canary, np.uint8)
        self.a = self.full[GUARD:GUARD + int(nbytes)]
        self.canary = canary

    @property
    def ptr(self):
        return self.a.ctypes.data

    def read(self):
        assert (self.full[:GUARD] == self.canary).all() and (self.full[GUARD + self.a.size:] == self.canary).all(), "a call wrote outside its host output"
        return self.a


class Words:
    """n int32 result words (cbytes, status) between two guard words"""

    def __init__(self, n):
        self.full = np.full(n + 2, WORD, np.int32)
        self.a = self.full[1:n + 1]

    @property
    def ptr(self):
        return self.a.ctypes.data

    def read(self):
        assert self.full[0] == WORD and self.full[-1] == WORD, "a call wrote outside its result words"
        return self.a.copy()


class Eng:
    """one engine of `lib`, created fresh; device memory it handed out is freed with it"""

    def __init__(self, lib, gpu):
        self.L, self.gpu, self.areas = lib, gpu, []
        self.h = C.c_void_p()
        rc = lib.cimg_engine_create(0 if gpu else -1, C.byref(self.h))
        assert rc == 0, rc

    def has(self, *names):
        return all(hasattr(self.L, n) for n in names)

    def sync(self):
        assert self.L.cimg_engine_synchronize(self.h) == 0

    def error(self):
        return (self.L.cimg_last_error(self.h) or b"").decode(errors="replace")

    def close(self):
        if self.h:
            self.L.cimg_engine_synchronize(self.h)
            for a in self.areas:
                self.L.cimg_device_free(self.h, a.base)
            self.areas = []
            self.L.cimg_engine_destroy(self.h)
            self.h = None


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
TCODE = {"uint8": H.T_U8, "uint16": H.T_U16, "float16": H.T_F16, "float32": H.T_F32}


def engine_cparams(po):
    """the cimg_cparams of an oracle CParams (cimg_cparams_init's fields, filled by hand: no library is needed)"""
    p = H.CParams()
    p.typesize, p.clevel, p.blocksize, p.compcode, p.splitmode = po.typesize, po.clevel, po.blocksize, po.compcode, po.splitmode
    for i in range(6):
        p.filters[i], p.filters_meta[i] = po.filters[i], po.filters_meta[i]
    return p


class Fixture:
    """pixels, chunks and cparams of one small plane.  raw: what a compress call is given; pixels: what a decompress call returns (raw
    but for trunc-prec); chunks: the oracle's, with destsize = nbytes + 32.  compress: the engine's chunks are the oracle's bytes;
    write: window writes are checked on it; gpu_only: the emulator behind the mock does not take it (blocks beyond the LDS)."""

    def __init__(self, name, ts, po, raw, chunks, pixels=None, compress=True, write=None, gpu_only=False, tcode=None):
        self.name, self.ts, self.po, self.raw, self.chunks = name, ts, po, np.ascontiguousarray(raw), [bytes(c) for c in chunks]
        self.p = engine_cparams(po) if po is not None else None
        self.pixels = self.raw if pixels is None else np.ascontiguousarray(pixels)
        sizes = [O.cbuffer_sizes(np.frombuffer(c[:32], np.uint8)) for c in self.chunks]
        self.nbytes = [s[0] for s in sizes]
        self.blocksize = [s[2] for s in sizes]
        self.n = len(self.chunks)
        self.destsize = [nb + 32 for nb in self.nbytes]
        self.raw_off = [int(x) for x in np.concatenate([[0], np.cumsum(self.nbytes[:-1])])]
        self.compress, self.gpu_only, self.tcode = compress, gpu_only, tcode
        self.trunc = po is not None and po.filters[4] == T.TRUNC_PREC
        self.write = compress if write is None else write
        self.elems = self.pixels.size // ts
        self.windows = all(nb % ts == 0 for nb in self.nbytes) and self.elems >= 16 * ROW
        self.interleavable = compress and self.raw.size % 32 == 0 and ts in (1, 2, 4, 8)
        assert self.pixels.size == sum(self.nbytes) and self.pixels.size <= 1 << 20
        self.cache = {}

    def __repr__(self):
        return self.name

    # the compressed side as the device / host decode calls take it: chunks at 64-byte boundaries with a canary gap between them
    def comp_layout(self):
        if "comp" not in self.cache:
            off, at = [], 0
            for c in self.chunks:
                off.append(at)
                at += (len(c) + 63) // 64 * 64 + 64
            buf = np.full(at + 64, 0xC3, np.uint8)
            for o, c in zip(off, self.chunks):
                buf[o:o + len(c)] = np.frombuffer(c, np.uint8)
            self.cache["comp"] = (buf, off, [len(c) for c in self.chunks])
        return self.cache["comp"]

    def dest_layout(self, destsize=None):
        """where a compress call is told to put its chunks: destsize each, a canary gap between them -> (offsets, total)"""
        off, at = [], 0
        for d in (self.destsize if destsize is None else destsize):
            off.append(at)
            at += (d + 63) // 64 * 64 + 64
        return off, at

    def interleaved(self):
        """the plane as TWO channels of npixels elements, pixel-major: what the _interleaved_begin call uploads"""
        npix = self.raw.size // (2 * self.ts)
        return np.ascontiguousarray(self.raw.reshape(2, npix, self.ts).transpose(1, 0, 2)).ravel(), npix


def _plane(name, arr, chunk_bytes, compress=True, gpu_only=False, trunc=None, **kw):
    raw = np.ascontiguousarray(arr).view(np.uint8).ravel()
    ts = arr.dtype.itemsize
    if trunc is None:
        po, pixels = O.cparams(ts, **kw), raw
    else:
        po, pixels = T.oracle_cparams(ts, trunc, **kw), T.trunc(raw, ts, trunc)
    chunks = []
    for o in range(0, raw.size, chunk_bytes):
        piece = pixels[o:o + chunk_bytes]
        r, c = O.compress(po, piece, destsize=piece.size + 32)
        assert r > 0 and r == len(c), (name, r)
        chunks.append(c)
    return Fixture(name, ts, po, raw, chunks, pixels=pixels, compress=compress, write=compress and trunc is None, gpu_only=gpu_only,
                   tcode=TCODE[arr.dtype.name])


def _zstd_fixture(golden_dir):
    """zstd chunks are read only (the engine's zstd writer is format-valid, not libzstd's bytes): from the oracle's libzstd layer where
    there is one, else three frames of tests/golden/zstd_kat.npz, each the one stream of a one-block chunk"""
    if O.zstd_available():
        a = synth.natural_channel(np.uint16, ROW, 144)
        fx = _plane("zstd_u16_b4k_c3", a, 6144, compress=False, compcode=O.ZSTD, clevel=5, blocksize=4096)
    else:
        import _zstd_streams as Z
        kat = np.load(os.path.join(golden_dir, "zstd_kat.npz"))
        names = ("text", "ramp", "nibbles_16k")
        chunks = [Z.chunk_of_frame(kat["frame|%s|L3" % n].tobytes(), kat["in|" + n]) for n in names]
        fx = Fixture("zstd_golden_c3", 1, None, np.concatenate([kat["in|" + n] for n in names]), chunks, compress=False, tcode=H.T_U8)
    return fx


def _zstd_wide_fixture(golden_dir):
    """two libzstd chunks with 160 KiB blocks (a whole block and a shorter one each) out of tests/golden/zstd_wide_kat.npz, their
    pixels from the generator beside it and checked against the recorded digests: the wide zstd read path (decompress_finish_wide_zstd,
    zplan behind a wide batch)"""
    import hashlib
    import importlib.util
    kat = np.load(os.path.join(golden_dir, "zstd_wide_kat.npz"))
    spec = importlib.util.spec_from_file_location("make_zstd_wide_golden", os.path.join(golden_dir, "make_zstd_wide_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inputs = gen.inputs()
    names = ("tiled_uint16_b163840_c3", "tiled_uint16_b163840_c9")
    raws = [np.ascontiguousarray(inputs[n][0]).view(np.uint8).ravel() for n in names]
    for n, r in zip(names, raws):
        assert hashlib.sha256(r.tobytes()).hexdigest() == str(kat["in_sha256|" + n]), n
    return Fixture("zstd_wide_u16_b160k_c2", 2, None, np.concatenate(raws), [kat["chunk|" + n].tobytes() for n in names], compress=False,
                   gpu_only=True, tcode=H.T_U16)


_FIXTURES = {}


def fixtures(golden_dir=os.path.join(HERE, "golden")):
    """name -> Fixture, built once per session on the CPU"""
    if _FIXTURES:
        return _FIXTURES
    f16t = synth.tiled_channel(np.float16, 256, 396)                    # 2 chunks of three 32 KiB blocks and a leftover block
    f16n = synth.natural_channel(np.float16, 256, 396)
    six, six_plane = SC.six_chunks()
    made = [
        _plane("u16_b256_c1", synth.natural_channel(np.uint16, ROW, 64), 8192, blocksize=256),
        _plane("f32_b1k_c3", synth.natural_channel(np.float32, ROW, 60), 6144, blocksize=1024),                    # 6144 + 6144 + 3072
        _plane("u16_b4k_c40", synth.tiled_channel(np.uint16, ROW, 40 * 70), 8960, blocksize=4096),                  # 40 chunks, 8960 = 2 x 4096 + 768
        _plane("f16_tiled_b32k", f16t, 3 * 32768 + 3072, blocksize=32768),
        _plane("f16_natural_b32k", f16n, 3 * 32768 + 3072, blocksize=32768),
        _plane("blosclz_u16_b4k_c2", synth.natural_channel(np.uint16, ROW, 160), 10240, compcode=O.BLOSCLZ, blocksize=4096),
        _plane("u8_unsplit_b4k_c3", synth.natural_channel(np.uint8, ROW, 480), 10240, blocksize=4096),
        # (128 KiB blocks of float32 split into four 32 KiB planes: streams the oracle writes too, so the wide encoder's bytes are its)
        _plane("f32_wide_b128k_c2", synth.tiled_channel(np.float32, 256, 520), 2 * 131072 + 4096, blocksize=131072, gpu_only=True),
        _zstd_fixture(golden_dir),
        _zstd_wide_fixture(golden_dir),
        _plane("u16_clevel0_c2", synth.natural_channel(np.uint16, ROW, 128), 8192, clevel=0, blocksize=4096),
        Fixture("special6", SC.TS, SC.plane_params(), six_plane.view(np.uint8).ravel(), six, compress=False, tcode=H.T_F32),
        _plane("f32_trunc12_c2", synth.natural_channel(np.float32, ROW, 64), 8192, trunc=12, blocksize=4096),
    ]
    for fx in made:
        _FIXTURES[fx.name] = fx
    return _FIXTURES


# ---- ops --------------------------------------------------------------------------------------------------------------------------
class Op:
    """One call.  begins / fetches: the PendingModel slot it opens / consumes ("enc": the compress device flight, "dec": the
    decompress device flight, "staged": the staging-area batch); voids: the slots whose pending _begin it makes void; needs: the entry
    points it calls; count: the chunk count a _fetch names (None: cimg_decompress_batch_device_fetch names none)."""
    begins = fetches = None
    voids = ()
    needs = ()
    count = None
    gpu_only = False
    accepted = True                    # (a _begin that is itself refused opens nothing)

    def __init__(self, fx=None):
        self.fx = fx

    @property
    def name(self):
        return type(self).__name__ + ("" if self.fx is None else "(%s)" % self.fx.name)

    def __repr__(self):
        return self.name

    def available(self, eng):
        if not eng.has(*self.needs):
            return False
        if eng.gpu or self.fx is None:
            return eng.gpu or not self.gpu_only
        # (the emulator behind the mock takes no wide blocks, and its compress batch no trunc-prec)
        return not (self.gpu_only or self.fx.gpu_only or (self.fx.trunc and isinstance(self, (_Compress, _BadParams))))

    def cached(self, key, make):
        c = self.fx.cache
        if key not in c:
            c[key] = make()
        return c[key]

    def expected(self):
        return 0, {}


def _chunks_at(buf, off, cbytes):
    return [buf[o:o + max(int(c), 0)].tobytes() for o, c in zip(off, cbytes)]


def _gaps_intact(buf, off, room, canary=CANARY):
    """the bytes between the chunk slots of a compress output are still canary"""
    ok = True
    for i, o in enumerate(off):
        end = off[i + 1] if i + 1 < len(off) else buf.size
        ok = ok and bool((buf[o + room[i]:end] == canary).all())
    return ok


class _Compress(Op):
    """shared by every compress call: the oracle's chunks and sizes for the fixture's destsize"""
    voids = ("enc",)
    destsize = None                    # None: the fixture's (every chunk fits)

    def sizes(self):
        return self.fx.destsize if self.destsize is None else self.destsize

    def expected(self):
        def make():
            out = []
            for i, ds in enumerate(self.sizes()):
                if ds == self.fx.destsize[i]:
                    out.append(self.fx.chunks[i])
                else:
                    piece = self.fx.pixels[self.fx.raw_off[i]:self.fx.raw_off[i] + self.fx.nbytes[i]]
                    r, c = O.compress(self.fx.po, piece, destsize=ds)
                    out.append(c if r > 0 else b"")
            return out
        chunks = self.cached(("compress", tuple(self.sizes())), make)
        return 0, {"cbytes": np.array([len(c) for c in chunks], np.int32), "chunks": chunks}

    def device_inputs(self, eng):
        fx = self.fx
        self.d_raw = Area(eng, fx.raw.size, fx.raw)
        self.off, total = fx.dest_layout(self.sizes())
        self.d_comp = Area(eng, total)
        self.keep = [_i64(fx.raw_off), _i32(fx.nbytes), _i64(self.off), _i32(self.sizes())]
        self.args = (C.byref(fx.p), fx.n, self.d_raw.ptr, _p(self.keep[0]), _p(self.keep[1]), self.d_comp.ptr, _p(self.keep[2]), _p(self.keep[3]))

    def device_outputs(self, cbytes):
        buf = self.d_comp.read()
        assert _gaps_intact(buf, self.off, self.sizes()), "%s wrote between its chunk slots" % self.name
        return {"cbytes": cbytes, "chunks": _chunks_at(buf, self.off, cbytes)}


class CompressDevice(_Compress):
    needs = ("cimg_compress_batch_device",)
    reuse = False                      # True: a second run() of the op goes into the device buffers of the first

    def run(self, eng):
        if not (self.reuse and hasattr(self, "d_comp")):
            self.device_inputs(eng)
        cb = Words(self.fx.n)
        rc = eng.L.cimg_compress_batch_device(eng.h, *self.args, cb.ptr)
        return rc, self.device_outputs(cb.read())


class CompressDeviceDoesNotFit(CompressDevice):
    """chunk 0 is given 48 bytes: cbytes 0, the others as ever"""

    def __init__(self, fx):
        super().__init__(fx)
        self.destsize = [48] + fx.destsize[1:]


class CompressDeviceBegin(_Compress):
    needs = ("cimg_compress_batch_device_begin",)
    begins = "enc"

    def run(self, eng):
        self.device_inputs(eng)
        return eng.L.cimg_compress_batch_device_begin(eng.h, *self.args), {}

    def expected(self):
        return 0, {}


class CompressDeviceFetch(Op):
    needs = ("cimg_compress_batch_device_fetch",)
    fetches = "enc"

    def __init__(self, count):
        super().__init__()
        self.count = count

    def run(self, eng, begin=None):
        cb = Words(self.count)
        rc = eng.L.cimg_compress_batch_device_fetch(eng.h, self.count, cb.ptr)
        out = {"cbytes": cb.read()}
        if begin is not None and rc == 0:
            out = begin.device_outputs(out["cbytes"])
        return rc, out

    @staticmethod
    def expected_of(begin):
        return _Compress.expected(begin)


class _Decompress(Op):
    voids = ("dec",)
    sized = False

    def expected(self):
        return 0, {"status": np.zeros(self.fx.n, np.int32), "pixels": self.fx.pixels}

    def device_inputs(self, eng, d_comp=None, comp_off=None):
        fx = self.fx
        buf, off, sizes = fx.comp_layout()
        self.d_comp = Area(eng, buf.size, buf) if d_comp is None else d_comp
        self.d_raw = Area(eng, fx.pixels.size)
        self.keep = [_i64(off if comp_off is None else comp_off), _i32(sizes), _i32(fx.nbytes), _i32(fx.blocksize), _i64(fx.raw_off)]
        k = self.keep
        head = (fx.n, self.d_comp.ptr, _p(k[0]))
        tail = (_p(k[2]), _p(k[3]), self.d_raw.ptr, _p(k[4]))
        self.args = head + ((_p(k[1]),) if self.sized else ()) + tail

    def device_outputs(self, status):
        return {"status": status, "pixels": self.d_raw.read()}


class DecompressDevice(_Decompress):
    needs = ("cimg_decompress_batch_device",)
    reuse = False                      # True: a second run() of the op goes into the device buffers of the first

    def run(self, eng):
        if not (self.reuse and hasattr(self, "d_raw")):
            self.device_inputs(eng)
        st = Words(self.fx.n)
        rc = eng.L.cimg_decompress_batch_device(eng.h, *self.args, st.ptr)
        return rc, self.device_outputs(st.read())


class DecompressDeviceSized(_Decompress):
    needs = ("cimg_decompress_batch_device_sized",)
    sized = True

    def run(self, eng):
        self.device_inputs(eng)
        st = Words(self.fx.n)
        rc = eng.L.cimg_decompress_batch_device_sized(eng.h, *self.args, st.ptr)
        return rc, self.device_outputs(st.read())


class DecompressDeviceBegin(_Decompress):
    """after: a CompressDeviceBegin still in flight whose chunks this batch reads (the chain include/cimg_hip.h:92-95 allows)"""
    needs = ("cimg_decompress_batch_device_begin",)
    begins = "dec"

    def __init__(self, fx, after=None):
        super().__init__(fx)
        self.after = after

    def run(self, eng):
        if self.after is None:
            self.device_inputs(eng)
        else:
            self.device_inputs(eng, self.after.d_comp, self.after.off)
        fn = eng.L.cimg_decompress_batch_device_begin_sized if self.sized else eng.L.cimg_decompress_batch_device_begin
        return fn(eng.h, *self.args), {}

    def result(self):
        return _Decompress.expected(self)

    def expected(self):
        return 0, {}


class DecompressDeviceBeginSized(DecompressDeviceBegin):
    needs = ("cimg_decompress_batch_device_begin_sized",)
    sized = True


class DecompressDeviceFetch(Op):
    needs = ("cimg_decompress_batch_device_fetch",)
    fetches = "dec"

    def __init__(self, nstatus):
        super().__init__()
        self.nstatus = nstatus             # (the call names no count: this many status words are offered)

    def run(self, eng, begin=None):
        st = Words(self.nstatus)
        rc = eng.L.cimg_decompress_batch_device_fetch(eng.h, st.ptr)
        out = {"status": st.read()}
        if begin is not None and rc == 0:
            assert (out["status"][begin.fx.n:] == WORD).all(), "the fetch wrote more status words than the begun batch has chunks"
            out = begin.device_outputs(out["status"][:begin.fx.n])
        return rc, out

    @staticmethod
    def expected_of(begin):
        return begin.result()


def _host_comp_out(fx, sizes):
    off, total = fx.dest_layout(sizes)
    return off, HostArea(total)


class CompressHost(_Compress):
    needs = ("cimg_compress_batch_host",)
    voids = ("enc", "staged")

    def run(self, eng):
        fx = self.fx
        off, out = _host_comp_out(fx, self.sizes())
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i64(off), _i32(self.sizes())]
        rc = eng.L.cimg_compress_batch_host(eng.h, C.byref(fx.p), fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), out.ptr, _p(k[2]), _p(k[3]), cb.ptr)
        cbytes = cb.read()
        buf = out.read()
        assert _gaps_intact(buf, off, self.sizes())
        return rc, {"cbytes": cbytes, "chunks": _chunks_at(buf, off, cbytes) if rc == 0 else []}


class CompressHostBegin(_Compress):
    needs = ("cimg_compress_batch_host_begin",)
    voids = ("enc", "staged")
    begins = "staged"

    def run(self, eng):
        fx = self.fx
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i32(self.sizes())]
        rc = eng.L.cimg_compress_batch_host_begin(eng.h, C.byref(fx.p), fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), _p(k[2]), cb.ptr)
        return rc, {"cbytes": cb.read()}

    def expected(self):
        rc, want = _Compress.expected(self)
        return rc, {"cbytes": want["cbytes"]}


class CompressHostInterleavedBegin(CompressHostBegin):
    needs = ("cimg_compress_batch_host_interleaved_begin",)

    def run(self, eng):
        fx = self.fx
        il, npix = fx.interleaved()
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i32(self.sizes())]
        rc = eng.L.cimg_compress_batch_host_interleaved_begin(eng.h, C.byref(fx.p), 2, npix, _p(il), fx.n, _p(k[0]), _p(k[1]), _p(k[2]), cb.ptr)
        return rc, {"cbytes": cb.read()}


class CompressHostFetch(Op):
    needs = ("cimg_compress_batch_host_fetch",)
    fetches = "staged"

    def __init__(self, count, room=None):
        super().__init__()
        self.count = count
        self.room = room if room is not None else [ROOM] * count       # bytes offered per chunk (the begun batch's cbytes where it is known)

    def run(self, eng, begin=None):
        room = [len(c) for c in _Compress.expected(begin)[1]["chunks"]] if begin is not None else self.room
        off, at = [], 0
        for r in room:
            off.append(at)
            at += r + 64
        out = HostArea(at)
        k = _i64(off)
        rc = eng.L.cimg_compress_batch_host_fetch(eng.h, self.count, out.ptr, _p(k))
        buf = out.read()
        if rc == 0:
            assert _gaps_intact(buf, off, room), "the fetch wrote between its chunk slots"
            return rc, {"chunks": _chunks_at(buf, off, room)}
        return rc, {"chunks": _chunks_at(buf, off, room), "all": buf}       # (a void fetch: the runner wants every byte untouched, gaps included)

    @staticmethod
    def expected_of(begin):
        return 0, {"chunks": _Compress.expected(begin)[1]["chunks"]}


class CompressHostPacked(_Compress):
    needs = ("cimg_compress_batch_host_packed",)
    voids = ("enc", "staged")

    def run(self, eng):
        fx = self.fx
        cb = Words(fx.n)
        ptrs = (C.c_void_p * fx.n)()
        keep = []

        def alloc(_user, n):
            b = C.create_string_buffer(max(int(n), 1))
            keep.append(b)
            return C.addressof(b)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i32(self.sizes())]
        rc = eng.L.cimg_compress_batch_host_packed(eng.h, C.byref(fx.p), fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), _p(k[2]), cb.ptr, H._ALLOC_FN(alloc), None, ptrs)
        cbytes = cb.read()
        chunks = [C.string_at(ptrs[i], int(cbytes[i])) if rc == 0 and ptrs[i] and cbytes[i] > 0 else b"" for i in range(fx.n)]
        return rc, {"cbytes": cbytes, "chunks": chunks}


class DecompressHost(_Decompress):
    needs = ("cimg_decompress_batch_host",)
    voids = ("dec", "staged")

    def run(self, eng):
        fx = self.fx
        buf, off, sizes = fx.comp_layout()
        out = HostArea(fx.pixels.size)
        st = Words(fx.n)
        k = [_i64(off), _i32(sizes), _i64(fx.raw_off), _i32(fx.nbytes)]
        if self.sized:
            rc = eng.L.cimg_decompress_batch_host_sized(eng.h, fx.n, _p(buf), _p(k[0]), _p(k[1]), out.ptr, _p(k[2]), _p(k[3]), st.ptr)
        else:
            rc = eng.L.cimg_decompress_batch_host(eng.h, fx.n, _p(buf), _p(k[0]), out.ptr, _p(k[2]), _p(k[3]), st.ptr)
        return rc, {"status": st.read(), "pixels": out.read()}


class DecompressHostSized(DecompressHost):
    needs = ("cimg_decompress_batch_host_sized",)
    sized = True


class CompressDevicePackedBegin(_Compress):
    needs = ("cimg_compress_batch_device_packed_begin",)
    voids = ("enc", "staged")
    begins = "staged"

    def run(self, eng):
        fx = self.fx
        d_raw = Area(eng, fx.raw.size, fx.raw)
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i32(self.sizes())]
        rc = eng.L.cimg_compress_batch_device_packed_begin(eng.h, C.byref(fx.p), fx.n, d_raw.ptr, _p(k[0]), _p(k[1]), _p(k[2]), cb.ptr)
        return rc, {"cbytes": cb.read()}

    def expected(self):
        rc, want = _Compress.expected(self)
        return rc, {"cbytes": want["cbytes"]}


class CompressDevicePackedFetch(Op):
    """chunks back to back at odd addresses: exactly the bytes _begin reported"""
    needs = ("cimg_compress_batch_device_packed_fetch",)
    fetches = "staged"

    def __init__(self, count, room=None):
        super().__init__()
        self.count = count
        self.room = room if room is not None else [ROOM] * count

    def run(self, eng, begin=None):
        room = [len(c) for c in _Compress.expected(begin)[1]["chunks"]] if begin is not None else self.room
        off, at = [], 3
        for r in room:
            off.append(at)
            at += r + 5
        dst = Area(eng, at)
        k = _i64(off)
        rc = eng.L.cimg_compress_batch_device_packed_fetch(eng.h, self.count, dst.ptr, _p(k))
        buf = dst.read()
        if rc == 0:
            assert _gaps_intact(buf, off, room), "the packed fetch wrote between its chunks"
            return rc, {"chunks": _chunks_at(buf, off, room)}
        return rc, {"chunks": _chunks_at(buf, off, room), "all": buf}

    expected_of = staticmethod(CompressHostFetch.expected_of)


class PackChunks(Op):
    """the fixture's chunks gathered out of one device buffer to odd addresses of another"""
    needs = ("cimg_pack_chunks_device",)

    def run(self, eng):
        buf, off, sizes = self.fx.comp_layout()
        src = Area(eng, buf.size, buf)
        dst_off, at = [], 1
        for s in sizes:
            dst_off.append(at)
            at += s + 7
        dst = Area(eng, at)
        addr = np.array([src.ptr + o for o in off], np.uint64)
        k = [_i32(sizes), _i64(dst_off)]
        rc = eng.L.cimg_pack_chunks_device(eng.h, self.fx.n, _p(addr), _p(k[0]), dst.ptr, _p(k[1]))
        out = dst.read()
        assert _gaps_intact(out, dst_off, sizes)
        return rc, {"chunks": _chunks_at(out, dst_off, sizes)}

    def expected(self):
        return 0, {"chunks": self.fx.chunks}


class Deinterleave(Op):
    """returns when enqueued: the engine is synchronised before the planes are read"""
    needs = ("cimg_deinterleave_device",)

    def run(self, eng):
        il, npix = self.fx.interleaved()
        src, dst = Area(eng, il.size, il), Area(eng, il.size)
        rc = eng.L.cimg_deinterleave_device(eng.h, src.ptr, 2, self.fx.ts, npix, dst.ptr, npix * self.fx.ts)
        eng.sync()
        return rc, {"planes": dst.read()}

    def expected(self):
        return 0, {"planes": self.fx.raw}


class Interleave(Op):
    needs = ("cimg_interleave_device",)

    def run(self, eng):
        il, npix = self.fx.interleaved()
        src, dst = Area(eng, il.size, self.fx.raw), Area(eng, il.size)
        rc = eng.L.cimg_interleave_device(eng.h, src.ptr, npix * self.fx.ts, 2, self.fx.ts, npix, dst.ptr)
        return rc, {"pixels": dst.read()}

    def expected(self):
        return 0, {"pixels": self.fx.interleaved()[0]}


# ---- window reads -----------------------------------------------------------------------------------------------------------------
def _standard(fx):
    """_windows.standard_windows over the fixture's plane (rows of ROW elements); with one chunk, the window that straddles "the chunk
    boundary" loses the rows that would lie behind the plane"""
    out = []
    for d in W.standard_windows(fx.elems, ROW, fx.nbytes[0] // fx.ts, fx.n):
        d = dict(d, col_pitch=1)
        while d["origin"] + (d["height"] - 1) * d["row_pitch"] + d["width"] > fx.elems:
            d["height"] -= 1
        assert d["height"] >= 1
        out.append(d)
    return out


def read_specs(fx):
    """the standard windows and two strided ones"""
    s = _standard(fx)
    s.append(dict(chunk_first=0, chunk_count=fx.n, origin=5, row_pitch=1, col_pitch=3, width=min(200, (fx.elems - 6) // 3 + 1), height=1))
    s.append(dict(chunk_first=0, chunk_count=fx.n, origin=11, row_pitch=2 * ROW + 1, col_pitch=2, width=29, height=5))
    return s


class _WindowRead(Op):
    voids = ("dec",)
    entry = None
    strided = True                     # the specs carry col_pitch
    host = False

    @property
    def needs(self):
        return (self.entry,)

    def specs(self):
        def make():
            s = read_specs(self.fx)
            if not self.strided:
                s = [{k: v for k, v in d.items() if k != "col_pitch"} for d in s if d["col_pitch"] == 1]
            return W.pack(s, self.fx.ts)
        return self.cached(("rspecs", self.strided), make)

    def expected(self):
        def make():
            specs, size = self.specs()
            full = [dict(d, col_pitch=d.get("col_pitch", 1)) for d in specs]
            return WS.expected([self.fx.pixels] * len(full), full, self.fx.ts, size)
        return 0, {"status": np.zeros(self.fx.n, np.int32), "out": self.cached(("rwant", self.strided), make)}

    def warr(self, specs):
        return H.strided_windows(specs) if self.strided else H.windows(specs)

    def run(self, eng):
        fx = self.fx
        specs, size = self.specs()
        buf, off, sizes = fx.comp_layout()
        st = Words(fx.n)
        w = self.warr(specs)
        fn = getattr(eng.L, self.entry)
        if self.host:
            out = HostArea(size, W.CANARY)
            k = [_i64(off), _i32(sizes)]
            rc = fn(eng.h, fx.n, _p(buf), _p(k[0]), _p(k[1]), len(specs), w, out.ptr, st.ptr)
        else:
            d_comp, out = Area(eng, buf.size, buf), Area(eng, size, canary=W.CANARY)
            k = [_i64(off), _i32(sizes), _i32(fx.nbytes), _i32(fx.blocksize)]
            rc = fn(eng.h, fx.n, d_comp.ptr, _p(k[0]), _p(k[1]), _p(k[2]), _p(k[3]), fx.ts, len(specs), w, out.ptr, st.ptr)
        return rc, {"status": st.read(), "out": out.read()}


class WindowsDevice(_WindowRead):
    entry, strided = "cimg_decompress_windows_device", False


class WindowsStridedDevice(_WindowRead):
    entry = "cimg_decompress_windows_strided_device"


class WindowsGroupedDevice(_WindowRead):
    entry = "cimg_decompress_windows_grouped_device"


class WindowsTypedDevice(_WindowRead):
    """the read windows dressed as _windows_typed dresses its own: one identity window, the others converted to float32 or float16 with
    the scale / offset pairs of _windows_typed.AFFINE in turn and an elem_pitch of 1, 3 or 4 output sizes; checked element by element,
    bit for bit, against numpy (_windows_typed.check_output, which also wants every other byte untouched)"""
    entry = "cimg_decompress_windows_typed_device"

    def specs(self):
        def make():
            tc = self.fx.tcode
            t = [WT.typed(d, tc, (H.T_F32, H.T_F16)[k % 2], *WT.AFFINE[k % len(WT.AFFINE)], pitch_mult=(1, 3, 4)[k % 3])
                 for k, d in enumerate(read_specs(self.fx))]
            t[0] = WT.typed(read_specs(self.fx)[0], tc, tc)
            return WT.pack_typed(t)
        return self.cached(("tspecs",), make)

    def warr(self, specs):
        return H.typed_windows(specs)

    def expected(self):
        return 0, {"status": np.zeros(self.fx.n, np.int32)}

    def run(self, eng):
        rc, out = super().run(eng)
        if rc == 0:
            specs, _ = self.specs()
            WT.check_output(out["out"], [self.fx.pixels.view(WT.DTYPE[self.fx.tcode])] * len(specs), specs)
        return rc, out


class WindowsHost(_WindowRead):
    entry, strided, host, voids = "cimg_decompress_windows_host", False, True, ("dec", "staged")


class WindowsStridedHost(_WindowRead):
    entry, host, voids = "cimg_decompress_windows_strided_host", True, ("dec", "staged")


class WindowsGroupedHost(_WindowRead):
    entry, host, voids = "cimg_decompress_windows_grouped_host", True, ("dec", "staged")


# ---- window writes ----------------------------------------------------------------------------------------------------------------
def write_specs(fx):
    s = [d for i, d in enumerate(_standard(fx)) if i in (0, 1, 3)]
    s.append(dict(chunk_first=0, chunk_count=fx.n, origin=ROW + 7, row_pitch=3 * ROW, col_pitch=2, width=23, height=4))
    return s


class _WindowWrite(Op):
    voids = ("enc", "dec")
    entry = None
    strided = True
    host = False

    @property
    def needs(self):
        return (self.entry,)

    def made(self):
        """-> (specs, uint8 source, uint8 masks or None, the oracle's new chunks), once per (op kind, fixture)"""
        def make():
            s = write_specs(self.fx)
            if not self.strided:
                s = [{k: v for k, v in d.items() if k != "col_pitch"} for d in s if d["col_pitch"] == 1]
            specs, src = WW.source(s, self.fx.ts, seed=len(self.fx.name))
            full = [dict(d, col_pitch=d.get("col_pitch", 1)) for d in specs]
            want, _ = WWS.expected(self.fx.po, self.fx.chunks, full, self.fx.ts, src, self.fx.destsize)
            return specs, src, None, want
        return self.cached(("write", self.strided), make)

    def expected(self):
        want = self.made()[3]
        return 0, {"status": np.zeros(self.fx.n, np.int32), "new_cbytes": np.array([len(c) if c else 0 for c in want], np.int32),
                   "new": [c if c else b"" for c in want]}

    def warr(self, specs):
        return H.strided_windows(specs) if self.strided else H.windows(specs)

    masked = False                     # the masked calls take a mask pointer behind the source

    def run(self, eng):
        fx = self.fx
        specs, src, masks, _ = self.made()
        buf, off, sizes = fx.comp_layout()
        st, ncb = Words(fx.n), Words(fx.n)
        w = self.warr(specs)
        fn = getattr(eng.L, self.entry)
        if self.host:
            ptrs = (C.c_void_p * fx.n)()
            keep = []

            def alloc(_user, n):
                b = C.create_string_buffer(max(int(n), 1))
                keep.append(b)
                return C.addressof(b)
            k = [_i64(off), _i32(sizes), _i32(fx.destsize)]
            extra = (_p(masks),) if self.masked else ()
            rc = fn(eng.h, C.byref(fx.p), fx.n, _p(buf), _p(k[0]), _p(k[1]), _p(k[2]), len(specs), w, _p(src), *extra, H._ALLOC_FN(alloc), None,
                    ptrs, ncb.ptr, st.ptr)
            cb = ncb.read()
            new = [C.string_at(ptrs[i], int(cb[i])) if ptrs[i] and cb[i] > 0 else b"" for i in range(fx.n)]
        else:
            new_off, total = fx.dest_layout()
            d_comp, d_src, d_new = Area(eng, buf.size, buf), Area(eng, src.size, src), Area(eng, total)
            k = [_i64(off), _i32(sizes), _i32(fx.nbytes), _i32(fx.blocksize), _i32(fx.destsize), _i64(new_off)]
            extra = (Area(eng, masks.size, masks).ptr,) if self.masked else ()
            rc = fn(eng.h, C.byref(fx.p), fx.n, d_comp.ptr, _p(k[0]), _p(k[1]), _p(k[2]), _p(k[3]), _p(k[4]), len(specs), w, d_src.ptr, *extra,
                    d_new.ptr, _p(k[5]), ncb.ptr, st.ptr)
            cb = ncb.read()
            out = d_new.read()
            assert _gaps_intact(out, new_off, fx.destsize)
            new = _chunks_at(out, new_off, cb)
        return rc, {"status": st.read(), "new_cbytes": cb, "new": new}


class UpdateDevice(_WindowWrite):
    entry, strided = "cimg_update_windows_device", False


class UpdateStridedDevice(_WindowWrite):
    entry = "cimg_update_windows_strided_device"


class UpdateTypedDevice(_WindowWrite):
    """the write windows dressed as _window_writes_typed dresses its own: float32 and float16 memory, the scale / offset pairs of its
    PAIRS in turn, elem_pitch of 1, 3 or 4 memory sizes, source values out of its tables (ties, saturation edges, NaN, subnormals); the
    new chunks are the oracle's for numpy's conversion (_window_writes_typed.expected)"""
    entry = "cimg_update_windows_typed_device"

    def made(self):
        def make():
            s, tc = write_specs(self.fx), self.fx.tcode
            t = WWT.dress(s[:2], tc, H.T_F32) + WWT.dress(s[2:], tc, H.T_F16, k0=2)
            specs, src, vals = WWT.source(t, seed=len(self.fx.name))
            want, _ = WWT.expected(self.fx.po, self.fx.chunks, specs, vals, self.fx.destsize)
            return specs, src, None, want
        return self.cached(("write", "typed"), make)

    def warr(self, specs):
        return H.typed_windows(specs)


class UpdateMaskedDevice(_WindowWrite):
    """the write windows dressed as _window_writes_masked dresses its own: the four forms in turn (array, constant, array under a mask,
    constant under a mask), the mask kinds in turn, mask rows at odd offsets; the new chunks are the oracle's for np.copyto(view, src or
    value, where=mask) (_window_writes_masked.expected)"""
    entry, masked = "cimg_update_windows_masked_device", True

    def made(self):
        def make():
            specs, src, masks = WWM.dress(write_specs(self.fx), "mixed", self.fx.ts, mask="cycle", seed=len(self.fx.name))
            want, _ = WWM.expected(self.fx.po, self.fx.chunks, specs, self.fx.ts, src, masks, self.fx.destsize)
            return specs, src, masks, want
        return self.cached(("write", "masked"), make)

    def warr(self, specs):
        return H.masked_windows(specs)


class UpdateHost(_WindowWrite):
    entry, strided, host, voids = "cimg_update_windows_host", False, True, ("enc", "dec", "staged")


class UpdateStridedHost(_WindowWrite):
    entry, host, voids = "cimg_update_windows_strided_host", True, ("enc", "dec", "staged")


class UpdateMaskedHost(UpdateMaskedDevice):
    entry, host, voids = "cimg_update_windows_masked_host", True, ("enc", "dec", "staged")


# ---- calls that touch no pending work -------------------------------------------------------------------------------------------
class WaitStream(Op):
    needs = ("cimg_engine_wait_stream",)

    def run(self, eng):
        return eng.L.cimg_engine_wait_stream(eng.h, None), {}


class EnableTiming(Op):
    needs = ("cimg_engine_enable_timing",)

    def __init__(self, period):
        super().__init__()
        self.period = period

    @property
    def name(self):
        return "EnableTiming(%d)" % self.period

    def run(self, eng):
        eng.L.cimg_engine_enable_timing(eng.h, self.period)
        return 0, {}


class ResetTiming(Op):
    needs = ("cimg_engine_reset_timing",)

    def run(self, eng):
        eng.L.cimg_engine_reset_timing(eng.h)
        return 0, {}


class DebugStamps(Op):
    needs = ("cimg_engine_debug_stamps",)

    def __init__(self, on):
        super().__init__()
        self.on = on

    @property
    def name(self):
        return "DebugStamps(%d)" % self.on

    def run(self, eng):
        eng.L.cimg_engine_debug_stamps(eng.h, self.on)
        return 0, {}


# ---- refused and failing calls: none hands a malformed stream to a kernel ---------------------------------------------------------
class Refused(Op):
    """expected(): the set of return codes the call may give; outputs it must leave alone are checked by run()"""
    codes = (ERR_INVALID_PARAM,)

    def expected(self):
        return self.codes, {}


class CompressDeviceNoChunks(Refused):
    """nchunks = 0: nothing to do, nothing launched, nothing voided"""
    needs, codes = ("cimg_compress_batch_device",), (0,)

    def run(self, eng):
        cb = Words(1)
        rc = eng.L.cimg_compress_batch_device(eng.h, C.byref(self.fx.p), 0, None, None, None, None, None, None, cb.ptr)
        assert cb.read()[0] == WORD
        return rc, {}


class DecompressDeviceNoChunks(Refused):
    needs, codes = ("cimg_decompress_batch_device",), (0,)

    def run(self, eng):
        st = Words(1)
        rc = eng.L.cimg_decompress_batch_device(eng.h, 0, None, None, None, None, None, None, st.ptr)
        assert st.read()[0] == WORD
        return rc, {}


class CompressDeviceNullArgument(Refused):
    """no cbytes array: refused before anything is looked at, so a pending compress _begin stands"""
    needs = ("cimg_compress_batch_device",)

    def run(self, eng):
        k = [_i64(self.fx.raw_off), _i32(self.fx.nbytes), _i32(self.fx.destsize)]
        d = Area(eng, 64)
        return eng.L.cimg_compress_batch_device(eng.h, C.byref(self.fx.p), self.fx.n, d.ptr, _p(k[0]), _p(k[1]), d.ptr, _p(k[0]), _p(k[2]), None), {}


class CompressHostNullArgument(Refused):
    """no destination: refused before the staging area is touched"""
    needs = ("cimg_compress_batch_host",)
    gpu_only = True                    # (the mock trusts its callers' pointers)

    def run(self, eng):
        fx = self.fx
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i32(fx.destsize)]
        rc = eng.L.cimg_compress_batch_host(eng.h, C.byref(fx.p), fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), None, None, _p(k[2]), cb.ptr)
        assert (cb.read() == WORD).all()
        return rc, {}


class CompressHostNullParams(Refused):
    """no cparams.  cimg_compress_batch_host has claimed the staging area by the time it looks at p (a staged batch is void), but not
    the compress result area: a pending compress _begin stands (include/cimg_hip.h:109-110)"""
    needs, voids = ("cimg_compress_batch_host",), ("staged",)
    gpu_only = True                    # (the mock trusts its callers' pointers)

    def run(self, eng):
        fx = self.fx
        off, out = _host_comp_out(fx, fx.destsize)
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i64(off), _i32(fx.destsize)]
        rc = eng.L.cimg_compress_batch_host(eng.h, None, fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), out.ptr, _p(k[2]), _p(k[3]), cb.ptr)
        assert (cb.read() == WORD).all() and (out.read() == CANARY).all()
        return rc, {}


class CompressHostPackedNullParams(CompressHostNullParams):
    needs = ("cimg_compress_batch_host_packed",)

    def run(self, eng):
        fx = self.fx
        cb = Words(fx.n)
        ptrs = (C.c_void_p * fx.n)()
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i32(fx.destsize)]
        rc = eng.L.cimg_compress_batch_host_packed(eng.h, None, fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), _p(k[2]), cb.ptr, H._ALLOC_FN(lambda u, n: None), None, ptrs)
        assert (cb.read() == WORD).all()
        return rc, {}


class CompressHostBeginNoChunks(Refused):
    """a _begin always replaces what its slot held, also with nchunks = 0: nothing is staged after it (include/cimg_hip.h:105-106, 166-167)"""
    needs, codes, voids = ("cimg_compress_batch_host_begin",), (0,), ("staged",)

    def run(self, eng):
        cb = Words(1)
        rc = eng.L.cimg_compress_batch_host_begin(eng.h, C.byref(self.fx.p), 0, None, None, None, None, cb.ptr)
        assert cb.read()[0] == WORD
        return rc, {}


class CompressDevicePackedBeginNoChunks(CompressHostBeginNoChunks):
    needs = ("cimg_compress_batch_device_packed_begin",)

    def run(self, eng):
        cb = Words(1)
        rc = eng.L.cimg_compress_batch_device_packed_begin(eng.h, C.byref(self.fx.p), 0, None, None, None, None, cb.ptr)
        assert cb.read()[0] == WORD
        return rc, {}


class CompressDeviceBeginNoChunks(Refused):
    """... and so does the device _begin: a batch of no chunks is in flight, a _fetch that names the old count fails"""
    needs, codes, voids = ("cimg_compress_batch_device_begin",), (0,), ("enc",)

    def run(self, eng):
        return eng.L.cimg_compress_batch_device_begin(eng.h, C.byref(self.fx.p), 0, None, None, None, None, None, None), {}


class _BadParams(Refused):
    codes = (ERR_CODEC_SUPPORT, ERR_INVALID_PARAM)

    def params(self):
        p = engine_cparams(self.fx.po)
        self.spoil(p)
        return p


class CompressDeviceBlocksizeZero(_BadParams):
    """the planner refuses blocksize = 0; the call is a plain compress call all the same: a pending compress _begin is void"""
    needs, voids = ("cimg_compress_batch_device",), ("enc",)
    gpu_only = True                    # (the emulator's planner picks a block size of its own)

    def spoil(self, p):
        p.blocksize = 0

    def run(self, eng):
        op = CompressDevice(self.fx)
        op.device_inputs(eng)
        cb = Words(self.fx.n)
        rc = eng.L.cimg_compress_batch_device(eng.h, C.byref(self.params()), *op.args[1:], cb.ptr)
        assert (cb.read() == WORD).all(), "a refused batch reported sizes"
        return rc, {}


class CompressHostTwoFilters(_BadParams):
    """shuffle AND bitshuffle: a pipeline the planner rejects, after the host call has claimed the staging area"""
    needs, voids = ("cimg_compress_batch_host",), ("enc", "staged")

    def spoil(self, p):
        p.filters[4], p.filters[5] = H.SHUFFLE, H.BITSHUFFLE

    def run(self, eng):
        fx = self.fx
        off, out = _host_comp_out(fx, fx.destsize)
        cb = Words(fx.n)
        k = [_i64(fx.raw_off), _i32(fx.nbytes), _i64(off), _i32(fx.destsize)]
        rc = eng.L.cimg_compress_batch_host(eng.h, C.byref(self.params()), fx.n, _p(fx.raw), _p(k[0]), _p(k[1]), out.ptr, _p(k[2]), _p(k[3]), cb.ptr)
        assert (out.read() == CANARY).all(), "a refused batch wrote chunks"
        return rc, {}


class DecompressDeviceSizedShortBuffer(_Decompress):
    """chunk 0's buffer is said to hold one byte less than its header's cbytes: READ_BUFFER for it, decided on the host; the others
    decode (include/cimg_hip.h:122-125)"""
    needs = ("cimg_decompress_batch_device_sized",)
    sized = True
    gpu_only = True                    # (the mock refuses the whole batch)

    def run(self, eng):
        self.device_inputs(eng)
        self.keep[1][0] -= 1
        st = Words(self.fx.n)
        rc = eng.L.cimg_decompress_batch_device_sized(eng.h, *self.args, st.ptr)
        out = self.device_outputs(st.read())
        n0 = self.fx.nbytes[0]
        assert (out["pixels"][:n0] == CANARY).all(), "pixels of a refused chunk were written"
        return rc, {"status": out["status"], "pixels": out["pixels"][n0:]}

    def expected(self):
        st = np.zeros(self.fx.n, np.int32)
        st[0] = ERR_READ_BUFFER
        return ERR_READ_BUFFER, {"status": st, "pixels": self.fx.pixels[self.fx.nbytes[0]:]}


class DecompressDeviceSizedZlibHeader(DecompressDeviceSizedShortBuffer):
    """chunk 0's header names zlib (codec format 3): CODEC_SUPPORT for it, decided on the host; the others decode"""

    def run(self, eng):
        buf, off, sizes = self.fx.comp_layout()
        bad = buf.copy()
        bad[off[0] + 2] = (bad[off[0] + 2] & 0x1F) | (3 << 5)
        self.device_inputs(eng, Area(eng, bad.size, bad))
        st = Words(self.fx.n)
        rc = eng.L.cimg_decompress_batch_device_sized(eng.h, *self.args, st.ptr)
        out = self.device_outputs(st.read())
        n0 = self.fx.nbytes[0]
        assert (out["pixels"][:n0] == CANARY).all(), "pixels of a refused chunk were written"
        return rc, {"status": out["status"], "pixels": out["pixels"][n0:]}

    def expected(self):
        st = np.zeros(self.fx.n, np.int32)
        st[0] = ERR_CODEC_SUPPORT
        return ERR_CODEC_SUPPORT, {"status": st, "pixels": self.fx.pixels[self.fx.nbytes[0]:]}


# ---- the vocabulary ---------------------------------------------------------------------------------------------------------------
COMPRESS_OPS = (CompressDevice, CompressHost, CompressHostPacked)
DECOMPRESS_OPS = (DecompressDevice, DecompressDeviceSized, DecompressHost, DecompressHostSized)
READ_OPS = (WindowsDevice, WindowsStridedDevice, WindowsGroupedDevice, WindowsTypedDevice, WindowsHost, WindowsStridedHost, WindowsGroupedHost)
WRITE_OPS = (UpdateDevice, UpdateStridedDevice, UpdateTypedDevice, UpdateMaskedDevice, UpdateHost, UpdateStridedHost, UpdateMaskedHost)
REFUSED_OPS = (CompressDeviceNoChunks, DecompressDeviceNoChunks, CompressDeviceNullArgument, CompressHostNullArgument, CompressDeviceBlocksizeZero,
               CompressHostNullParams, CompressHostPackedNullParams, CompressHostBeginNoChunks, CompressDevicePackedBeginNoChunks, CompressDeviceBeginNoChunks,
               CompressHostTwoFilters)
FAILING_OPS = (DecompressDeviceSizedShortBuffer, DecompressDeviceSizedZlibHeader, CompressDeviceDoesNotFit)
BEGIN_OPS = (CompressDeviceBegin, DecompressDeviceBegin, DecompressDeviceBeginSized, CompressHostBegin, CompressHostInterleavedBegin,
             CompressDevicePackedBegin)
FETCH_OF = {"enc": CompressDeviceFetch, "dec": DecompressDeviceFetch}


def fits(cls, fx):
    """may an op of this class be made on this fixture?"""
    if issubclass(cls, (CompressHostInterleavedBegin, Deinterleave, Interleave)):
        return fx.interleavable
    if issubclass(cls, _WindowWrite):
        return fx.write and fx.windows
    if issubclass(cls, _WindowRead):
        return fx.windows and (not issubclass(cls, WindowsTypedDevice) or fx.tcode is not None)
    if issubclass(cls, (_Compress, Refused)) and not issubclass(cls, DecompressDeviceNoChunks):
        return fx.compress
    if issubclass(cls, DecompressDeviceSizedZlibHeader):              # (a memcpyed chunk has no coded stream: nobody asks for its codec)
        return fx.n > 1 and fx.compress and fx.po.clevel > 0
    if issubclass(cls, DecompressDeviceSizedShortBuffer):
        return fx.n > 1 and fx.compress
    return True


def plain_ops(fx_by_name, small="f32_b1k_c3"):
    """one op of every successful kind that opens no pending work, each on the small fixture: the intervening ops of the pending
    matrix and the followers of the error tests"""
    fx = fx_by_name[small]
    ops = [cls(fx) for cls in COMPRESS_OPS + DECOMPRESS_OPS + READ_OPS + WRITE_OPS + (PackChunks, Deinterleave, Interleave) if fits(cls, fx)]
    return ops + [WaitStream(), EnableTiming(1), EnableTiming(0), ResetTiming(), DebugStamps(1), DebugStamps(0)]


def pending_ops(fx_by_name, n, other="u8_unsplit_b4k_c3"):
    """one _begin of every kind (on another geometry) and one _fetch of every kind (naming n chunks): the rest of the pending matrix's
    intervening ops"""
    fx = fx_by_name[other]
    return [cls(fx) for cls in BEGIN_OPS if fits(cls, fx)] + [CompressDeviceFetch(n), DecompressDeviceFetch(64), CompressHostFetch(n),
                                                              CompressDevicePackedFetch(n)]


def error_ops(fx_by_name, small="f32_b1k_c3"):
    fx = fx_by_name[small]
    return [cls(fx) for cls in REFUSED_OPS + FAILING_OPS if fits(cls, fx)]


# ---- the model --------------------------------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self, ok, begin):
        self.ok, self.begin = ok, begin


class PendingModel:
    """include/cimg_hip.h on pending work, and nothing else.  Three slots, each None or the _begin op whose results wait there:

      enc     the compress device flight     cimg_compress_batch_device_begin -> _device_fetch(nchunks)
      dec     the decompress device flight   cimg_decompress_batch_device_begin(_sized) -> _device_fetch
      staged  the staging-area batch         cimg_compress_batch_host_begin, _host_interleaved_begin, _device_packed_begin
                                             -> cimg_compress_batch_host_fetch(nchunks) or _device_packed_fetch(nchunks)

    apply(op) -> None, or for a _fetch a Verdict: does the header say it succeeds, and which _begin does it deliver.
    An op says what it is through begins / fetches / voids / count (class Op); the rules those attributes follow are the header's:

      R1  "ONE compress batch and ONE decompress batch may be in flight together" (h:92): enc and dec are separate slots, and a call
          of one kind leaves the other kind's flight alone.
      R2  "Each _fetch refers to the most recent _begin of its kind" (h:96): a _begin replaces what its slot held.
      R3  "every call that compresses -- the plain device call, the host-resident calls, _device_packed_begin, the window writes -- voids
          a pending compress _begin, every call that decompresses -- plain, sized, host-resident, the window reads and writes -- a
          pending decompress _begin" (h:96-103, as corrected: the engine keeps one result area per kind, and such a call overwrites
          it).  voids holds "enc" / "dec" accordingly.
      R4  "_fetch refers to the most recent _begin on this engine; a call that reuses the staging area -- every host-resident batch,
          window and update call, and _device_packed_begin -- voids it; device-resident calls leave it valid" (h:159-168, as corrected;
          the packed section h:432-436 always said so).  voids holds "staged" for those.
      R5  a _fetch whose chunk count is not the pending batch's fails and leaves the batch pending (h:110-111, h:168, as corrected).
      R6  "A _begin ALWAYS replaces what its slot held, also when it is refused or has nchunks <= 0"; of the other refused calls a
          plain device call with nchunks <= 0 or a missing array, and a host-resident call with nchunks <= 0 or without its
          destination, void nothing; any other refused call may void like a call of its kind, and a host-resident call refused for a
          missing p has claimed the staging area (h:105-111, h:166-168, as corrected).  Each refused op states its case in voids.
      R7  "delivers it once" (h:96, h:161): a _fetch that succeeds empties its slot, a second _fetch fails.  Calls that neither
          compress, decompress nor stage (deinterleave, interleave, pack, wait_stream, timing, stamps) void nothing (h:104-105).
      R8  window reads void a pending decompress _begin, the host forms the staged batch as well (h:207-209); window writes void
          both device flights, the host forms the staged batch as well (h:319-321); _device_packed_begin voids a pending compress
          _begin (h:436-437)."""

    SLOTS = ("enc", "dec", "staged")

    def __init__(self):
        self.enc = self.dec = self.staged = None

    def pending(self, slot):
        return getattr(self, slot)

    def apply(self, op):
        verdict = None
        if op.fetches:
            begin = getattr(self, op.fetches)
            if begin is None:                                              # R7, or never begun
                verdict = Verdict(False, None)
            elif op.count is not None and op.count != begin.fx.n:          # R5
                verdict = Verdict(False, None)
            else:
                verdict = Verdict(True, begin)
                setattr(self, op.fetches, None)                            # R7
        for slot in op.voids:                                              # R3, R4, R6
            setattr(self, slot, None)
        if op.begins and op.accepted:                                      # R2
            setattr(self, op.begins, op)
        return verdict


# ---- the runner -------------------------------------------------------------------------------------------------------------------
def _same(got, want):
    if isinstance(want, (list, tuple)):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    if isinstance(want, (bytes, bytearray)):
        return bytes(got) == bytes(want)
    return np.array_equal(np.asarray(got), np.asarray(want))


def _untouched(v):
    if isinstance(v, (list, tuple)):
        return all(_untouched(x) for x in v)
    a = np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else np.ascontiguousarray(v).view(np.uint8)
    return bool((a == CANARY).all())


class Runner:
    """an engine and the model beside it; step(op) runs the op and checks everything it returned"""

    def __init__(self, eng, label=""):
        self.eng, self.model, self.log, self.label = eng, PendingModel(), [], label

    def fail(self, op, what):
        tail = "\n".join("    %3d  %s" % (len(self.log) - len(self.log[-10:]) + i, o.name) for i, o in enumerate(self.log[-10:]))
        raise AssertionError("%s%s: %s\n  engine says: %s\n  the last ops (replay in this order on a fresh engine):\n%s"
                             % (self.label and self.label + ": ", op.name, what, self.eng.error(), tail))

    def step(self, op):
        if not op.available(self.eng):
            return False
        verdict = self.model.apply(op)
        self.log.append(op)
        if op.fetches:
            rc, got = op.run(self.eng, verdict.begin if verdict.ok else None)
            if verdict.ok:
                want_rc, want = op.expected_of(verdict.begin)
            else:
                if rc != ERR_INVALID_PARAM:
                    self.fail(op, "the header says this _fetch is void (ERR_INVALID_PARAM), it returned %d" % rc)
                if not _untouched(list(got.values())):
                    self.fail(op, "a void _fetch wrote into the caller's output")
                return True
        else:
            rc, got = op.run(self.eng)
            want_rc, want = op.expected()
        if not (rc in want_rc if isinstance(want_rc, tuple) else rc == want_rc):
            self.fail(op, "returned %d, expected %s" % (rc, want_rc))
        for key, w in want.items():
            if not _same(got[key], w):
                self.fail(op, "%s differs from the oracle's" % key)
        return True


# ---- seeded sequences -------------------------------------------------------------------------------------------------------------
def seeded_sequence(runner, fx_by_name, rng, nops, names=None):
    """nops ops drawn from the whole vocabulary, the model kept beside the engine and everything checked after every op.  The weights:
    the geometry (fixture) changes every few ops, about one op in five is a _begin -- left open until a _fetch of its kind is drawn,
    another _begin replaces it or a call voids it --, one in five a _fetch (sometimes with a wrong count, often of nothing), one in ten
    a refused or failing call."""
    fxs = [fx_by_name[n] for n in (names or list(fx_by_name))]
    plain = COMPRESS_OPS + DECOMPRESS_OPS + READ_OPS + WRITE_OPS + (PackChunks, Deinterleave, Interleave)
    errors = REFUSED_OPS + FAILING_OPS
    fx = fxs[0]
    done = tries = 0
    while done < nops and tries < 20 * nops:
        tries += 1
        if rng.random() < 0.3:
            fx = fxs[int(rng.integers(len(fxs)))]
        u, m, op = rng.random(), runner.model, None
        if u < 0.20:
            cls = BEGIN_OPS[int(rng.integers(len(BEGIN_OPS)))]
            if issubclass(cls, DecompressDeviceBegin) and m.enc is not None and rng.random() < 0.5:
                op = cls(m.enc.fx, after=m.enc)                            # the chain: it reads the chunks of the compress batch in flight
            elif issubclass(cls, DecompressDeviceBegin) or fits(cls, fx):
                op = cls(fx)
        elif u < 0.40:
            slot = PendingModel.SLOTS[int(rng.integers(3))]
            pend = m.pending(slot)
            n = (pend.fx.n if pend is not None else fx.n) + (1 if rng.random() < 0.15 else 0)
            op = (CompressDeviceFetch(n) if slot == "enc" else DecompressDeviceFetch(64) if slot == "dec" else
                  (CompressHostFetch if rng.random() < 0.5 else CompressDevicePackedFetch)(n))
        elif u < 0.50:
            cls = errors[int(rng.integers(len(errors)))]
            op = cls(fx) if fits(cls, fx) else None
        elif u < 0.56:
            op = (WaitStream(), EnableTiming(int(rng.choice([0, 1, 3]))), ResetTiming(), DebugStamps(int(rng.integers(2))))[int(rng.integers(4))]
        else:
            cls = plain[int(rng.integers(len(plain)))]
            op = cls(fx) if fits(cls, fx) else None
        if op is not None and runner.step(op):
            done += 1
    assert done == nops, "only %d of %d ops could be drawn" % (done, nops)
