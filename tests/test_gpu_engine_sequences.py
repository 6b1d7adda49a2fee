"""Call sequences over the engine's cross-call state (csrc/engine.hip, struct cimg_engine) on the MI355X: every entry point of
include/cimg_hip.h that does work, in orders no other test file uses, on engines created fresh, with the header's protocol
(tests/_engine_model.py: PendingModel) kept beside the engine and every result compared with the oracle's.

  a. the pending matrix: every kind of _begin x every kind of call in between x its _fetch
  b. after every refused or failing call, every successful call
  c. named scenarios, one per piece of state: descriptor caches, growth and shrink of the scratch areas, queue-head parity, the
     adaptive decode shape, timing, codecs back to back -- and the shrunk forms of what (a) found
  d. seeded sequences over the whole vocabulary (CIMG_TEST_SEED moves the seeds)

Nothing here is timed, no child process is started, no environment switch is read but CIMG_TEST_SEED.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import _engine_model as M
from cimg import hip

pytestmark = pytest.mark.gpu

SMALL, OTHER = "f32_b1k_c3", "u8_unsplit_b4k_c3"


@pytest.fixture(scope="module")
def fx(golden_dir):
    return M.fixtures(golden_dir)


@pytest.fixture(scope="module")
def lib():
    return M.bind(hip.load())


@pytest.fixture
def run(lib):
    eng = M.Eng(lib, gpu=True)
    yield M.Runner(eng)
    eng.close()


def decode_stats(run):
    v = [C.c_int64(0) for _ in range(4)]
    run.eng.L.cimg_engine_decode_stats(run.eng.h, *[C.byref(x) for x in v])
    return {"lean_batches": v[0].value, "left": v[1].value, "total": v[2].value, "zstd_batches": v[3].value}


def kernel_launches(run, kernel):
    ms, n = C.c_double(0), C.c_int64(0)
    assert run.eng.L.cimg_engine_kernel_time(run.eng.h, kernel, C.byref(ms), C.byref(n)) == 0
    return n.value


# ---- a. the pending matrix ----------------------------------------------------------------------------------------------------------
FETCHES = {"enc": (M.CompressDeviceFetch,), "dec": (M.DecompressDeviceFetch,), "staged": (M.CompressHostFetch, M.CompressDevicePackedFetch)}


def _fetch(cls, n):
    return cls(64) if cls is M.DecompressDeviceFetch else cls(n)


PENDING = {
    "compress_device_begin": (M.CompressDeviceBegin, SMALL),
    "decompress_device_begin": (M.DecompressDeviceBegin, SMALL),
    "decompress_device_begin_sized": (M.DecompressDeviceBeginSized, SMALL),
    "decompress_device_begin_sized_wide": (M.DecompressDeviceBeginSized, "f32_wide_b128k_c2"),
    "decompress_device_begin_sized_wide_zstd": (M.DecompressDeviceBeginSized, "zstd_wide_u16_b160k_c2"),
    "compress_host_begin": (M.CompressHostBegin, SMALL),
    "compress_host_interleaved_begin": (M.CompressHostInterleavedBegin, SMALL),
    "compress_device_packed_begin": (M.CompressDevicePackedBegin, SMALL),
}


@pytest.mark.parametrize("kind", list(PENDING))
def test_pending_matrix(fx, run, kind):
    """_begin, one call in between, _fetch -- for every kind of call: the fetch succeeds exactly where PendingModel (the header) says
    so and then delivers the begun batch; where it fails it fails with ERR_INVALID_PARAM and leaves the caller's output alone; the
    call in between gives its own expected result; and the next plain calls on the same engine give theirs."""
    begin_cls, name = PENDING[kind]
    base, other = fx[name], fx[OTHER]
    # every successful kind, every refused and failing kind, a _begin of every kind (the second _begin of the same kind among them, of
    # another geometry) and a _fetch of every kind
    between = M.plain_ops(fx) + M.error_ops(fx) + M.pending_ops(fx, base.n, OTHER)
    assert len(between) == 54, len(between)                        # 30 successful kinds, 14 refused or failing, 6 _begin, 4 _fetch
    pairs = 0
    for x in between:
        for fetch_cls in FETCHES[begin_cls.begins]:                # (a staged batch: once through each of its two _fetch kinds)
            run.label = "pair (%s, %s, %s)" % (kind, x.name, fetch_cls.__name__)
            begin = begin_cls(base)
            assert run.step(begin)
            assert run.step(copy.copy(x)), x.name
            run.step(_fetch(fetch_cls, base.n))
            left = run.model.pending(begin.begins)                  # (the second _begin, where the first fetch named the wrong count)
            if left is not None:
                run.step(_fetch(fetch_cls, left.fx.n))
            run.step(M.CompressDevice(other))
            run.step(M.DecompressDevice(other))
            pairs += 1
    assert pairs == len(between) * len(FETCHES[begin_cls.begins]), pairs


def test_fetch_with_the_wrong_chunk_count_leaves_the_batch_pending(fx, run):
    f = fx[SMALL]
    for begin, fetch in ((M.CompressDeviceBegin, M.CompressDeviceFetch), (M.CompressHostBegin, M.CompressHostFetch),
                         (M.CompressDevicePackedBegin, M.CompressDevicePackedFetch)):
        run.step(begin(f))
        run.step(fetch(f.n + 1))
        run.step(fetch(f.n - 1))
        run.step(fetch(f.n))
        run.step(fetch(f.n))                                       # delivered once
    run.step(M.DecompressDeviceFetch(64))                          # never begun


@pytest.mark.parametrize("order", ["compress_first", "decompress_first"])
def test_compress_and_decompress_fetch_in_either_order(fx, run, order):
    a, b = fx[SMALL], fx["u16_b4k_c40"]
    for enc_fx, dec_fx in ((a, b), (b, a), (a, a)):
        run.step(M.CompressDeviceBegin(enc_fx))
        run.step(M.DecompressDeviceBegin(dec_fx))
        fetches = [M.CompressDeviceFetch(enc_fx.n), M.DecompressDeviceFetch(64)]
        for f in (fetches if order == "compress_first" else fetches[::-1]):
            run.step(f)


def test_decompress_begin_directly_behind_the_compress_begin_it_reads(fx, run):
    """include/cimg_hip.h:92-95: stream order lets the decode batch see the chunks the compress batch in flight is writing"""
    for name in (SMALL, "f16_tiled_b32k", "u16_b4k_c40", OTHER):
        enc = M.CompressDeviceBegin(fx[name])
        run.step(enc)
        run.step(M.DecompressDeviceBegin(fx[name], after=enc))
        run.step(M.CompressDeviceFetch(fx[name].n))
        run.step(M.DecompressDeviceFetch(64))


# ---- b. after every error, every call -----------------------------------------------------------------------------------------------
def _error_names():
    return [c.__name__ for c in M.REFUSED_OPS + M.FAILING_OPS]


@pytest.mark.parametrize("error", _error_names())
def test_after_an_error_every_call_gives_its_result(fx, run, error):
    """the class of ADVICE r2 (a rejected batch finished on the previous batch's state, a result area read before it was reserved, a
    retry that cleared the wrong status words), closed over the whole ABI: each refused or failing call, then each successful kind"""
    err, o = getattr(M, error)(fx[SMALL]), fx[OTHER]
    units = [[op] for op in M.plain_ops(fx)]
    units += [[M.CompressDeviceBegin(o), M.CompressDeviceFetch(o.n)], [M.DecompressDeviceBegin(o), M.DecompressDeviceFetch(64)],
              [M.DecompressDeviceBeginSized(o), M.DecompressDeviceFetch(64)], [M.CompressHostBegin(o), M.CompressHostFetch(o.n)],
              [M.CompressDevicePackedBegin(o), M.CompressDevicePackedFetch(o.n)], [M.CompressHostInterleavedBegin(o), M.CompressHostFetch(o.n)]]
    for unit in units:
        run.label = "(%s, %s)" % (error, unit[0].name)
        assert run.step(copy.copy(err))
        for op in unit:
            assert run.step(copy.copy(op))


def test_an_error_on_a_fresh_engine_then_a_begin(fx, lib):
    for error in _error_names():
        eng = M.Eng(lib, gpu=True)
        r = M.Runner(eng, error)
        r.step(getattr(M, error)(fx[SMALL]))
        r.step(M.DecompressDeviceBegin(fx[SMALL]))
        r.step(M.CompressDeviceBegin(fx[SMALL]))
        r.step(M.DecompressDeviceFetch(64))
        r.step(M.CompressDeviceFetch(fx[SMALL].n))
        eng.close()


# ---- c. named scenarios -------------------------------------------------------------------------------------------------------------
def test_compress_host_call_voids_a_compress_device_begin(fx, run):
    """Found by the matrix.  The host-resident compress calls run compress_launch inside, which reuses the one result area the compress
    kinds share (h_out); the engine left cflight_chunks standing, and cimg_compress_batch_device_fetch handed out the HOST batch's
    sizes as the begun batch's.  The results are not intact, so the fetch must fail: the engine now voids the flight."""
    for host in (M.CompressHost, M.CompressHostBegin, M.CompressHostPacked, M.CompressHostInterleavedBegin):
        run.step(M.CompressDeviceBegin(fx["u16_b4k_c40"]))
        run.step(host(fx[SMALL]))
        run.step(M.CompressDeviceFetch(fx["u16_b4k_c40"].n))
        run.step(M.CompressDeviceFetch(fx[SMALL].n))
        run.step(M.CompressDevice(fx["u16_b4k_c40"]))


def test_decompress_host_call_voids_a_decompress_device_begin(fx, run):
    """Found by the matrix.  cimg_decompress_batch_host(_sized) runs decompress_launch inside, which resets the one decode flight
    (dflight, h_dec); the engine left dflight_open standing, and cimg_decompress_batch_device_fetch finished the HOST batch a second
    time, writing ITS chunk count of status words into the caller's array.  The fetch must fail: the engine now voids the flight."""
    for host in (M.DecompressHost, M.DecompressHostSized):
        run.step(M.DecompressDeviceBegin(fx[SMALL]))
        run.step(host(fx["u16_b4k_c40"]))
        run.step(M.DecompressDeviceFetch(64))
        run.step(M.DecompressDevice(fx[SMALL]))


# the same op with another destsize (compress) or the chunks elsewhere in their buffer (comp_off): geometry the descriptor caches
# (shadow_enc, shadow_dec, shadow_wide) must notice; d_comp / d_raw are new device buffers in every op anyway
class CompressDeviceRoomier(M.CompressDevice):
    def __init__(self, fx):
        super().__init__(fx)
        self.destsize = [d + 64 for d in fx.destsize]


class CompressDeviceShifted(M.CompressDevice):
    def device_inputs(self, eng):
        super().device_inputs(eng)
        self.off = [o + 64 for o in self.off]
        self.d_comp = M.Area(eng, self.d_comp.n + 64)
        self.keep[2] = M._i64(self.off)
        self.args = self.args[:5] + (self.d_comp.ptr, M._p(self.keep[2]), self.args[7])


class DecompressDeviceShifted(M.DecompressDevice):
    def device_inputs(self, eng, d_comp=None, comp_off=None):
        buf, off, _ = self.fx.comp_layout()
        moved = np.concatenate([np.full(192, 0xC3, np.uint8), buf])
        super().device_inputs(eng, M.Area(eng, moved.size, moved), [o + 192 for o in off])


@pytest.mark.parametrize("name", [SMALL, "f16_tiled_b32k", "f32_wide_b128k_c2"])
def test_descriptor_cache(fx, run, name):
    """shadow_enc / shadow_dec / shadow_wide (the third fixture takes the wide encoder and the wide decoder): the same batch three times
    in the same device buffers and twice in others (the upload is skipped), then only destsize changed, only comp_off
    changed, and the first geometry again after a 40-chunk batch has reallocated the descriptor buffers"""
    f, many = fx[name], fx["u16_b4k_c40"]
    again = [M.CompressDevice(f), M.DecompressDevice(f)]              # the same batch in the SAME device buffers: identical descriptors
    for op in again:
        op.reuse = True
        for _ in range(3):
            run.step(op)
    if f.compress:
        for op in (M.CompressDevice, M.CompressDevice, CompressDeviceRoomier, M.CompressDevice, CompressDeviceShifted, M.CompressDevice):
            run.step(op(f))
        run.step(M.CompressDevice(many))
        run.step(M.CompressDevice(f))
        run.step(CompressDeviceShifted(f))
    for op in (M.DecompressDevice, M.DecompressDevice, DecompressDeviceShifted, M.DecompressDevice, M.DecompressDeviceSized, DecompressDeviceShifted):
        run.step(op(f))
    run.step(M.DecompressDevice(many))
    for op in again:
        run.step(op)
    run.step(M.DecompressDevice(f))
    run.step(DecompressDeviceShifted(f))
    run.step(M.DecompressDeviceBegin(f))
    run.step(M.DecompressDeviceFetch(64))


def test_growth_and_shrink(fx, run):
    """chunk counts 1 -> 40 -> 2 -> 3 and block sizes 256 B -> 32 KiB -> 1 KiB through compress, decompress, grouped windows and
    strided updates: sync / sync_chunks / placed, the descriptor buffers and every grow-only area reserve() frees and reallocates;
    then a compress _begin held open across a decode batch that grows, and the reverse"""
    order = ["u16_b256_c1", "u16_b4k_c40", "f16_tiled_b32k", SMALL]
    for name in order + order[::-1]:
        f = fx[name]
        for cls in (M.CompressDevice, M.DecompressDevice, M.WindowsGroupedDevice, M.UpdateStridedDevice, M.CompressHost, M.DecompressHost,
                    M.WindowsGroupedHost, M.UpdateStridedHost):
            run.step(cls(f))
    for held, grows in (("u16_b256_c1", "u16_b4k_c40"), (SMALL, "f16_natural_b32k"), ("u16_b4k_c40", "f32_wide_b128k_c2")):
        run.step(M.CompressDeviceBegin(fx[held]))
        run.step(M.DecompressDevice(fx[grows]))
        run.step(M.WindowsGroupedDevice(fx[grows]))
        run.step(M.CompressDeviceFetch(fx[held].n))
        run.step(M.DecompressDeviceBegin(fx[held]))
        if fx[grows].compress:
            run.step(M.CompressDevice(fx[grows]))
        run.step(M.CompressDevice(fx["u16_b4k_c40"]))
        run.step(M.DecompressDeviceFetch(64))


def test_queue_head_parity(fx, run):
    """qpar[2]: an odd number of split launches and an even number of unsplit ones, interleaved, a refused batch and a does-not-fit
    batch in between; then a batch with leftover blocks (its second launch on the side stream: side_used) directly followed by a
    refused call and a plain batch"""
    split, unsplit, left = fx[SMALL], fx[OTHER], fx["f16_tiled_b32k"]
    for op in (M.CompressDevice(split), M.CompressDevice(unsplit), M.CompressDevice(split), M.CompressDeviceBlocksizeZero(split),
               M.CompressDevice(unsplit), M.CompressDeviceDoesNotFit(split), M.CompressDevice(split), M.CompressDevice(unsplit),
               M.CompressDeviceDoesNotFit(unsplit), M.CompressDevice(unsplit), M.CompressDevice(split)):
        run.step(op)
    for refused in (M.CompressDeviceBlocksizeZero, M.CompressDeviceNullArgument, M.CompressHostTwoFilters):
        run.step(M.CompressDevice(left))
        run.step(refused(split))
        run.step(M.CompressDevice(split))
        run.step(M.CompressDeviceBegin(left))
        run.step(refused(split))
        run.step(M.CompressDevice(left))


def test_lean_adaptivity(fx, run):
    """lean_last_skipped / lean_hold.  The natural 32 KiB-block batch has both planes coded: the lean kernel leaves more than a quarter
    of its blocks, which arms the hold -- `if ((int64_t)skipped * 4 > plan.total_blocks) e->lean_hold = 16;` in
    decompress_finish_normal (csrc/engine.hip) -- and decompress_launch skips the lean launch while it counts the hold down, one a
    batch.  So of 18 tiled batches behind it the first 16 are not lean and the 17th is again: lean_batches rises no later than the
    17th.  Every batch is pixel-exact."""
    run.step(M.DecompressDevice(fx["f16_natural_b32k"]))
    s = decode_stats(run)
    assert s["lean_batches"] == 1 and s["left"] * 4 > s["total"], s
    rose = None
    for k in range(1, 19):
        run.step(M.DecompressDevice(fx["f16_tiled_b32k"]))
        if rose is None and decode_stats(run)["lean_batches"] > 1:
            rose = k
    assert rose is not None and rose <= 17, rose


def test_timing_periods(fx, run):
    """timing / timing_period / batch_no: enable_timing(1), (3) and (0) around the batches with leftover blocks (a timed batch skips the
    side-stream shape); results do not change, one K_DECODE launch is counted per timed decode call (lean + general = one timed
    decode) and one K_ENCODE launch per timed compress call of a batch with one kind of block, and reset_timing between a _begin and its _fetch loses nothing"""
    f, one = fx["f16_tiled_b32k"], fx["u16_b256_c1"]
    for _ in range(2):                                             # (untimed first: lean_last_skipped settles, the side-stream shape is in use)
        run.step(M.DecompressDevice(f))
    for period, calls, timed in ((1, 4, 4), (3, 7, 3), (0, 3, 0)):
        run.step(M.EnableTiming(period))
        run.step(M.ResetTiming())
        for _ in range(calls):
            run.step(M.DecompressDevice(f))
            run.step(M.CompressDevice(one))
        assert kernel_launches(run, hip.K_DECODE) == timed, (period, kernel_launches(run, hip.K_DECODE))
        # (a compress batch is one encode launch per kind of block, include/cimg_hip.h:75; `one` has one kind: split, no leftover block)
        assert kernel_launches(run, hip.K_ENCODE) == timed, (period, kernel_launches(run, hip.K_ENCODE))
        run.step(M.CompressDevice(f))
    run.step(M.EnableTiming(1))
    run.step(M.CompressDeviceBegin(f))
    run.step(M.DecompressDeviceBegin(f))
    run.step(M.ResetTiming())
    run.step(M.DecompressDeviceFetch(64))
    run.step(M.CompressDeviceFetch(f.n))
    run.step(M.EnableTiming(0))
    run.step(M.DecompressDevice(f))


def test_mixed_codecs_back_to_back(fx, run):
    """zstd decode (plans, zplan groups), lz4, wide blocks, wide zstd (libzstd's chunks with 160 KiB blocks: decompress_finish_wide_zstd,
    zplan behind a wide batch), the wide encoder, special chunks, a trunc-prec compress (trunc_src) -- then the list reversed; and the
    wide zstd batch held open as a _begin across the others"""
    z = next(f for n, f in fx.items() if n.startswith("zstd"))
    ops = [M.DecompressDevice(z), M.WindowsGroupedDevice(z), M.CompressDevice(fx[SMALL]), M.DecompressDevice(fx[SMALL]),
           M.DecompressDevice(fx["f32_wide_b128k_c2"]), M.WindowsDevice(fx["f32_wide_b128k_c2"]), M.DecompressDevice(fx["zstd_wide_u16_b160k_c2"]),
           M.WindowsGroupedDevice(fx["zstd_wide_u16_b160k_c2"]), M.DecompressDeviceSized(fx["zstd_wide_u16_b160k_c2"]),
           M.CompressDevice(fx["f32_wide_b128k_c2"]), M.DecompressDevice(fx["special6"]),
           M.WindowsStridedDevice(fx["special6"]), M.CompressDevice(fx["f32_trunc12_c2"]), M.DecompressDevice(fx["f32_trunc12_c2"]),
           M.CompressDevice(fx["blosclz_u16_b4k_c2"]), M.CompressDevice(fx["u16_clevel0_c2"]), M.DecompressDevice(fx["u16_clevel0_c2"])]
    for op in ops + [copy.copy(o) for o in ops[::-1]]:
        run.step(op)
    assert decode_stats(run)["zstd_batches"] >= 2
    zw = fx["zstd_wide_u16_b160k_c2"]
    for op in (M.CompressDevice(fx[SMALL]), M.CompressDevice(fx["f32_wide_b128k_c2"]), M.PackChunks(z), M.CompressDeviceBegin(fx["f16_tiled_b32k"])):
        run.step(M.DecompressDeviceBeginSized(zw))
        run.step(op)
        run.step(M.DecompressDeviceFetch(64))
    run.step(M.CompressDeviceFetch(fx["f16_tiled_b32k"].n))


def test_python_bindings_of_the_two_step_host_calls(fx):
    """cimg/hip.py: compress_host_begin / _fetch, compress_host_packed, compress_host_interleaved_begin, decompress_device_begin_sized"""
    f = fx[SMALL]
    e = hip.Engine(0)
    p = hip.cparams(f.ts, blocksize=1024)
    cb = e.compress_host_begin(p, f.raw, f.nbytes, f.destsize)
    assert [int(c) for c in cb] == [len(c) for c in f.chunks]
    assert e.compress_host_fetch(cb) == f.chunks
    rc, _ = e.compress_host_fetch(cb, check=False)
    assert rc == M.ERR_INVALID_PARAM
    assert e.compress_host_packed(p, f.raw, f.nbytes, f.destsize) == f.chunks
    il, npix = f.interleaved()
    rc, cb = e.compress_host_interleaved_begin(p, 2, npix, il, f.raw_off, f.nbytes, f.destsize, check=False)
    assert rc == 0 and e.compress_host_fetch(cb) == f.chunks
    rc, _ = e.compress_host_begin(hip.cparams(f.ts, compcode=hip.ZLIB), f.raw, f.nbytes, f.destsize, check=False)
    assert rc < 0
    rc, chunks = e.compress_host_packed(hip.cparams(f.ts, compcode=hip.ZLIB), f.raw, f.nbytes, f.destsize, check=False)
    assert rc < 0 and not any(chunks)
    buf, off, sizes = f.comp_layout()
    d_comp, d_raw = e.alloc(buf.size), e.alloc(f.pixels.size)
    d_comp.upload(buf)
    n = e.decompress_device_begin_sized(d_comp.ptr, off, sizes, f.nbytes, f.blocksize, d_raw.ptr, f.raw_off)
    assert not e.decompress_device_fetch(n).any() and np.array_equal(d_raw.download(), f.pixels)
    rc, n = e.decompress_device_begin_sized(d_comp.ptr, off, [sizes[0] - 1] + sizes[1:], f.nbytes, f.blocksize, d_raw.ptr, f.raw_off, check=False)
    assert rc == 0
    st = e.decompress_device_fetch(n, check=False)
    assert st[0] == M.ERR_READ_BUFFER and not st[1:].any()
    e.close()


# ---- d. seeded sequences ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_seeded_sequence(fx, lib, k):
    """150 ops drawn from the whole vocabulary (tests/_engine_model.py: seeded_sequence); a failure prints the seed, the op index and the
    last ten ops as a list to replay.  What it finds goes into (c) as a named test before it is fixed."""
    seed = int(os.environ.get("CIMG_TEST_SEED", "0")) + k
    eng = M.Eng(lib, gpu=True)
    r = M.Runner(eng, "seed %d" % seed)
    try:
        M.seeded_sequence(r, fx, np.random.default_rng(20261021 + seed), 150)
    finally:
        print("seed %d: %d ops" % (seed, len(r.log)))
        eng.close()
