"""ctypes binding of libcimg_hip.so (include/cimg_hip.h + include/blosc2.h).

Plumbing for bench.py, __graft_entry__.py and the GPU tests: it only marshals pointers and sizes
into the C ABI.  There is no fallback: if the library is missing or no gfx950 device is present the
calls raise.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("CIMG_LIB") or os.path.join(_PKG, "libcimg_hip.so")   # CIMG_LIB: diagnostic builds

K_ENCODE, K_LAYOUT, K_EMIT, K_DECODE, K_DEINTERLEAVE, K_DECODE_ZSTD, K_ENCODE_ZSTD, K_ZSTD_WALK, K_ZSTD_REPLAY, K_ZSTD_FUSED, K_ZSTD_SEQ, K_ZSTD_LIT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
K_ENCODE_WIDE, K_DECODE_WIDE = 12, 13          # blocks beyond the normal kernels' LDS (csrc/wide_kernel.h)
K_ENCODE_WIDE_ZSTD, K_ZSTD_REPLAY_WIDE = 14, 15  # ... of zstd chunks
K_DECODE_WINDOW = 16                           # windows: the blocks a window meets (csrc/window_kernel.h)
K_UPDATE_PATCH, K_UPDATE_LAYOUT, K_UPDATE_EMIT = 17, 18, 19   # window writes (csrc/update_kernel.h)
K_PACK, K_INTERLEAVE = 20, 21                  # packed device storage (csrc/pack_kernel.h, csrc/interleave_kernel.h)
K_DECODE_WINDOW_STRIDED = 22                   # strided windows: the blocks that hold a sampled element (csrc/window_kernel.h)
K_TRUNC_PREC = 23                              # trunc-prec: the masked copy in front of a compress batch (csrc/trunc_kernel.h)
K_DECODE_WINDOW_GROUPED = 24                   # grouped windows: every block staged once for all its windows (csrc/window_kernel.h)
K_ENCODE_WIDE_BLOSCLZ = 25                     # BloscLZ streams beyond 65 535 bytes: the wide encoder's BloscLZ instance (csrc/wide_kernel.h)
K_UPDATE_PATCH_STRIDED = 26                    # strided window writes: the patch launch of cimg_update_windows_strided_* (csrc/update_kernel.h)
K_DECODE_WINDOW_TYPED = 27                     # typed windows: convert, scale and place each element in the launch (csrc/window_kernel.h)
K_UPDATE_PATCH_TYPED = 28                      # typed window writes: unscale, round and store each element in the patch launch (csrc/update_kernel.h)
K_UPDATE_PATCH_MASKED = 29                     # masked and constant window writes: the patch launch of cimg_update_windows_masked_* (csrc/update_kernel.h)
# names by timing id (cimg_kernel_name).  K_ENCODE times whichever of cimg_encode_streams / _blosclz the codec selects; K_DECODE
# times the pair cimg_decode_lean + cimg_decode_blocks (the second only runs for blocks the first left): bench.py reports it under
# the kernel that did the work
KERNELS = ("cimg_encode_streams", "cimg_layout_chunks", "cimg_emit_blocks", "cimg_decode_blocks", "cimg_deinterleave",
           "cimg_decode_zstd", "cimg_encode_streams_zstd", "cimg_zstd_walk", "cimg_zstd_replay", "cimg_decode_zstd_fused", "cimg_zstd_seq", "cimg_zstd_lit",
           "cimg_encode_wide", "cimg_decode_wide", "cimg_encode_wide_zstd", "cimg_zstd_replay_wide", "cimg_decode_window",
           "cimg_update_patch", "cimg_update_layout", "cimg_update_emit", "cimg_pack_chunks", "cimg_interleave", "cimg_decode_window_strided",
           "cimg_trunc_prec", "cimg_decode_window_grouped", "cimg_encode_wide_blosclz", "cimg_update_patch_strided",
           "cimg_decode_window_typed", "cimg_update_patch_typed", "cimg_update_patch_masked")
# (K_DECODE_ZSTD times the zstd read path of a batch as a whole -- cimg_zstd_walk + cimg_zstd_lit + cimg_zstd_seq + cimg_zstd_replay, and
# cimg_decode_zstd behind them for blocks the walk refused; for wide blocks, behind cimg_decode_wide: cimg_zstd_walk + cimg_zstd_replay_wide;
# the ids from K_ZSTD_WALK on time those launches one by one)
BLOSCLZ, LZ4, LZ4HC, ZLIB, ZSTD = 0, 1, 2, 4, 5
NOFILTER, SHUFFLE, BITSHUFFLE = 0, 1, 2
TRUNC_PREC = 4                                 # slot 4 only (csrc/trunc_plan.h)
MAX_OVERHEAD = 32

EXPORTS = (
    # include/cimg_hip.h
    "cimg_cparams_init", "cimg_engine_create", "cimg_engine_destroy", "cimg_last_error",
    "cimg_engine_synchronize", "cimg_engine_lock", "cimg_engine_unlock", "cimg_engine_stream", "cimg_compress_batch_device",
    "cimg_decompress_batch_device", "cimg_compress_batch_host", "cimg_decompress_batch_host", "cimg_decompress_batch_host_sized",
    "cimg_compress_batch_host_begin", "cimg_compress_batch_host_fetch", "cimg_compress_batch_host_packed",
    "cimg_deinterleave_device", "cimg_compress_batch_host_interleaved_begin",
    "cimg_compress_batch_device_begin", "cimg_compress_batch_device_fetch", "cimg_decompress_batch_device_begin", "cimg_decompress_batch_device_fetch",
    "cimg_decompress_batch_device_sized", "cimg_decompress_batch_device_begin_sized",
    "cimg_device_malloc", "cimg_device_free", "cimg_memcpy_h2d", "cimg_memcpy_d2h", "cimg_host_malloc", "cimg_host_free",
    "cimg_engine_enable_timing", "cimg_engine_reset_timing", "cimg_engine_kernel_time", "cimg_engine_kernel_samples", "cimg_engine_decode_stats", "cimg_engine_zstd_stats", "cimg_kernel_name",
    "cimg_engine_debug_stamps", "cimg_engine_read_stamps", "cimg_shared_engine", "cimg_context_cparams",
    "cimg_decompress_windows_device", "cimg_decompress_windows_host", "cimg_engine_window_stats",
    "cimg_decompress_windows_strided_device", "cimg_decompress_windows_strided_host",
    "cimg_decompress_windows_grouped_device", "cimg_decompress_windows_grouped_host", "cimg_decompress_windows_typed_device",
    "cimg_update_windows_device", "cimg_update_windows_host", "cimg_engine_update_stats",
    "cimg_update_windows_strided_device", "cimg_update_windows_strided_host", "cimg_update_windows_typed_device",
    "cimg_update_windows_masked_device", "cimg_update_windows_masked_host",
    "cimg_compress_batch_device_packed_begin", "cimg_compress_batch_device_packed_fetch", "cimg_pack_chunks_device",
    "cimg_interleave_device", "cimg_engine_wait_stream", "cimg_device_range_check",
    # include/blosc2.h
    "blosc2_create_cctx", "blosc2_create_dctx", "blosc2_free_ctx", "blosc2_compress_ctx",
    "blosc2_decompress_ctx", "blosc2_cbuffer_sizes", "blosc2_schunk_new", "blosc2_schunk_free",
    "blosc2_schunk_append_chunk", "register_filters", "print_error", "blosc2_getitem_ctx",
    "blosc2_chunk_zeros", "blosc2_chunk_nans", "blosc2_chunk_repeatval", "blosc2_chunk_uninit",
)


class CodecError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"blosc2 error {code}: {msg}")
        self.code = code


class CParams(C.Structure):
    _fields_ = [("typesize", C.c_int32), ("clevel", C.c_int32), ("blocksize", C.c_int32),
                ("compcode", C.c_int32), ("splitmode", C.c_int32),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6)]


_ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)   # cimg_alloc_fn


class Window(C.Structure):
    """cimg_window (include/cimg_hip.h)"""
    _fields_ = [("chunk_first", C.c_int32), ("chunk_count", C.c_int32), ("origin", C.c_int64), ("row_pitch", C.c_int64),
                ("width", C.c_int32), ("height", C.c_int32), ("out_off", C.c_int64), ("out_pitch", C.c_int64)]


def windows(specs):
    """dicts (or Window) with the fields of cimg_window -> a ctypes array"""
    arr = (Window * max(len(specs), 1))()
    for i, s in enumerate(specs):
        for k, v in (s.items() if isinstance(s, dict) else ((f, getattr(s, f)) for f, _ in Window._fields_)):
            setattr(arr[i], k, int(v))
    return arr


class StridedWindow(C.Structure):
    """cimg_window_strided (include/cimg_hip.h)"""
    _fields_ = [("chunk_first", C.c_int32), ("chunk_count", C.c_int32), ("origin", C.c_int64), ("row_pitch", C.c_int64),
                ("col_pitch", C.c_int64), ("width", C.c_int32), ("height", C.c_int32), ("out_off", C.c_int64), ("out_pitch", C.c_int64)]


def strided_windows(specs):
    """dicts (or StridedWindow) with the fields of cimg_window_strided -> a ctypes array (col_pitch defaults to 1)"""
    arr = (StridedWindow * max(len(specs), 1))()
    for i, s in enumerate(specs):
        arr[i].col_pitch = 1
        for k, v in (s.items() if isinstance(s, dict) else ((f, getattr(s, f)) for f, _ in StridedWindow._fields_)):
            setattr(arr[i], k, int(v))
    return arr


T_U8, T_I8, T_U16, T_I16, T_U32, T_I32, T_F16, T_F32, T_F64 = range(9)     # CIMG_T_* (include/cimg_hip.h)
_T_OF_DTYPE = {"uint8": T_U8, "int8": T_I8, "uint16": T_U16, "int16": T_I16, "uint32": T_U32, "int32": T_I32, "float16": T_F16,
               "float32": T_F32, "float64": T_F64}


def type_of(dtype):
    """the CIMG_T_* code of a numpy dtype"""
    return _T_OF_DTYPE[np.dtype(dtype).name]


class TypedWindow(C.Structure):
    """cimg_window_typed (include/cimg_hip.h)"""
    _fields_ = StridedWindow._fields_ + [("elem_pitch", C.c_int64), ("src_type", C.c_int32), ("out_type", C.c_int32),
                                         ("scale", C.c_float), ("offset", C.c_float)]


def typed_windows(specs):
    """dicts (or TypedWindow) with the fields of cimg_window_typed -> a ctypes array (col_pitch and scale default to 1)"""
    arr = (TypedWindow * max(len(specs), 1))()
    for i, s in enumerate(specs):
        arr[i].col_pitch, arr[i].scale = 1, 1.0
        for k, v in (s.items() if isinstance(s, dict) else ((f, getattr(s, f)) for f, _ in TypedWindow._fields_)):
            setattr(arr[i], k, float(v) if k in ("scale", "offset") else int(v))
    return arr


WM_CONST, WM_MASK = 1, 2                       # CIMG_WM_* (include/cimg_hip.h)


class MaskedWindow(C.Structure):
    """cimg_window_masked (include/cimg_hip.h)"""
    _fields_ = StridedWindow._fields_ + [("mask_off", C.c_int64), ("mask_pitch", C.c_int64), ("flags", C.c_int32), ("pad_", C.c_int32),
                                         ("value", C.c_uint8 * 8)]


def masked_windows(specs):
    """dicts (or MaskedWindow) with the fields of cimg_window_masked -> a ctypes array (col_pitch defaults to 1; value: up to 8 bytes)"""
    arr = (MaskedWindow * max(len(specs), 1))()
    for i, s in enumerate(specs):
        arr[i].col_pitch = 1
        for k, v in (s.items() if isinstance(s, dict) else ((f, getattr(s, f)) for f, _ in MaskedWindow._fields_)):
            if k == "value":
                for j, b in enumerate(bytes(v)[:8]):
                    arr[i].value[j] = b
            else:
                setattr(arr[i], k, int(v))
    return arr


class Blosc2CParams(C.Structure):
    _fields_ = [("compcode", C.c_uint8), ("compcode_meta", C.c_uint8), ("clevel", C.c_uint8),
                ("use_dict", C.c_int), ("typesize", C.c_int32), ("nthreads", C.c_int16),
                ("blocksize", C.c_int32), ("splitmode", C.c_int32), ("schunk", C.c_void_p),
                ("filters", C.c_uint8 * 6), ("filters_meta", C.c_uint8 * 6),
                ("prefilter", C.c_void_p), ("preparams", C.c_void_p), ("tuner_params", C.c_void_p),
                ("tuner_id", C.c_int), ("instr_codec", C.c_bool), ("codec_params", C.c_void_p),
                ("filter_params", C.c_void_p * 6)]


class Blosc2DParams(C.Structure):
    _fields_ = [("nthreads", C.c_int16), ("schunk", C.c_void_p), ("postfilter", C.c_void_p),
                ("postparams", C.c_void_p)]


_lib = None


def load():
    """dlopen the in-tree library (raises OSError if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      f"(or `make -C compressed-image_amd`)")
    L = C.CDLL(LIB_PATH)
    vp, i32p, i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.cimg_cparams_init.argtypes = [C.POINTER(CParams), C.c_int32]
    L.cimg_engine_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.cimg_engine_destroy.argtypes = [vp]
    L.cimg_last_error.argtypes = [vp]
    L.cimg_last_error.restype = C.c_char_p
    L.cimg_engine_synchronize.argtypes = [vp]
    L.cimg_engine_stream.argtypes = [vp]
    L.cimg_engine_stream.restype = vp
    L.cimg_compress_batch_device.argtypes = [vp, C.POINTER(CParams), C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.cimg_decompress_batch_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.cimg_decompress_batch_device_sized.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.cimg_decompress_batch_device_begin_sized.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.cimg_deinterleave_device.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int64, vp, C.c_int64]
    L.cimg_compress_batch_host_interleaved_begin.argtypes = [vp, C.POINTER(CParams), C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, vp, vp]
    L.cimg_compress_batch_device_begin.argtypes = [vp, C.POINTER(CParams), C.c_int32, vp, vp, vp, vp, vp, vp]
    L.cimg_compress_batch_device_fetch.argtypes = [vp, C.c_int32, vp]
    L.cimg_decompress_batch_device_begin.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.cimg_decompress_batch_device_fetch.argtypes = [vp, vp]
    L.cimg_compress_batch_host.argtypes = [vp, C.POINTER(CParams), C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.cimg_compress_batch_host_begin.argtypes = [vp, C.POINTER(CParams), C.c_int32, vp, vp, vp, vp, vp]
    L.cimg_compress_batch_host_fetch.argtypes = [vp, C.c_int32, vp, vp]
    L.cimg_compress_batch_host_packed.argtypes = [vp, C.POINTER(CParams), C.c_int32, vp, vp, vp, vp, vp, _ALLOC_FN, vp, vp]
    L.cimg_decompress_batch_host.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.cimg_decompress_batch_host_sized.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.cimg_device_malloc.argtypes = [vp, C.c_size_t]
    L.cimg_device_malloc.restype = vp
    L.cimg_device_free.argtypes = [vp, vp]
    L.cimg_host_malloc.argtypes = [C.c_size_t]
    L.cimg_host_malloc.restype = vp
    L.cimg_host_free.argtypes = [vp]
    L.cimg_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.cimg_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.cimg_engine_enable_timing.argtypes = [vp, C.c_int]
    L.cimg_engine_reset_timing.argtypes = [vp]
    L.cimg_engine_kernel_time.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.cimg_engine_kernel_samples.argtypes = [vp, C.c_int, vp, C.c_int]
    L.cimg_engine_decode_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cimg_engine_decode_stats.restype = None
    L.cimg_engine_zstd_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cimg_engine_zstd_stats.restype = None
    L.cimg_kernel_name.argtypes = [C.c_int]
    L.cimg_kernel_name.restype = C.c_char_p
    L.cimg_engine_debug_stamps.argtypes = [vp, C.c_int]
    L.cimg_engine_read_stamps.argtypes = [vp, C.c_int, vp, C.c_int]
    L.blosc2_create_cctx.argtypes = [Blosc2CParams]
    L.blosc2_create_cctx.restype = vp
    L.blosc2_create_dctx.argtypes = [Blosc2DParams]
    L.blosc2_create_dctx.restype = vp
    L.blosc2_free_ctx.argtypes = [vp]
    L.blosc2_compress_ctx.argtypes = [vp, vp, C.c_int32, vp, C.c_int32]
    L.blosc2_decompress_ctx.argtypes = [vp, vp, C.c_int32, vp, C.c_int32]
    L.blosc2_cbuffer_sizes.argtypes = [vp, i32p, i32p, i32p]
    L.print_error.argtypes = [C.c_int]
    L.cimg_decompress_windows_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.cimg_decompress_windows_host.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp]
    L.cimg_engine_window_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.cimg_decompress_windows_strided_device.argtypes = L.cimg_decompress_windows_device.argtypes
    L.cimg_decompress_windows_strided_host.argtypes = L.cimg_decompress_windows_host.argtypes
    L.cimg_decompress_windows_grouped_device.argtypes = L.cimg_decompress_windows_device.argtypes
    L.cimg_decompress_windows_grouped_host.argtypes = L.cimg_decompress_windows_host.argtypes
    if hasattr(L, "cimg_decompress_windows_typed_device"):      # (a CIMG_LIB build from before it)
        L.cimg_decompress_windows_typed_device.argtypes = L.cimg_decompress_windows_device.argtypes
    L.cimg_update_windows_device.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.cimg_update_windows_host.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, _ALLOC_FN, vp, vp, vp, vp]
    L.cimg_engine_update_stats.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4
    L.cimg_update_windows_strided_device.argtypes = L.cimg_update_windows_device.argtypes
    L.cimg_update_windows_strided_host.argtypes = L.cimg_update_windows_host.argtypes
    if hasattr(L, "cimg_update_windows_typed_device"):          # (a CIMG_LIB build from before it)
        L.cimg_update_windows_typed_device.argtypes = L.cimg_update_windows_device.argtypes
    if hasattr(L, "cimg_update_windows_masked_device"):
        L.cimg_update_windows_masked_device.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
        L.cimg_update_windows_masked_host.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, vp, _ALLOC_FN, vp, vp, vp, vp]
    L.cimg_compress_batch_device_packed_begin.argtypes = [vp, C.POINTER(CParams), C.c_int32, vp, vp, vp, vp, vp]
    L.cimg_compress_batch_device_packed_fetch.argtypes = [vp, C.c_int32, vp, vp]
    L.cimg_pack_chunks_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    L.cimg_interleave_device.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, C.c_int64, vp]
    L.cimg_engine_wait_stream.argtypes = [vp, vp]
    L.cimg_device_range_check.argtypes = [vp, vp, C.c_size_t]
    L.blosc2_getitem_ctx.argtypes = [vp, vp, C.c_int32, C.c_int, C.c_int, vp, C.c_int32]
    if hasattr(L, "blosc2_chunk_repeatval"):                # (a CIMG_LIB build from before them: a benchmark against an older library)
        for name in ("blosc2_chunk_zeros", "blosc2_chunk_nans", "blosc2_chunk_uninit"):      # host-only writers of special chunks
            getattr(L, name).argtypes = [Blosc2CParams, C.c_int32, vp, C.c_int32]
        L.blosc2_chunk_repeatval.argtypes = [Blosc2CParams, C.c_int32, vp, C.c_int32, vp]
    L.print_error.restype = C.c_char_p
    _lib = L
    return L


def cparams(typesize, clevel=9, blocksize=32768, compcode=LZ4, splitmode=3, filters=(0, 0, 0, 0, 0, SHUFFLE), trunc_prec=None):
    """trunc_prec: blosc2's trunc-prec filter in slot 4 with this int8 meta (> 0: mantissa bits kept, < 0: bits zeroed)"""
    p = CParams()
    load().cimg_cparams_init(C.byref(p), typesize)
    p.clevel, p.blocksize, p.compcode, p.splitmode = clevel, blocksize, compcode, splitmode
    for i, f in enumerate(filters):
        p.filters[i] = f
    if trunc_prec is not None:
        p.filters[4] = TRUNC_PREC
        p.filters_meta[4] = int(trunc_prec) & 0xFF
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def _i32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int32))


class DeviceBuffer:
    """A device allocation owned through the C ABI (no HIP / torch types involved)."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        self.ptr = load().cimg_device_malloc(engine.handle, self.nbytes)
        if not self.ptr:
            raise CodecError(-4, engine.last_error())
        engine._buffers.add(self)

    def upload(self, host, offset=0):
        h = np.ascontiguousarray(host).view(np.uint8).ravel()
        self.engine._check(load().cimg_memcpy_h2d(self.engine.handle, self.ptr + offset, _ptr(h), h.size))

    def download(self, nbytes=None, offset=0):
        n = self.nbytes - offset if nbytes is None else int(nbytes)
        out = np.empty(n, np.uint8)
        self.engine._check(load().cimg_memcpy_d2h(self.engine.handle, _ptr(out), self.ptr + offset, n))
        return out

    def free(self):
        # an engine that is closed first frees its buffers itself (Engine.close), so the handle is live here
        if self.ptr and self.engine.handle:
            load().cimg_device_free(self.engine.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One MI355X codec engine (stream + scratch) -- wraps cimg_engine_*."""

    def __init__(self, device=-1):
        import weakref
        self._buffers = weakref.WeakSet()
        self.handle = C.c_void_p()
        rc = load().cimg_engine_create(device, C.byref(self.handle))
        if rc != 0:
            raise CodecError(rc, load().cimg_last_error(None).decode())

    def close(self):
        if self.handle:
            for b in list(self._buffers):          # device memory goes before the engine, whatever the GC order
                b.free()
            load().cimg_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return load().cimg_last_error(self.handle).decode()

    def _check(self, rc):
        if rc < 0:
            raise CodecError(rc, self.last_error())
        return rc

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def synchronize(self):
        self._check(load().cimg_engine_synchronize(self.handle))

    # ---- device-resident batches (pointers are raw device addresses: DeviceBuffer.ptr or tensor.data_ptr()) ----
    def compress_device(self, p, d_raw, raw_off, nbytes, d_comp, comp_off, destsize):
        raw_off, comp_off, nbytes, destsize = _i64(raw_off), _i64(comp_off), _i32(nbytes), _i32(destsize)
        cbytes = np.zeros(nbytes.size, np.int32)
        self._check(load().cimg_compress_batch_device(self.handle, C.byref(p), nbytes.size, d_raw, _ptr(raw_off), _ptr(nbytes),
                                                      d_comp, _ptr(comp_off), _ptr(destsize), _ptr(cbytes)))
        return cbytes

    def decompress_device(self, d_comp, comp_off, nbytes, blocksize, d_raw, raw_off, check=True, comp_size=None):
        raw_off, comp_off, nbytes, blocksize = _i64(raw_off), _i64(comp_off), _i32(nbytes), _i32(blocksize)
        status = np.zeros(nbytes.size, np.int32)
        if comp_size is not None:       # the caller knows how many bytes each compressed buffer holds
            comp_size = _i32(comp_size)
            rc = load().cimg_decompress_batch_device_sized(self.handle, nbytes.size, d_comp, _ptr(comp_off), _ptr(comp_size), _ptr(nbytes),
                                                           _ptr(blocksize), d_raw, _ptr(raw_off), _ptr(status))
        else:
            rc = load().cimg_decompress_batch_device(self.handle, nbytes.size, d_comp, _ptr(comp_off), _ptr(nbytes), _ptr(blocksize),
                                                     d_raw, _ptr(raw_off), _ptr(status))
        if check:
            self._check(rc)
        return status

    def deinterleave_device(self, d_interleaved, nchannels, typesize, npixels, d_planar, plane_stride):
        """interleaved pixels -> one plane per channel (plane c at d_planar + c * plane_stride), enqueued on the engine's stream"""
        self._check(load().cimg_deinterleave_device(self.handle, d_interleaved, nchannels, typesize, npixels, d_planar, plane_stride))

    # the same in two steps (include/cimg_hip.h): the kernels of one compress and one decompress batch may be in flight together
    def compress_device_begin(self, p, d_raw, raw_off, nbytes, d_comp, comp_off, destsize):
        raw_off, comp_off, nbytes, destsize = _i64(raw_off), _i64(comp_off), _i32(nbytes), _i32(destsize)
        self._check(load().cimg_compress_batch_device_begin(self.handle, C.byref(p), nbytes.size, d_raw, _ptr(raw_off), _ptr(nbytes),
                                                            d_comp, _ptr(comp_off), _ptr(destsize)))
        return nbytes.size

    def compress_device_fetch(self, nchunks):
        cbytes = np.zeros(nchunks, np.int32)
        self._check(load().cimg_compress_batch_device_fetch(self.handle, nchunks, _ptr(cbytes)))
        return cbytes

    def decompress_device_begin(self, d_comp, comp_off, nbytes, blocksize, d_raw, raw_off):
        raw_off, comp_off, nbytes, blocksize = _i64(raw_off), _i64(comp_off), _i32(nbytes), _i32(blocksize)
        self._check(load().cimg_decompress_batch_device_begin(self.handle, nbytes.size, d_comp, _ptr(comp_off), _ptr(nbytes), _ptr(blocksize),
                                                              d_raw, _ptr(raw_off)))
        return nbytes.size

    def decompress_device_begin_sized(self, d_comp, comp_off, comp_size, nbytes, blocksize, d_raw, raw_off, check=True):
        """cimg_decompress_batch_device_begin_sized: _begin for callers that know how many bytes each compressed buffer holds"""
        raw_off, comp_off, comp_size, nbytes, blocksize = _i64(raw_off), _i64(comp_off), _i32(comp_size), _i32(nbytes), _i32(blocksize)
        rc = load().cimg_decompress_batch_device_begin_sized(self.handle, nbytes.size, d_comp, _ptr(comp_off), _ptr(comp_size), _ptr(nbytes),
                                                             _ptr(blocksize), d_raw, _ptr(raw_off))
        if check:
            self._check(rc)
            return nbytes.size
        return rc, nbytes.size

    def decompress_device_fetch(self, nchunks, check=True):
        status = np.zeros(nchunks, np.int32)
        rc = load().cimg_decompress_batch_device_fetch(self.handle, _ptr(status))
        if check:
            self._check(rc)
        return status

    def roundtrip_calls(self, p, d_raw, raw_off, nbytes, d_comp, comp_off, destsize, blocksize, d_out):
        """The four calls of a device-resident round trip (compress _begin, decompress _begin, both _fetch) with their arguments
        marshalled ONCE: returns step() -> cbytes.  For callers that repeat the same batch geometry (bench.py): the per-call numpy
        -> ctypes conversions of the methods above cost the host more than the C calls themselves."""
        L = load()
        raw_off, comp_off, nbytes, destsize, blocksize = _i64(raw_off), _i64(comp_off), _i32(nbytes), _i32(destsize), _i32(blocksize)
        n = int(nbytes.size)
        cbytes = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        keep = (raw_off, comp_off, nbytes, destsize, blocksize, cbytes, status, p)          # the pointers below point into these
        h, pp = self.handle, C.byref(p)
        a_raw, a_comp, a_nb, a_ds, a_bs = _ptr(raw_off), _ptr(comp_off), _ptr(nbytes), _ptr(destsize), _ptr(blocksize)
        a_cb, a_st = _ptr(cbytes), _ptr(status)
        vr, vc, vo = C.c_void_p(d_raw), C.c_void_p(d_comp), C.c_void_p(d_out)
        cb_begin, db_begin, cb_fetch, db_fetch = (L.cimg_compress_batch_device_begin, L.cimg_decompress_batch_device_begin,
                                                  L.cimg_compress_batch_device_fetch, L.cimg_decompress_batch_device_fetch)
        check = self._check

        def step(_keep=keep):
            check(cb_begin(h, pp, n, vr, a_raw, a_nb, vc, a_comp, a_ds))
            check(db_begin(h, n, vc, a_comp, a_nb, a_bs, vo, a_raw))
            check(cb_fetch(h, n, a_cb))
            check(db_fetch(h, a_st))
            return cbytes
        return step

    def stream_handle(self):
        """the engine's hipStream_t as an integer (torch.cuda.ExternalStream(handle) enqueues a caller's own kernels on it)"""
        return int(load().cimg_engine_stream(self.handle) or 0)

    def single_chunk_calls(self, p, d_work, d_comp, comp_off, chunk_bytes, destsize, blocksize):
        """get_chunk(i) / set_chunk(i) of a channel whose chunks live at d_comp + comp_off[i] (the random-access loop of the
        reference's examples/lazy_channels/main.cpp:35-52; channel.h:502-538): one device-resident decompress call of ONE chunk into
        d_work, one compress call of ONE chunk from d_work back into its slot.  Arguments marshalled once (a per-call numpy -> ctypes
        conversion costs the host more than a single-chunk launch).  set_chunk returns the chunk's new compressed size."""
        L = load()
        comp_off = _i64(comp_off)
        n = int(comp_off.size)
        zero = _i64([0]); nb = _i32([chunk_bytes]); ds = _i32([destsize]); bs = _i32([blocksize])
        cb = np.zeros(1, np.int32); st = np.zeros(1, np.int32)
        keep = (comp_off, zero, nb, ds, bs, cb, st, p)
        h, pp = self.handle, C.byref(p)
        base = comp_off.ctypes.data
        a_zero, a_nb, a_ds, a_bs, a_cb, a_st = _ptr(zero), _ptr(nb), _ptr(ds), _ptr(bs), _ptr(cb), _ptr(st)
        vw, vc = C.c_void_p(d_work), C.c_void_p(d_comp)
        dec, enc, check = L.cimg_decompress_batch_device, L.cimg_compress_batch_device, self._check

        def get_chunk(i, _keep=keep):
            check(dec(h, 1, vc, C.c_void_p(base + 8 * i), a_nb, a_bs, vw, a_zero, a_st))

        def set_chunk(i, _keep=keep):
            check(enc(h, pp, 1, vw, a_zero, a_nb, vc, C.c_void_p(base + 8 * i), a_ds, a_cb))
            return int(cb[0])
        assert n > 0
        return get_chunk, set_chunk

    # ---- host-resident batches ----
    def compress_host(self, p, raw, nbytes, destsize):
        """raw: numpy array holding the chunks back to back.  Returns list of chunk bytes (b'' = does not fit)."""
        raw = np.ascontiguousarray(raw).view(np.uint8).ravel()
        nbytes, destsize = _i32(nbytes), _i32(destsize)
        raw_off = _i64(np.concatenate([[0], np.cumsum(nbytes[:-1], dtype=np.int64)]))
        stride = int(destsize.max()) + 32
        comp_off = _i64(np.arange(nbytes.size, dtype=np.int64) * stride)
        comp = np.zeros(stride * nbytes.size, np.uint8)
        cbytes = np.zeros(nbytes.size, np.int32)
        self._check(load().cimg_compress_batch_host(self.handle, C.byref(p), nbytes.size, _ptr(raw), _ptr(raw_off), _ptr(nbytes),
                                                    _ptr(comp), _ptr(comp_off), _ptr(destsize), _ptr(cbytes)))
        return [comp[o:o + max(c, 0)].tobytes() for o, c in zip(comp_off, cbytes)]

    # the same in two steps, in one call into the caller's allocator, and from interleaved pixels (include/cimg_hip.h); with
    # check=False each returns its return code first and raises nothing
    def compress_host_begin(self, p, raw, nbytes, destsize, check=True):
        """cimg_compress_batch_host_begin: the chunks stay in the engine's staging area.  Returns cbytes."""
        raw = np.ascontiguousarray(raw).view(np.uint8).ravel()
        nbytes, destsize = _i32(nbytes), _i32(destsize)
        raw_off = _i64(np.concatenate([[0], np.cumsum(nbytes[:-1], dtype=np.int64)]))
        cbytes = np.zeros(nbytes.size, np.int32)
        rc = load().cimg_compress_batch_host_begin(self.handle, C.byref(p), nbytes.size, _ptr(raw), _ptr(raw_off), _ptr(nbytes), _ptr(destsize),
                                                   _ptr(cbytes))
        if check:
            self._check(rc)
            return cbytes
        return rc, cbytes

    def compress_host_fetch(self, cbytes, check=True):
        """cimg_compress_batch_host_fetch of the batch whose _begin reported `cbytes`.  Returns list of chunk bytes (b'' = did not fit)."""
        cbytes = _i32(cbytes)
        room = np.maximum(cbytes, 0).astype(np.int64) + 64
        comp_off = _i64(np.concatenate([[0], np.cumsum(room[:-1])]))
        comp = np.zeros(int(room.sum()), np.uint8)
        rc = load().cimg_compress_batch_host_fetch(self.handle, cbytes.size, _ptr(comp), _ptr(comp_off))
        chunks = [comp[o:o + max(c, 0)].tobytes() for o, c in zip(comp_off, cbytes)]
        if check:
            self._check(rc)
            return chunks
        return rc, chunks

    def compress_host_packed(self, p, raw, nbytes, destsize, check=True):
        """cimg_compress_batch_host_packed with an allocator that hands out plain host memory.  Returns list of chunk bytes."""
        raw = np.ascontiguousarray(raw).view(np.uint8).ravel()
        nbytes, destsize = _i32(nbytes), _i32(destsize)
        raw_off = _i64(np.concatenate([[0], np.cumsum(nbytes[:-1], dtype=np.int64)]))
        cbytes = np.zeros(nbytes.size, np.int32)
        ptrs = (C.c_void_p * max(nbytes.size, 1))()
        keep = []

        def alloc(_user, n):
            b = C.create_string_buffer(max(int(n), 1))
            keep.append(b)
            return C.addressof(b)
        rc = load().cimg_compress_batch_host_packed(self.handle, C.byref(p), nbytes.size, _ptr(raw), _ptr(raw_off), _ptr(nbytes), _ptr(destsize),
                                                    _ptr(cbytes), _ALLOC_FN(alloc), None, ptrs)
        chunks = [C.string_at(ptrs[i], int(cbytes[i])) if rc == 0 and ptrs[i] and cbytes[i] > 0 else b"" for i in range(nbytes.size)]
        if check:
            self._check(rc)
            return chunks
        return rc, chunks

    def compress_host_interleaved_begin(self, p, nchannels, npixels, interleaved, raw_off, nbytes, destsize, check=True):
        """cimg_compress_batch_host_interleaved_begin: raw_off / nbytes address the PLANAR layout (channel c at c * plane_stride,
        plane_stride = npixels * typesize rounded up to 16).  Returns cbytes; compress_host_fetch delivers the chunks."""
        il = np.ascontiguousarray(interleaved).view(np.uint8).ravel()
        raw_off, nbytes, destsize = _i64(raw_off), _i32(nbytes), _i32(destsize)
        cbytes = np.zeros(nbytes.size, np.int32)
        rc = load().cimg_compress_batch_host_interleaved_begin(self.handle, C.byref(p), nchannels, npixels, _ptr(il), nbytes.size, _ptr(raw_off),
                                                               _ptr(nbytes), _ptr(destsize), _ptr(cbytes))
        if check:
            self._check(rc)
            return cbytes
        return rc, cbytes

    def decompress_host(self, chunks, check=True):
        """chunks: list of bytes.  Returns (list of uint8 arrays, status array)."""
        sizes = [len(c) for c in chunks]
        comp_off = _i64(np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.int64)]))
        comp = np.frombuffer(b"".join(chunks), np.uint8)
        nb = _i32([int.from_bytes(c[4:8], "little", signed=True) for c in chunks])
        raw_off = _i64(np.concatenate([[0], np.cumsum(nb[:-1], dtype=np.int64)]))
        raw = np.zeros(max(int(nb.sum()), 1), np.uint8)
        status = np.zeros(nb.size, np.int32)
        held = _i32(sizes)
        rc = load().cimg_decompress_batch_host_sized(self.handle, nb.size, _ptr(comp), _ptr(comp_off), _ptr(held), _ptr(raw), _ptr(raw_off),
                                                     _ptr(nb), _ptr(status))
        if check:
            self._check(rc)
        return [raw[o:o + n] for o, n in zip(raw_off, nb)], status

    # ---- packed device storage (include/cimg_hip.h) ----
    def compress_device_packed_begin(self, p, d_raw, raw_off, nbytes, destsize):
        """compress device-resident pixels into the engine's staging area; returns cbytes (the sizes _fetch will move)"""
        raw_off, nbytes, destsize = _i64(raw_off), _i32(nbytes), _i32(destsize)
        cbytes = np.zeros(nbytes.size, np.int32)
        self._check(load().cimg_compress_batch_device_packed_begin(self.handle, C.byref(p), nbytes.size, d_raw, _ptr(raw_off), _ptr(nbytes),
                                                                   _ptr(destsize), _ptr(cbytes)))
        return cbytes

    def compress_device_packed_fetch(self, nchunks, d_dst, dst_off):
        dst_off = _i64(dst_off)
        self._check(load().cimg_compress_batch_device_packed_fetch(self.handle, nchunks, d_dst, _ptr(dst_off)))

    def pack_chunks_device(self, d_src, nbytes, d_dst, dst_off):
        """d_src: device ADDRESSES of the pieces (a host list); piece i (nbytes[i] bytes) goes to d_dst + dst_off[i]"""
        src = np.ascontiguousarray(np.asarray(d_src, dtype=np.uint64))
        nbytes, dst_off = _i32(nbytes), _i64(dst_off)
        self._check(load().cimg_pack_chunks_device(self.handle, nbytes.size, _ptr(src), _ptr(nbytes), d_dst, _ptr(dst_off)))

    def interleave_device(self, d_planar, plane_stride, nchannels, typesize, npixels, d_interleaved):
        """one plane per channel (plane c at d_planar + c * plane_stride) -> interleaved pixels"""
        self._check(load().cimg_interleave_device(self.handle, d_planar, plane_stride, nchannels, typesize, npixels, d_interleaved))

    def wait_stream(self, stream=None):
        """the engine's stream waits for what `stream` (an integer hipStream_t; None: the null stream) holds now"""
        self._check(load().cimg_engine_wait_stream(self.handle, stream))

    def device_range_check(self, ptr, nbytes):
        """0 if [ptr, ptr + nbytes) is memory of the engine's device inside one allocation, else the (negative) error code"""
        return load().cimg_device_range_check(self.handle, ptr, nbytes)

    # ---- windows (include/cimg_hip.h: cimg_window) ----
    def decompress_windows_device(self, d_comp, comp_off, nbytes, blocksize, typesize, specs, d_out, comp_size=None, check=True,
                                  strided=False, grouped=False):
        """windows of device-resident chunks into device memory at d_out; returns the per-chunk status.  strided: the specs are
        cimg_window_strided (with col_pitch) and go through cimg_decompress_windows_strided_device; grouped: the same specs
        through cimg_decompress_windows_grouped_device (every block staged once)"""
        comp_off, nbytes, blocksize = _i64(comp_off), _i32(nbytes), _i32(blocksize)
        cs = _i32(comp_size) if comp_size is not None else None
        w = strided_windows(specs) if strided or grouped else windows(specs)
        status = np.zeros(nbytes.size, np.int32)
        fn = load().cimg_decompress_windows_strided_device if strided else load().cimg_decompress_windows_device
        if grouped:
            fn = load().cimg_decompress_windows_grouped_device
        rc = fn(self.handle, nbytes.size, d_comp, _ptr(comp_off), _ptr(cs) if cs is not None else None, _ptr(nbytes), _ptr(blocksize), typesize,
                len(specs), w, d_out, _ptr(status))
        if check:
            self._check(rc)
        return status if check else (rc, status)

    def decompress_windows_typed_device(self, d_comp, comp_off, nbytes, blocksize, typesize, specs, d_out, comp_size=None, check=True):
        """typed windows (cimg_window_typed specs: elem_pitch, src_type, out_type, scale, offset) of device-resident chunks into
        device memory at d_out through cimg_decompress_windows_typed_device; returns the per-chunk status"""
        comp_off, nbytes, blocksize = _i64(comp_off), _i32(nbytes), _i32(blocksize)
        cs = _i32(comp_size) if comp_size is not None else None
        status = np.zeros(nbytes.size, np.int32)
        rc = load().cimg_decompress_windows_typed_device(self.handle, nbytes.size, d_comp, _ptr(comp_off), _ptr(cs) if cs is not None else None,
                                                         _ptr(nbytes), _ptr(blocksize), typesize, len(specs), typed_windows(specs), d_out,
                                                         _ptr(status))
        if check:
            self._check(rc)
        return status if check else (rc, status)

    def decompress_windows_host(self, chunks, specs, out, check=True, strided=False, grouped=False):
        """chunks: list of bytes; out: a writable uint8 numpy array the windows' out_off / out_pitch point into.  strided: the
        specs are cimg_window_strided and go through cimg_decompress_windows_strided_host; grouped: through
        cimg_decompress_windows_grouped_host"""
        sizes = [len(c) for c in chunks]
        comp_off = _i64(np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.int64)]))
        comp = np.frombuffer(b"".join(chunks) + bytes(16), np.uint8)
        held = _i32(sizes)
        w = strided_windows(specs) if strided or grouped else windows(specs)
        status = np.zeros(len(chunks), np.int32)
        assert out.dtype == np.uint8 and out.flags.c_contiguous
        fn = load().cimg_decompress_windows_strided_host if strided else load().cimg_decompress_windows_host
        if grouped:
            fn = load().cimg_decompress_windows_grouped_host
        rc = fn(self.handle, len(chunks), _ptr(comp), _ptr(comp_off), _ptr(held), len(specs), w, _ptr(out), _ptr(status))
        if check:
            self._check(rc)
        return status if check else (rc, status)

    # ---- window writes (include/cimg_hip.h: cimg_update_windows_*) ----
    def update_windows_strided_device(self, p, d_comp, comp_off, nbytes, blocksize, destsize, specs, d_src, d_new, new_off, comp_size=None,
                                      check=True):
        """update_windows_device over cimg_window_strided specs (with col_pitch): cimg_update_windows_strided_device"""
        return self.update_windows_device(p, d_comp, comp_off, nbytes, blocksize, destsize, specs, d_src, d_new, new_off, comp_size, check,
                                          strided=True)

    def update_windows_typed_device(self, p, d_comp, comp_off, nbytes, blocksize, destsize, specs, d_src, d_new, new_off, comp_size=None,
                                    check=True, new_cbytes=None, status=None):
        """typed windows (cimg_window_typed specs; out_off / out_pitch / elem_pitch / out_type describe the SOURCE at d_src) converted
        and written into device-resident chunks through cimg_update_windows_typed_device.  Returns as update_windows_device does;
        new_cbytes / status: int32 arrays to hand to the call in place of fresh zeros."""
        comp_off, nbytes, blocksize, destsize, new_off = _i64(comp_off), _i32(nbytes), _i32(blocksize), _i32(destsize), _i64(new_off)
        cs = _i32(comp_size) if comp_size is not None else None
        status = np.zeros(nbytes.size, np.int32) if status is None else status
        ncb = np.zeros(nbytes.size, np.int32) if new_cbytes is None else new_cbytes
        rc = load().cimg_update_windows_typed_device(self.handle, C.byref(p), nbytes.size, d_comp, _ptr(comp_off),
                                                     _ptr(cs) if cs is not None else None, _ptr(nbytes), _ptr(blocksize), _ptr(destsize),
                                                     len(specs), typed_windows(specs), d_src, d_new, _ptr(new_off), _ptr(ncb), _ptr(status))
        if check:
            self._check(rc)
            return ncb, status
        return rc, ncb, status

    def update_windows_masked_device(self, p, d_comp, comp_off, nbytes, blocksize, destsize, specs, d_src, d_mask, d_new, new_off,
                                     comp_size=None, check=True, new_cbytes=None, status=None):
        """masked / constant windows (cimg_window_masked specs; d_src may be None when every window is constant, d_mask when none is
        masked) written into device-resident chunks through cimg_update_windows_masked_device.  Returns as update_windows_device
        does; new_cbytes / status: int32 arrays to hand to the call in place of fresh zeros."""
        comp_off, nbytes, blocksize, destsize, new_off = _i64(comp_off), _i32(nbytes), _i32(blocksize), _i32(destsize), _i64(new_off)
        cs = _i32(comp_size) if comp_size is not None else None
        status = np.zeros(nbytes.size, np.int32) if status is None else status
        ncb = np.zeros(nbytes.size, np.int32) if new_cbytes is None else new_cbytes
        rc = load().cimg_update_windows_masked_device(self.handle, C.byref(p), nbytes.size, d_comp, _ptr(comp_off),
                                                      _ptr(cs) if cs is not None else None, _ptr(nbytes), _ptr(blocksize), _ptr(destsize),
                                                      len(specs), masked_windows(specs), d_src, d_mask, d_new, _ptr(new_off), _ptr(ncb),
                                                      _ptr(status))
        if check:
            self._check(rc)
            return ncb, status
        return rc, ncb, status

    def update_windows_masked_host(self, p, chunks, destsize, specs, src, mask, check=True, new_cbytes=None, status=None):
        """update_windows_host over cimg_window_masked specs: cimg_update_windows_masked_host (src / mask: uint8 arrays or None)"""
        sizes = [len(c) for c in chunks]
        comp_off = _i64(np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.int64)]))
        comp = np.frombuffer(b"".join(chunks) + bytes(16), np.uint8)
        held, destsize = _i32(sizes), _i32(destsize)
        n = len(chunks)
        status = np.zeros(n, np.int32) if status is None else status
        ncb = np.zeros(n, np.int32) if new_cbytes is None else new_cbytes
        ptrs = (C.c_void_p * max(n, 1))()
        keep = []

        def alloc(_user, nbytes):
            b = C.create_string_buffer(max(int(nbytes), 1))
            keep.append(b)
            return C.addressof(b)
        cb = _ALLOC_FN(alloc)
        src = None if src is None else np.ascontiguousarray(src).view(np.uint8)
        mask = None if mask is None else np.ascontiguousarray(mask).view(np.uint8)
        rc = load().cimg_update_windows_masked_host(self.handle, C.byref(p), n, _ptr(comp), _ptr(comp_off), _ptr(held), _ptr(destsize),
                                                    len(specs), masked_windows(specs), None if src is None else _ptr(src),
                                                    None if mask is None else _ptr(mask), cb, None, ptrs, _ptr(ncb), _ptr(status))
        new = [C.string_at(ptrs[i], int(ncb[i])) if ptrs[i] and ncb[i] > 0 else None for i in range(n)]
        if check:
            self._check(rc)
            return new, status
        return rc, new, status

    def update_windows_strided_host(self, p, chunks, destsize, specs, src, check=True):
        """update_windows_host over cimg_window_strided specs: cimg_update_windows_strided_host"""
        return self.update_windows_host(p, chunks, destsize, specs, src, check, strided=True)

    def update_windows_device(self, p, d_comp, comp_off, nbytes, blocksize, destsize, specs, d_src, d_new, new_off, comp_size=None,
                              check=True, strided=False):
        """windows of d_src written into device-resident chunks; the touched chunks' new forms go to d_new + new_off[i].
        Returns (new_cbytes, status) (with check=False: (rc, new_cbytes, status))."""
        comp_off, nbytes, blocksize, destsize, new_off = _i64(comp_off), _i32(nbytes), _i32(blocksize), _i32(destsize), _i64(new_off)
        cs = _i32(comp_size) if comp_size is not None else None
        w = strided_windows(specs) if strided else windows(specs)
        status = np.zeros(nbytes.size, np.int32)
        ncb = np.zeros(nbytes.size, np.int32)
        fn = load().cimg_update_windows_strided_device if strided else load().cimg_update_windows_device
        rc = fn(self.handle, C.byref(p), nbytes.size, d_comp, _ptr(comp_off), _ptr(cs) if cs is not None else None, _ptr(nbytes),
                _ptr(blocksize), _ptr(destsize), len(specs), w, d_src, d_new, _ptr(new_off), _ptr(ncb), _ptr(status))
        if check:
            self._check(rc)
            return ncb, status
        return rc, ncb, status

    def update_windows_host(self, p, chunks, destsize, specs, src, check=True, strided=False):
        """chunks: list of bytes; src: a uint8 numpy array the windows' out_off / out_pitch point into.  Returns (list of new chunk
        bytes, None where untouched, status) (with check=False: (rc, new chunks, status))."""
        sizes = [len(c) for c in chunks]
        comp_off = _i64(np.concatenate([[0], np.cumsum(sizes[:-1], dtype=np.int64)]))
        comp = np.frombuffer(b"".join(chunks) + bytes(16), np.uint8)
        held, destsize = _i32(sizes), _i32(destsize)
        w = strided_windows(specs) if strided else windows(specs)
        n = len(chunks)
        status = np.zeros(n, np.int32)
        ncb = np.zeros(n, np.int32)
        ptrs = (C.c_void_p * max(n, 1))()
        keep = []

        def alloc(_user, nbytes):
            b = C.create_string_buffer(max(int(nbytes), 1))
            keep.append(b)
            return C.addressof(b)
        cb = _ALLOC_FN(alloc)
        src = np.ascontiguousarray(src).view(np.uint8)
        fn = load().cimg_update_windows_strided_host if strided else load().cimg_update_windows_host
        rc = fn(self.handle, C.byref(p), n, _ptr(comp), _ptr(comp_off), _ptr(held), _ptr(destsize), len(specs), w, _ptr(src), cb, None, ptrs,
                _ptr(ncb), _ptr(status))
        new = [C.string_at(ptrs[i], int(ncb[i])) if ptrs[i] else None for i in range(n)]
        if check:
            self._check(rc)
            return new, status
        return rc, new, status

    def update_stats(self):
        v = [C.c_int64(0) for _ in range(4)]
        load().cimg_engine_update_stats(self.handle, *[C.byref(x) for x in v])
        return {"blocks_decoded": v[0].value, "blocks_encoded": v[1].value, "chunks_whole": v[2].value, "bytes_uploaded": v[3].value}

    def window_stats(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        load().cimg_engine_window_stats(self.handle, C.byref(a), C.byref(b), C.byref(c))
        return {"blocks_decoded": a.value, "chunks_whole": b.value, "comp_bytes_uploaded": c.value}

    # ---- timing ----
    def enable_timing(self, on=True):
        """on: False/0 off, True/1 every batch call, n > 1 every n-th batch call."""
        load().cimg_engine_enable_timing(self.handle, int(on))

    def reset_timing(self):
        load().cimg_engine_reset_timing(self.handle)

    def debug_stamps(self, on=True):
        load().cimg_engine_debug_stamps(self.handle, 1 if on else 0)

    def read_stamps(self, which, max_workgroups=1 << 20):
        out = np.zeros((max_workgroups, 16), np.uint64)
        n = self._check(load().cimg_engine_read_stamps(self.handle, which, _ptr(out), max_workgroups))
        return out[:n]

    def kernel_time(self, kernel):
        ms, n = C.c_double(0), C.c_int64(0)
        self._check(load().cimg_engine_kernel_time(self.handle, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_samples(self, kernel, max_samples=65536):
        """milliseconds of every timed launch of `kernel` since reset_timing(), oldest first"""
        out = np.zeros(max_samples, np.float32)
        n = load().cimg_engine_kernel_samples(self.handle, kernel, _ptr(out), max_samples)
        if n < 0:
            self._check(n)
        return out[:n].copy()

    def decode_stats(self):
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        load().cimg_engine_decode_stats(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return {"lean_batches": a.value, "blocks_left_to_general": b.value, "blocks_total": c.value, "zstd_batches": d.value}

    def zstd_stats(self):
        a, b = C.c_int64(0), C.c_int64(0)
        load().cimg_engine_zstd_stats(self.handle, C.byref(a), C.byref(b))
        return {"zstd_batches": a.value, "blocks_refused": b.value}


def cbuffer_sizes(chunk):
    c = np.frombuffer(bytes(chunk[:32]), np.uint8)
    a, b, d = C.c_int32(), C.c_int32(), C.c_int32()
    rc = load().blosc2_cbuffer_sizes(_ptr(c), C.byref(a), C.byref(b), C.byref(d))
    if rc < 0:
        raise CodecError(rc, load().print_error(rc).decode())
    return a.value, b.value, d.value
