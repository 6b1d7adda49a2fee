"""Helpers of the BloscLZ wide-block tests (test_emu_blosclz_wide.py, test_gpu_blosclz_wide.py): the golden's inputs and the chunk cases."""
import hashlib
import importlib.util
import os

import numpy as np

import _oracle as O
from cimg import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_kat():
    return np.load(os.path.join(GOLDEN, "blosclz_wide_kat.npz"))


def load_stream_inputs(kat):
    """The vectors' inputs, rebuilt by the generator's own stream_inputs() and checked against the digests in the file."""
    spec = importlib.util.spec_from_file_location("make_blosclz_wide_golden", os.path.join(GOLDEN, "make_blosclz_wide_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    inputs = dict(gen.stream_inputs())
    for name, src in inputs.items():
        assert hashlib.sha256(src.tobytes()).hexdigest() == str(kat["in_sha256|" + name]), name
    return inputs


CHUNKS = {
    # name: (pixels, typesize, blocksize, splitmode, filter)
    "u8_natural_b131072": (lambda: synth.natural_channel(np.uint8, 1024, 512), 1, 131072, O.AUTO_SPLIT, O.SHUFFLE),
    "u8_natural_b262144": (lambda: synth.natural_channel(np.uint8, 1024, 512), 1, 262144, O.AUTO_SPLIT, O.SHUFFLE),
    "f16_tiled_b262144": (lambda: synth.tiled_channel(np.float16, 1024, 512), 2, 262144, O.AUTO_SPLIT, O.SHUFFLE),
    "f16_natural_b262144": (lambda: synth.natural_channel(np.float16, 1024, 512), 2, 262144, O.AUTO_SPLIT, O.SHUFFLE),
    # 65 536-byte planes: the first length the uint16 table cannot hold
    "f32_tiled_b262144": (lambda: synth.tiled_channel(np.float32, 512, 512), 4, 262144, O.AUTO_SPLIT, O.SHUFFLE),
    "f16_never_split_b262144": (lambda: synth.natural_channel(np.float16, 1024, 512), 2, 262144, O.NEVER_SPLIT, O.SHUFFLE),
    "f16_nofilter_b262144": (lambda: synth.tiled_channel(np.float16, 1024, 512), 2, 262144, O.AUTO_SPLIT, O.NOFILTER),
    # 2 * 262 144 + 70 001 bytes of float16 pixels (the last element cut in half): the never-split leftover block is one stream of
    # 70 001 bytes through the whole-block shuffle staging
    "f16_ragged_b262144": (lambda: synth.natural_channel(np.float16, 1024, 300).view(np.uint8).ravel()[:2 * 262144 + 70001], 2, 262144,
                           O.AUTO_SPLIT, O.SHUFFLE),
    "u8_noise_b262144": (lambda: np.random.Generator(np.random.PCG64(3)).integers(0, 256, 1048576, dtype=np.uint8), 1, 262144,
                         O.AUTO_SPLIT, O.SHUFFLE),
}

_made = {}


def chunk_case(name, clevel=9):
    """-> (uint8 pixels, typesize, blocksize, splitmode, filter, the oracle's chunk), computed once"""
    key = (name, clevel)
    if key not in _made:
        make, ts, blk, split, filt = CHUNKS[name]
        raw = np.ascontiguousarray(make()).view(np.uint8).ravel()
        raw.setflags(write=False)
        r, want = O.compress(O.cparams(ts, clevel=clevel, blocksize=blk, compcode=O.BLOSCLZ, splitmode=split, filters=(0, 0, 0, 0, 0, filt)), raw)
        assert r > 0 and r == len(want)
        _made[key] = (raw, ts, blk, split, filt, want)
    return _made[key]
