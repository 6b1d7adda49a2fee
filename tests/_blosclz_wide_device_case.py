"""The DeviceChannel case of tests/test_gpu_blosclz_wide.py: BloscLZ with 256 KiB blocks on torch tensors.  Run as a script, in a
process of its own that imports torch FIRST (one HIP runtime in the process: torch's), as tests/_device_cases.py does."""
import os
import sys

import torch  # noqa: F401  (first)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "compressed-image_amd"), os.path.join(ROOT, "tests")]

from _device_cases import TorchAdapter, load_module  # noqa: E402
from cimg import synth  # noqa: E402


def main():
    ci, A = load_module("gpu"), TorchAdapter()
    W, H = 1024, 600
    for dtype in (np.uint8, np.float16, np.float32):
        arr = synth.natural_channel(dtype, W, H)
        patch = synth.tiled_channel(dtype, 200, 100)
        ch = ci.DeviceChannel(A.dev(arr), W, H, compression_codec=ci.Codec.blosclz, block_size=262144)
        assert ch.block_size() == 262144
        assert np.array_equal(A.host(ch.get_decompressed()), arr), dtype
        assert np.array_equal(A.host(ch.get_region(300, 200, 400, 77)), arr[200:277, 300:700]), dtype
        # the same chunks as the host class: both are BloscLZ's bytes
        host = ci.Channel(arr, W, H, compression_codec=ci.Codec.blosclz, block_size=262144)
        assert ch.compressed_bytes() == host.compressed_bytes() and ch.num_chunks() == host.num_chunks(), dtype
        ch.set_region(50, 60, A.dev(patch))
        edited = arr.copy()
        edited[60:160, 50:250] = patch
        assert np.array_equal(A.host(ch.get_decompressed()), edited), dtype
        assert np.array_equal(A.host(ch.get_region(40, 50, 300, 200)), edited[50:250, 40:340]), dtype
    print("case ok")


if __name__ == "__main__":
    main()
