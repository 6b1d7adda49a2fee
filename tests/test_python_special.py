"""DeviceChannel.full / zeros / full_like / zeros_like of the `compressed_image` module: blank channels made of blosc2 special-value
chunks (compressed/device_channel.h: full), 64 bytes of device memory a chunk until set_region paints into them.

The cases are in tests/_device_cases_special.py.  On the "mock" backend (the module linked against the emulator, device memory is
host memory) they run in this process; the GPU case runs in tests/test_gpu_special_chunks.py, in a child process that imports torch
first."""
import os
import subprocess

import pytest

import _device_cases as D
import _device_cases_special as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_mock = {}


def _module():
    if not _mock:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compressed-image_amd", "python"), "mock"])
        _mock["ci"] = D.load_module("mock")
    return _mock["ci"]


@pytest.mark.parametrize("case", ["full_reads", "full_set_region", "full_host_round_trip", "full_mantissa"])
def test_blank_channels_on_the_mock_device(case):
    S.CASES[case](_module(), D.MockAdapter())
