"""dtype=, scale= and offset= of DeviceChannel / DeviceImage set_region, set_regions and set_pixels, and DeviceImage's
interleaved=True (`compressed_image` module over cimg_update_windows_typed_device), on the "mock" backend (the module linked against
the emulator, tests/emu/mock_window_write_typed.cpp) and on the MI355X.  Written pixels are compared bit for bit with numpy's
conversion of the source values assigned into a copy of the pixels.  The cases are in tests/_device_cases_typed_writes.py; with the
`gpu` parameter they run on torch tensors in a child process that imports torch first, like tests/test_python_windows_typed.py's.
On the mock backend every typed write must make exactly one engine call, a typed one, which the mock counts."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import sysconfig

import numpy as np
import pytest

import _device_cases as D
import _device_cases_typed_writes as S
from _device_cases_grouped import H, W, kw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = sysconfig.get_config_var("EXT_SUFFIX")
_cache = {}


def _load_mock():
    if "mock" not in _cache:
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compressed-image_amd", "python"), "mock"])
        spec = importlib.util.spec_from_file_location("compressed_image", os.path.join(ROOT, "tests", "emu", "compressed_image" + EXT))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache["mock"] = mod
    return _cache["mock"]


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.param


def _run(backend, case):
    if backend == "mock":
        S.CASES[case](_load_mock(), D.MockAdapter())
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases_typed_writes.py"), case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_channel_typed_writes(backend):
    _run(backend, "channel_typed_writes")


def test_device_image_typed_writes(backend):
    _run(backend, "image_typed_writes")


def test_read_then_write_leaves_the_image_as_it_was(backend):
    _run(backend, "round_trip")


def test_errors(backend):
    _run(backend, "typed_write_errors")


def test_one_typed_engine_call_per_write():
    """one typed update call per write with dtype=, whatever the regions and channels; writes without dtype= make none"""
    ci = _load_mock()
    lib = ctypes.CDLL(ci.__file__)
    lib.mock_typed_update_calls.restype = ctypes.c_int64
    A = D.MockAdapter()
    planes = np.stack([S.pixels(np.uint8, seed=s) for s in range(3)])
    ch = ci.DeviceChannel(A.dev(planes[0]), W, H, **kw(np.uint8))
    img = ci.DeviceImage(np.uint8, A.dev(planes), W, H, **kw(np.uint8))
    n = lib.mock_typed_update_calls()
    ch.set_regions([0, 128, 7], [10, 10, 99], A.dev(np.zeros((3, 30, 64), np.float32)), step_x=2, dtype=np.float32, scale=1 / 255)
    assert lib.mock_typed_update_calls() == n + 1
    img.set_regions([0, 128, 7], [10, 10, 99], A.dev(np.zeros((3, 30, 64, 3), np.float16)), step_x=2, dtype=np.float16, scale=[1 / 255] * 3, interleaved=True)
    img.set_pixels([1, 2], [3, 4], A.dev(np.zeros((2, 3), np.float32)), dtype=np.float32)
    assert lib.mock_typed_update_calls() == n + 3
    ch.set_regions([], [], A.dev(np.zeros((0, 4, 4), np.float32)), dtype=np.float32)
    ch.set_region(0, 0, A.dev(np.zeros((4, 4), np.uint8)))
    img.set_regions([1], [2], A.dev(np.zeros((1, 3, 4, 4), np.uint8)))
    assert lib.mock_typed_update_calls() == n + 3
