"""dtype=, scale= and offset= of DeviceChannel / DeviceImage get_region, get_regions and get_pixels, and
DeviceImage.get_regions(interleaved=True) (`compressed_image` module over cimg_decompress_windows_typed_device), on the "mock"
backend (the module linked against the emulator, tests/emu/mock_window_typed.cpp) and on the MI355X.  Results are compared bit for
bit with numpy's two-ufunc conversion of the source pixels.  The cases are in tests/_device_cases_typed.py; with the `gpu`
parameter they run on torch tensors in a child process that imports torch first, like tests/test_python_device.py's.  On the mock
backend every typed read must make exactly one engine call, a typed one, which the mock counts."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import sysconfig

import numpy as np
import pytest

import _device_cases as D
import _device_cases_typed as S
from _device_cases_grouped import H, W, kw, probe_points

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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases_typed.py"), case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_channel_typed(backend):
    _run(backend, "channel_typed")


def test_device_image_typed(backend):
    _run(backend, "image_typed")


def test_one_typed_engine_call_per_read():
    """one typed call per read with dtype= (or interleaved get_regions), whatever the regions and channels, and no other window
    call beside it -- no scratch planes, no second pass; reads without dtype= make none"""
    ci = _load_mock()
    lib = ctypes.CDLL(ci.__file__)
    lib.mock_window_calls.restype = lib.mock_typed_window_calls.restype = ctypes.c_int64

    def calls():
        return lib.mock_window_calls(), lib.mock_typed_window_calls()

    A = D.MockAdapter()
    planes = np.stack([S.pixels(np.uint8, seed=s) for s in range(3)])
    ch = ci.DeviceChannel(A.dev(planes[0]), W, H, **kw(np.uint8))
    img = ci.DeviceImage(np.uint8, A.dev(planes), W, H, **kw(np.uint8))
    xs, ys = probe_points(64)
    for o, extra in ((ch, {}), (img, dict(interleaved=True))):
        n, t = calls()
        o.get_regions([0, 128, 256, 384, 7], [10, 10, 10, 10, 99], 128, 30, step_x=2, dtype=np.float32, scale=1 / 255, **extra)
        assert calls() == (n + 1, t + 1), type(o)
        o.get_pixels(xs, ys, dtype=np.float16)
        o.get_region(3, 4, 200, 60, dtype=np.float32, offset=-1.0, **extra)
        assert calls() == (n + 3, t + 3), type(o)
        o.get_regions([], [], 4, 4, dtype=np.float32)
        assert calls() == (n + 3, t + 3), type(o)
        o.get_regions([1, 2], [3, 4], 20, 10)
        o.get_region(3, 4, 20, 10)
        assert calls()[0] == n + 5 and calls()[1] == t + 3, type(o)
    n, t = calls()
    img.get_regions([1, 2], [3, 4], 20, 10, interleaved=True)
    assert calls() == (n + 1, t + 1)
