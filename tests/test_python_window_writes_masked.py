"""DeviceChannel.fill_region / fill_regions and mask= / masks= of its set_region / set_regions (`compressed_image` module over
cimg_update_windows_masked_device), on the "mock" backend (the module linked against the emulator,
tests/emu/mock_window_write_masked.cpp) and on the MI355X.  Written pixels are compared bit for bit with
np.copyto(view, src_or_value, where=mask) into a copy of the pixels.  The cases are in tests/_device_cases_masked.py; with the `gpu`
parameter they run on torch tensors in a child process that imports torch first, like tests/test_python_window_writes_typed.py's.
On the mock backend every fill and every masked write must make exactly one engine call, a masked one, which the mock counts; calls
with mask=None make none."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import sysconfig

import numpy as np
import pytest

import _device_cases as D
import _device_cases_masked as S
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases_masked.py"), case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_channel_fill_and_masked_writes(backend):
    _run(backend, "channel_fill_and_masked_writes")


def test_blank_channel(backend):
    _run(backend, "blank_channel")


def test_errors(backend):
    _run(backend, "masked_errors")


def test_host_channel(backend):
    _run(backend, "host_channel")


def test_host_image(backend):
    _run(backend, "host_image")


def test_device_image(backend):
    _run(backend, "device_image")


def test_host_errors(backend):
    _run(backend, "host_errors")


def test_host_and_image_classes_make_one_masked_call_and_none_without_a_mask():
    """Channel, Image and DeviceImage: one masked engine call per fill or masked write (the three channels of these images share their
    cparams: one group); with mask=None the calls are the plain or strided ones of before"""
    ci = _load_mock()
    lib = ctypes.CDLL(ci.__file__)
    lib.mock_masked_update_calls.restype = ctypes.c_int64
    A = D.MockAdapter()
    planes = np.stack([S.pixels(np.uint8, seed=s) for s in range(3)])
    ch = ci.Channel(planes[0], W, H, **kw(np.uint8))
    img = ci.Image(np.uint8, list(planes), W, H, ["r", "g", "b"], **kw(np.uint8))
    dimg = ci.DeviceImage(np.uint8, A.dev(planes), W, H, **kw(np.uint8))
    m2, m3 = np.ones((8, 8), bool), np.ones((2, 30, 32), np.uint8)
    n = lib.mock_masked_update_calls()
    ch.fill_region(3, 4, 100, 50, 7)
    ch.set_regions([0, 128], [10, 10], np.zeros((2, 30, 32), np.uint8), step_x=2, masks=m3)
    assert lib.mock_masked_update_calls() == n + 2
    img.fill_regions([0, 128, 7], [10, 10, 99], 64, 30, [1, 2, 3], step_x=2)
    img.set_region(5, 5, [np.zeros((8, 8), np.uint8)] * 3, mask=m2)
    assert lib.mock_masked_update_calls() == n + 4
    dimg.fill_region(3, 4, 100, 50, [7, 8, 9])
    dimg.set_regions([0, 128], [10, 10], A.dev(np.zeros((2, 3, 30, 32), np.uint8)), step_x=2, masks=A.dev(m3))
    assert lib.mock_masked_update_calls() == n + 6
    ch.set_region(0, 0, np.zeros((4, 4), np.uint8), mask=None)
    ch.set_regions([1], [2], np.zeros((1, 4, 4), np.uint8), step_x=2, masks=None)
    img.set_region(0, 0, [np.zeros((4, 4), np.uint8)] * 3)
    img.set_regions([1], [2], np.zeros((1, 3, 4, 4), np.uint8))
    dimg.set_region(0, 0, A.dev(np.zeros((3, 4, 4), np.uint8)))
    dimg.set_regions([1], [2], A.dev(np.zeros((1, 3, 4, 4), np.uint8)), masks=None)
    assert lib.mock_masked_update_calls() == n + 6


def test_one_masked_engine_call_per_write_and_none_without_a_mask():
    ci = _load_mock()
    lib = ctypes.CDLL(ci.__file__)
    lib.mock_masked_update_calls.restype = ctypes.c_int64
    lib.mock_typed_update_calls.restype = ctypes.c_int64
    A = D.MockAdapter()
    ch = ci.DeviceChannel(A.dev(S.pixels(np.uint8)), W, H, **kw(np.uint8))
    n, t = lib.mock_masked_update_calls(), lib.mock_typed_update_calls()
    ch.fill_region(3, 4, 100, 50, 7)
    ch.fill_regions([0, 128, 7], [10, 10, 99], 64, 30, [1, 2, 3], step_x=2)
    ch.set_region(5, 5, A.dev(np.zeros((8, 8), np.uint8)), mask=A.dev(np.ones((8, 8), bool)))
    ch.set_regions([0, 128], [10, 10], A.dev(np.zeros((2, 30, 32), np.uint8)), step_x=2, masks=A.dev(np.ones((2, 30, 32), np.uint8)))
    assert lib.mock_masked_update_calls() == n + 4
    # mask=None: the entry points of before
    ch.set_region(0, 0, A.dev(np.zeros((4, 4), np.uint8)))
    ch.set_region(0, 0, A.dev(np.zeros((4, 4), np.uint8)), step_x=2, mask=None)
    ch.set_regions([1], [2], A.dev(np.zeros((1, 4, 4), np.uint8)), masks=None)
    ch.set_pixels([1, 2], [3, 4], A.dev(np.zeros(2, np.uint8)))
    ch[0:4, 0:4] = A.dev(np.zeros((4, 4), np.uint8))
    ch.set_region(0, 0, A.dev(np.zeros((4, 4), np.float32)), dtype=np.float32)
    assert lib.mock_masked_update_calls() == n + 4 and lib.mock_typed_update_calls() == t + 1
    ch.fill_regions([], [], 4, 4, 1)                     # nothing to do: no call
    assert lib.mock_masked_update_calls() == n + 4
