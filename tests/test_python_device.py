"""DeviceChannel / DeviceImage / DeviceArray of the `compressed_image` module (compressed/device_channel.h, device_image.h): images
kept compressed in device memory, taking and filling GPU arrays through __cuda_array_interface__.

The cases are in tests/_device_cases.py.  On the "mock" backend (the module linked against the emulator, with
tests/emu/mock_device.cpp) device memory is host memory and a few-line class exposes __cuda_array_interface__ over numpy arrays.
With the `gpu` parameter every case runs on torch tensors on the MI355X, in a child process that imports torch first, so that torch
and the module share one HIP runtime whatever this process has loaded before.
"""
import os
import subprocess
import sys

import pytest

import _device_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_mock = {}


def _run(backend, case):
    if backend == "mock":
        if not _mock:
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "emu")])
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "compressed-image_amd", "python"), "mock"])
            _mock["ci"] = D.load_module("mock")
        D.CASES[case](_mock["ci"], D.MockAdapter())
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_device_cases.py"), case], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "case %s ok" % case in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.param


def test_channel_pixels_and_regions(backend):
    _run(backend, "channel_pixels_and_regions")


def test_channel_set_region(backend):
    _run(backend, "channel_set_region")


def test_channel_host_round_trip(backend):
    _run(backend, "channel_host_round_trip")


def test_image(backend):
    _run(backend, "image")


def test_bad_arguments_raise_before_anything_runs(backend):
    _run(backend, "bad_arguments")


@pytest.mark.gpu
def test_torch_stream_and_zero_copy_result():
    _run("gpu", "gpu_stream_and_zero_copy")


@pytest.mark.gpu
def test_headline_geometry_round_trip():
    _run("gpu", "gpu_headline_geometry")
