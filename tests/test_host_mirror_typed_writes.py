"""Typed region writes of compressed::device_channel<T> / device_image<T> through C++: tests/cpp/typed_region_writes_test.cpp, against
the emulator-backed mock of the C ABI (planner and kernel body on the emulator: tests/emu/mock_window_write_typed.cpp) and against
libcimg_hip.so on the GPU.  Built with -ffp-contract=off: the test's own expectation is a difference rounded before the quotient."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "typed_region_writes_test.cpp")
EMU = os.path.join(ROOT, "tests", "emu")
FLAGS = ["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fno-strict-aliasing", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
         "-I", os.path.join(ROOT, "compressed-image_amd", "include")]


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "\n0 failures" in res.stdout


def test_typed_region_writes_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU])
    exe = str(tmp_path / "typed_region_writes_test_mock")
    mocks = [os.path.join(EMU, f) for f in ("mock_device.cpp", "mock_window_typed.cpp", "mock_window_write_typed.cpp")]
    subprocess.check_call(FLAGS + ["-DCIMG_MOCK_BACKEND", "-I", os.path.join(ROOT, "compressed-image_amd", "csrc"), SRC, *mocks, "-o", exe,
                                   "-L", EMU, "-lcimg_hip_mock", "-Wl,-rpath," + EMU, "-pthread"])
    _run(exe)


@pytest.mark.gpu
def test_typed_region_writes_on_gpu(tmp_path):
    libdir = os.path.join(ROOT, "compressed-image_amd")
    exe = str(tmp_path / "typed_region_writes_test_gpu")
    subprocess.check_call(FLAGS + [SRC, "-o", exe, "-L", libdir, "-lcimg_hip", "-Wl,-rpath," + libdir, "-pthread"])
    _run(exe)
