"""fill_region / fill_regions and the masked set_region / set_regions of compressed::channel<T>, image<T>, device_channel<T> and
device_image<T> through C++:
tests/cpp/masked_region_writes_test.cpp, against the emulator-backed mock of the C ABI (planner and kernel body on the emulator:
tests/emu/mock_window_write_masked.cpp) and against libcimg_hip.so on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "masked_region_writes_test.cpp")
EMU = os.path.join(ROOT, "tests", "emu")
FLAGS = ["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fno-strict-aliasing", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
         "-I", os.path.join(ROOT, "compressed-image_amd", "include")]


def _run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "\n0 failures" in res.stdout


def test_masked_region_writes_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU])
    exe = str(tmp_path / "masked_region_writes_test_mock")
    mocks = [os.path.join(EMU, f) for f in ("mock_device.cpp", "mock_window_typed.cpp", "mock_window_write_masked.cpp")]
    subprocess.check_call(FLAGS + ["-DCIMG_MOCK_BACKEND", "-I", os.path.join(ROOT, "compressed-image_amd", "csrc"), SRC, *mocks, "-o", exe,
                                   "-L", EMU, "-lcimg_hip_mock", "-Wl,-rpath," + EMU, "-pthread"])
    _run(exe)


@pytest.mark.gpu
def test_masked_region_writes_on_gpu(tmp_path):
    libdir = os.path.join(ROOT, "compressed-image_amd")
    exe = str(tmp_path / "masked_region_writes_test_gpu")
    subprocess.check_call(FLAGS + [SRC, "-o", exe, "-L", libdir, "-lcimg_hip", "-Wl,-rpath," + libdir, "-pthread"])
    _run(exe)
