"""The mantissa_bits parameter of compressed::channel<T> / image<T> / device_channel<T> / device_image<T> through C++:
tests/cpp/trunc_prec_test.cpp.  Its argument checks run against the emulator-backed mock of the C ABI (which refuses the filter itself,
so nothing more runs there); the round trips -- set_chunk, the iterator's write-back, set_region, from_* / to_* -- run on the GPU
against libcimg_hip.so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "trunc_prec_test.cpp")
EMU = os.path.join(ROOT, "tests", "emu")
FLAGS = ["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fno-strict-aliasing", "-I", os.path.join(ROOT, "include"),
         "-I", os.path.join(ROOT, "compressed-image_amd", "include")]


def _run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert "0 failures" in res.stdout


def test_argument_checks_on_emulator(tmp_path):
    subprocess.check_call(["make", "-s", "-C", EMU])
    exe = str(tmp_path / "trunc_prec_test_mock")
    mocks = [os.path.join(EMU, f) for f in ("mock_device.cpp", "mock_window.cpp", "mock_window_write.cpp")]
    subprocess.check_call(FLAGS + ["-I", os.path.join(ROOT, "compressed-image_amd", "csrc"), SRC, *mocks, "-o", exe,
                                   "-L", EMU, "-lcimg_hip_mock", "-Wl,-rpath," + EMU, "-pthread"])
    _run(exe, "checks")


@pytest.mark.gpu
def test_round_trips_on_gpu(tmp_path):
    libdir = os.path.join(ROOT, "compressed-image_amd")
    exe = str(tmp_path / "trunc_prec_test_gpu")
    subprocess.check_call(FLAGS + [SRC, "-o", exe, "-L", libdir, "-lcimg_hip", "-Wl,-rpath," + libdir, "-pthread"])
    _run(exe, "all")
