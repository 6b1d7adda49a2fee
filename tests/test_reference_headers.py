"""The reference's OWN host headers over this repository's C ABI.

The program is built by build() (oracle/Makefile, `ref`) into oracle/_ref/ -- the reference's headers are named on the include
path where they lie and nothing of them is copied; this test runs what was built.  tests/cpp/ref_headers_test.cpp includes the
reference's blosc2/wrapper.h, schunk.h, lazyschunk.h (+ schunk_mixin.h through them) and, in a second build, blosc2/typedefs.h +
iterators/iterator.h, compiles them against include/blosc2.h -- this repository's re-declaration of the eleven c-blosc2 symbols
the reference binds -- and links tests/emu/libcimg_hip_mock.so (the C ABI served by the host lane emulator).  It then replays the checks of the reference's
test/src/test_schunk.cpp:19-75 and the channel's chunk loop on the iterator.  <format>, which this image's libstdc++ 11 lacks, is
served by the {fmt} headers the image ships with torch (tests/cpp/compat/format).

What does NOT compile here, and why: compressed/channel.h stops at `#include "nlohmann/json.hpp"` (channel.h:12 -- a library the
image does not have; not stubbed), and with it image.h.  The seam itself -- every call the reference makes into c-blosc2 -- sits
below that line and is exercised here.  This is a test of the boundary, not an oracle: the bytes behind it are the emulator's.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref")


@pytest.mark.parametrize("with_iterator", [False, True], ids=["schunk_layer", "iterator_layer"])
def test_reference_headers_run_over_the_c_abi(with_iterator):
    exe = os.path.join(REF_BIN, "ref_headers_test_iterator" if with_iterator else "ref_headers_test")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ holds no reference build: build() found no reference checkout (oracle/Makefile, REFERENCE)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
