"""Idle waves place stored planes of busy waves (encode_kernel.h: encode_emit_own), on the GPU.  The shapes are the smallest at
which it can go wrong, not the workload's: batches with far fewer items than resident waves, so that nearly every wave is a pure
helper; one block; a memcpyed chunk between regular ones; chunks off a 4-byte boundary, which helpers keep out of; and 20 chunks at
one workgroup per CU, where waves place and help while most items have not been taken.  Every batch must be the oracle's bytes,
leave the bytes behind its chunks' capacity alone and decode to the pixels -- with helpers (CIMG_ENC_HELPERS=1; they are off by
default) and with CIMG_ENC_NO_HELPERS=1.  The engine reads the switches when it is created, so each setting runs in a child process
of its own (tests/_helpers_gpu_child.py), under a time limit of its own."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_helpers_gpu_child.py")
SHAPES = ["two_chunks_of_8_blocks_ts2", "two_chunks_of_8_blocks_ts4", "one_block", "random_chunk_memcpyed", "odd_comp_off",
          "twenty_chunks_one_workgroup_per_cu"]


@pytest.mark.parametrize("helpers", ["on", "off"])
def test_helpers_on_the_gpu(helpers):
    env = {k: v for k, v in os.environ.items() if k not in ("CIMG_ENC_NO_HELPERS", "CIMG_ENC_HELPERS")}
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, _CHILD, helpers], env=env, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    for s in SHAPES:
        assert "ok " + s in r.stdout, r.stdout
    assert "done %d" % len(SHAPES) in r.stdout
