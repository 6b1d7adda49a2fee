"""The call-sequence vocabulary on a machine without a GPU: PendingModel against a table transcribed from include/cimg_hip.h, and the
runner of tests/_engine_model.py over the mock library (tests/emu/libcimg_hip_mock_full.so: the host batch family, the packed pair,
pack, interleave and deinterleave, the sized device decode, the window reads and writes -- what tests/emu/mock_*.cpp serve).  This leg
proves the ops, their expected values and the model; tests/test_gpu_engine_sequences.py runs the same on the engine.

What is checked on the mock: every op's results against the oracle, and the staging-area rules (the mock keeps its own record of the
staged batch, tests/emu/mock_cabi.cpp).  The host mirror and the Python CPU tests trust the mock to behave like the engine there.
"""
import copy
import os

import numpy as np
import pytest

import _engine_model as M


@pytest.fixture(scope="module")
def fx(golden_dir):
    return M.fixtures(golden_dir)


@pytest.fixture(scope="module")
def lib():
    return M.mock_library()


@pytest.fixture
def run(lib):
    eng = M.Eng(lib, gpu=False)
    yield M.Runner(eng)
    eng.close()


# ---- the model against the header -------------------------------------------------------------------------------------------------
class _Fx:
    def __init__(self, n):
        self.n, self.name = n, "n%d" % n


def _op(begins=None, fetches=None, voids=(), n=3, count=None, accepted=True):
    op = M.Op(_Fx(n))
    op.begins, op.fetches, op.voids, op.count, op.accepted = begins, fetches, voids, count, accepted
    return op


# (what lies between a _begin and its _fetch, the slot, does the header say the _fetch succeeds) -- include/cimg_hip.h, line by line
HEADER_TABLE = [
    # h:92 one compress and one decompress batch in flight together; h:96 a plain call of the same kind in between invalidates
    ("nothing", "enc", (), True),
    ("a decompress _begin and its _fetch", "enc", ("dec_begin", "dec_fetch"), True),
    ("a plain decompress call", "enc", (("dec",),), True),
    ("a plain compress call", "enc", (("enc",),), False),
    ("a plain compress call", "dec", (("enc",),), True),
    ("a plain decompress call", "dec", (("dec",),), False),
    # h:207-209 window reads void a pending decompress _begin; the host form the staged batch as well
    ("a device window read", "dec", (("dec",),), False),
    ("a device window read", "staged", (("dec",),), True),
    ("a host window read", "staged", (("dec", "staged"),), False),
    ("a host window read", "enc", (("dec", "staged"),), True),
    # h:159-168 (corrected) / h:432-436: only calls that reuse the staging area void the staged batch
    ("a plain device compress call", "staged", (("enc",),), True),
    ("a host decompress call", "staged", (("dec", "staged"),), False),
    ("a host compress call", "staged", (("enc", "staged"),), False),
    ("a host compress call", "enc", (("enc", "staged"),), False),
    ("a host decompress call", "dec", (("dec", "staged"),), False),
    # h:319-321 window writes decode and encode
    ("a device window write", "enc", (("enc", "dec"),), False),
    ("a device window write", "dec", (("enc", "dec"),), False),
    ("a device window write", "staged", (("enc", "dec"),), True),
    # h:104-105 calls that do neither
    ("interleave, pack, timing", "enc", ((),), True),
    ("interleave, pack, timing", "dec", ((),), True),
    ("interleave, pack, timing", "staged", ((),), True),
]


@pytest.mark.parametrize("what,slot,between,ok", HEADER_TABLE, ids=["%s then %s" % (r[1], r[0]) for r in HEADER_TABLE])
def test_model_says_what_the_header_says(what, slot, between, ok):
    m = M.PendingModel()
    begin = _op(begins=slot)
    assert m.apply(begin) is None
    for b in between:
        if b == "dec_begin":
            m.apply(_op(begins="dec"))
        elif b == "dec_fetch":
            assert m.apply(_op(fetches="dec")).ok
        else:
            assert m.apply(_op(voids=b)) is None
    v = m.apply(_op(fetches=slot, count=None if slot == "dec" else 3))
    assert v.ok == ok and (v.begin is begin) == ok


def test_model_fetch_rules():
    m = M.PendingModel()
    assert not m.apply(_op(fetches="enc", count=3)).ok              # never begun
    first, second = _op(begins="staged", n=3), _op(begins="staged", n=5)
    m.apply(first)
    m.apply(second)                                                 # h:159: the most recent _begin
    assert not m.apply(_op(fetches="staged", count=3)).ok           # the wrong count fails ...
    v = m.apply(_op(fetches="staged", count=5))                     # ... and leaves the batch pending
    assert v.ok and v.begin is second
    assert not m.apply(_op(fetches="staged", count=5)).ok           # delivered once
    m.apply(_op(begins="enc"))
    m.apply(_op(begins="enc", voids=("enc",), accepted=False))      # a _begin that is refused voids the earlier one and opens nothing
    assert not m.apply(_op(fetches="enc", count=3)).ok
    m.apply(_op(begins="enc"))
    m.apply(_op(begins="dec"))
    assert m.apply(_op(fetches="dec")).ok and m.apply(_op(fetches="enc", count=3)).ok      # either order
    m.apply(_op(begins="enc"))
    m.apply(_op(begins="dec"))
    assert m.apply(_op(fetches="enc", count=3)).ok and m.apply(_op(fetches="dec")).ok


# ---- the vocabulary on the mock ---------------------------------------------------------------------------------------------------
def _fixture_names():
    return ["u16_b256_c1", "f32_b1k_c3", "u16_b4k_c40", "f16_tiled_b32k", "f16_natural_b32k", "blosclz_u16_b4k_c2", "u8_unsplit_b4k_c3",
            "zstd", "u16_clevel0_c2", "special6", "f32_trunc12_c2"]


def _named(fx, name):
    return next(f for n, f in fx.items() if n.startswith(name))


@pytest.mark.parametrize("name", _fixture_names())
def test_every_op_alone_gives_the_oracles_result(fx, lib, name):
    """every op class that fits the fixture, one after the other on one engine: the expected-value code of the whole vocabulary"""
    f = _named(fx, name)
    eng = M.Eng(lib, gpu=False)
    r = M.Runner(eng, name)
    ran = 0
    for cls in M.COMPRESS_OPS + M.DECOMPRESS_OPS + (M.PackChunks, M.Deinterleave, M.Interleave) + M.READ_OPS + M.WRITE_OPS + M.FAILING_OPS + M.REFUSED_OPS:
        if M.fits(cls, f):
            ran += r.step(cls(f))
    for begin, fetch in ((M.CompressHostBegin, M.CompressHostFetch), (M.CompressDevicePackedBegin, M.CompressDevicePackedFetch),
                         (M.CompressHostInterleavedBegin, M.CompressHostFetch), (M.CompressHostBegin, M.CompressDevicePackedFetch)):
        if M.fits(begin, f):
            ran += r.step(begin(f)) and r.step(fetch(f.n))
    eng.close()
    assert ran >= 3, ran


STAGED_BEGINS = (M.CompressHostBegin, M.CompressHostInterleavedBegin, M.CompressDevicePackedBegin)


def test_pending_matrix_of_the_staging_area(fx, lib):
    """every staged _begin x every intervening op the mock serves x both _fetch kinds: the fetch's return code is the model's, a valid
    fetch delivers the begun batch, a void one leaves the output alone, and the next plain call works"""
    base, other = fx["f32_b1k_c3"], fx["u8_unsplit_b4k_c3"]
    inter = M.plain_ops(fx) + M.error_ops(fx) + M.pending_ops(fx, base.n)         # (the staged _begin kinds, on `other`, are among them)
    pairs = 0
    for begin_cls in STAGED_BEGINS:
        for k, x in enumerate(inter):
            for fetch_cls in (M.CompressHostFetch, M.CompressDevicePackedFetch):
                eng = M.Eng(lib, gpu=False)
                r = M.Runner(eng, "pair (%s, %s, %s)" % (begin_cls.__name__, x.name, fetch_cls.__name__))
                assert r.step(begin_cls(base))
                if not r.step(copy.copy(x)):
                    eng.close()
                    continue
                r.step(fetch_cls(base.n))
                r.step(M.CompressHost(other))
                r.step(M.DecompressHostSized(other))
                eng.close()
                pairs += 1
    assert pairs == 3 * 2 * 33, pairs                              # 33 of the 54 intervening ops have their entry points in the mock


def test_fetch_with_the_wrong_count_and_twice(fx, run):
    f = fx["f32_b1k_c3"]
    run.step(M.CompressHostBegin(f))
    run.step(M.CompressHostFetch(f.n + 1))
    run.step(M.CompressDevicePackedFetch(f.n - 1))
    run.step(M.CompressHostFetch(f.n))
    run.step(M.CompressHostFetch(f.n))
    run.step(M.CompressDevicePackedFetch(f.n))
    assert [o.name for o in run.log][-1].startswith("CompressDevicePackedFetch")


@pytest.mark.parametrize("k", range(6))
def test_seeded_sequence_on_the_mock(fx, lib, k):
    """the seeded runner of the GPU file, over the ops and fixtures the mock serves"""
    seed = int(os.environ.get("CIMG_TEST_SEED", "0")) + k
    eng = M.Eng(lib, gpu=False)
    try:
        M.seeded_sequence(M.Runner(eng, "seed %d" % seed), fx, np.random.default_rng(20261021 + seed), 150,
                          names=[n for n, f in fx.items() if not f.gpu_only])
    finally:
        eng.close()
