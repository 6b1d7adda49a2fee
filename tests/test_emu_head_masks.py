"""The head paths of the wave LZ4 encoder on the lane emulator, against the liblz4-pinned oracle, in all three write orders.

The planes (tests/_head_planes.py) are the smallest that reach each place where csrc/encode_kernel.h forms a lane mask: the run
path's hit test and both of its length scans, the extension's backward and forward masks, the three-probe hit mask with every
value of `clean`, the narrow path near the end of a plane, and the parked-lane flush.  Bytes, return value and `need` must be
the oracle's; one byte less than `need` must fail in both."""
import numpy as np
import pytest

import _emu as E
import _head_planes as H
import _oracle as O


@pytest.fixture(scope="module")
def planes():
    return H.planes()


@pytest.fixture(scope="module")
def wanted(planes):
    """the oracle's answer per plane, computed once: (return value, bytes, need) at c-blosc2's capacity (the plane's length)"""
    return {name: O.lz4_compress(p, cap=p.size, want_need=True) for name, p, _ in planes}


def test_every_case_of_the_list_is_there(planes):
    names = {name for name, _, _ in planes}
    for n in (13, 14, 16, 17, 76, 77, 80, 255, 256, 257, 258, 259, 260, 261, 16384):
        assert "tiles_%d" % n in names
    for want in ("candidate_zero", "back_0", "back_1", "back_over_64", "sequences_64", "sequences_65", "long_run_0", "long_run_1",
                 "slots_10_hitNone", "slots_21_hitNone", "slots_20_hitNone", "slots_equal_21", "slots_equal_20",
                 "run_to_matchlimit-1_n120_off1", "run_to_matchlimit+0_n120_hit", "run_to_matchlimit+1_n700_hit"):
        assert want in names, want


def test_planes_have_the_property_they_were_built_for(planes):
    """the sequential model is first pinned to the oracle's bytes (unlimited capacity), then asked what each plane went through"""
    for name, p, prop in planes:
        if p.size > 1000 and prop is None:
            continue                                      # (the model is plain Python: the large planes carry no property)
        stream, events = H.model(p)
        r, want = O.lz4_compress(p, cap=p.size + p.size // 255 + 32)[:2]
        assert stream == want[:r], name
        if prop is not None:
            assert prop(events), name


@pytest.mark.parametrize("order", [0, 1, 2])
def test_head_planes_match_the_oracle(planes, wanted, order):
    E.set_write_order(order)
    try:
        for name, p, _ in planes:
            want_r, want, want_need = wanted[name]
            r, out, need = E.lz4_encode(p, p.size)
            assert r == want_r, (name, r, want_r)
            assert out == want[:max(want_r, 0)], name
            if want_r > 0:
                assert need == want_need, name
    finally:
        E.set_write_order(0)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_budget_missed_by_one_byte(planes, wanted, order):
    """a capacity of need - 1 fails, a capacity of need succeeds with the same bytes -- in the emulator as in the oracle"""
    E.set_write_order(order)
    try:
        checked = 0
        for name, p, _ in planes:
            want_r, want, want_need = wanted[name]
            if want_r <= 0:
                continue
            assert O.lz4_compress(p, cap=want_need - 1)[0] == 0, name
            assert E.lz4_encode(p, want_need - 1)[0] == 0, name
            r, out, _ = E.lz4_encode(p, want_need)
            assert r == want_r and out == want[:want_r], name
            checked += 1
        assert checked > 40
    finally:
        E.set_write_order(0)
