"""csrc/trunc_plan.h: which cparams name blosc2's trunc-prec filter, which are valid, and the mask they stand for -- against the rule
restated in tests/_trunc.py (zeroed = M - m for m >= 0, -m for m < 0; valid iff |m| <= M and zeroed < M)."""
import ctypes as C

import pytest

import _trunc as T


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return T.build_emu(tmp_path_factory.mktemp("trunc_plan"))


@pytest.mark.parametrize("ts", [2, 4, 8])
def test_validity_and_mask_for_every_meta(L, ts):
    M = T.MANTISSA[ts]
    valid = 0
    for m in range(-M - 1, M + 2):
        z, mask = C.c_int(-1), C.c_uint64(0)
        rc = L.tremu_check(ts, m & 0xFF, C.byref(z), C.byref(mask))
        want = T.zeroed_bits(ts, m)
        if want is None:
            assert rc == T.ERR_INVALID_PARAM, (ts, m)
            continue
        valid += 1
        assert rc == 0 and z.value == want, (ts, m, z.value)
        elem = ~((1 << want) - 1) & ((1 << (8 * ts)) - 1)
        rep = 0
        for k in range(8 // ts):
            rep |= elem << (8 * ts * k)
        assert mask.value == rep, (ts, m, hex(mask.value))
        # sign and exponent are never touched
        assert elem >> M == (1 << (8 * ts - M)) - 1
    # m = 0 and m = -M are invalid, m = M is the valid no-op: M values each side
    assert valid == 2 * M - 1
    z, mask = C.c_int(-1), C.c_uint64(0)
    assert L.tremu_check(ts, M, C.byref(z), C.byref(mask)) == 0 and z.value == 0 and mask.value == (1 << 64) - 1
    assert L.tremu_check(ts, 0, C.byref(z), C.byref(mask)) == T.ERR_INVALID_PARAM
    assert L.tremu_check(ts, -M & 0xFF, C.byref(z), C.byref(mask)) == T.ERR_INVALID_PARAM


@pytest.mark.parametrize("ts", [1, 3, 16])
def test_other_typesizes_are_refused(L, ts):
    z, mask = C.c_int(-1), C.c_uint64(0)
    for m in (1, 5, -1):
        assert L.tremu_check(ts, m & 0xFF, C.byref(z), C.byref(mask)) == T.ERR_INVALID_PARAM
        assert L.tremu_from_cparams(C.byref(T.emu_cparams(ts, m))) == T.ERR_INVALID_PARAM
        assert L.tremu_plan_rc(C.byref(T.emu_cparams(ts, m)), 4096, 1) == T.ERR_INVALID_PARAM


def test_planner_takes_the_filter_only_on_the_callers_word(L):
    p = T.emu_cparams(4, 12)
    assert L.tremu_from_cparams(C.byref(p)) == 1
    assert L.tremu_plan_rc(C.byref(p), 65536, 0) == T.ERR_CODEC_SUPPORT      # nobody said the pass has run: refused as ever
    assert L.tremu_plan_rc(C.byref(p), 65536, 1) == 0
    assert L.tremu_plan_rc(C.byref(T.emu_cparams(4, 0)), 65536, 1) == T.ERR_INVALID_PARAM
    assert L.tremu_plan_rc(C.byref(T.emu_cparams(4, 24)), 65536, 1) == T.ERR_INVALID_PARAM
    plain = T.emu_cparams(4)
    assert L.tremu_from_cparams(C.byref(plain)) == 0 and L.tremu_plan_rc(C.byref(plain), 65536, 0) == 0


@pytest.mark.parametrize("filters", [(0, 0, 0, 0, 0, 4), (0, 0, 0, 0, 1, 4), (4, 0, 0, 0, 0, 1), (0, 0, 0, 4, 0, 1), (1, 0, 0, 0, 4, 1),
                                     (0, 0, 0, 0, 4, 3), (0, 0, 0, 0, 3, 1), (4, 1, 0, 0, 0, 0)])
def test_a_misplaced_filter_stays_codec_support(L, filters):
    p = T.emu_cparams(4, filters=filters, meta=(12,) * 6)
    assert L.tremu_from_cparams(C.byref(p)) == 0                              # not ours: the planner's refusal stands
    for truncated in (0, 1):
        assert L.tremu_plan_rc(C.byref(p), 65536, truncated) == T.ERR_CODEC_SUPPORT, (filters, truncated)
