"""The output transpose of the per-mask kernel in three instructions per stage (polar_sc_jit.cpp
kMaskFormsSrc row_transpose16_x) against row_transpose16 (polar_sc_device.h), both
restated in numpy over the 16 lanes of a row.

A stage is (x & M) | ((y << s) & ~M) on the lower lane of a pair and ((y >> s) & M) | (x & ~M) on
the upper, y the partner's word. The new form is bfi(A, x, rotr(y, r)) with A = M / ~M and
r = 32 - s / s: the bits the rotate wraps round fall under the side of the mask that takes x.
"""
import numpy as np
import pytest

U32 = np.uint32
STAGES = ((8, 0x00FF00FF), (4, 0x0F0F0F0F), (2, 0x33333333), (1, 0x55555555))   # (lane distance = shift, M)
LANES = np.arange(16)


def rotr(y, r):
    r = int(r) & 31                        # (v_alignbit_b32 reads the count modulo 32)
    return y if r == 0 else (y >> U32(r)) | (y << U32(32 - r))


def stage_former(v, s, M):
    p = v[:, LANES ^ s]
    M, nM = U32(M), U32(~M & 0xFFFFFFFF)
    lo = (v & M) | ((p & M) << U32(s))
    hi = ((p >> U32(s)) & M) | (v & nM)
    return np.where((LANES & s) == 0, lo, hi)


def constants(pl, s, M):
    """OutT::init for one stage: (A, r) of lane pl"""
    clear = (((pl >> {8: 3, 4: 2, 2: 1, 1: 0}[s]) & 1) - 1) & 0xFFFFFFFF    # clear_mask<B>(pl)
    A = clear ^ (~M & 0xFFFFFFFF)
    r = ((pl & s) << 1) + (32 - s)
    return A, r


def stage_new(v, s, M):
    p = v[:, LANES ^ s]
    out = np.empty_like(v)
    for pl in range(16):
        A, r = constants(pl, s, M)
        rot = rotr(p[:, pl], r)
        out[:, pl] = (v[:, pl] & U32(A)) | (rot & U32(~A & 0xFFFFFFFF))    # v_bfi_b32 A, x, rot
    return out


def words():
    rng = np.random.default_rng(1300)
    v = rng.integers(0, 1 << 32, size=(4096, 16), dtype=np.uint64).astype(U32)
    v[:4] = np.array([0xFFFFFFFF, 0, 0x80000001, 0x00018000], U32)[:, None]
    return v


@pytest.mark.parametrize("s,M", STAGES)
def test_constants(s, M):
    for pl in range(16):
        A, r = constants(pl, s, M)
        upper = bool(pl & s)
        assert A == ((~M & 0xFFFFFFFF) if upper else M)
        assert r & 31 == (s if upper else 32 - s)


@pytest.mark.parametrize("s,M", STAGES)
def test_wrapped_bits_fall_under_x(s, M):
    """rotl(y, s) differs from y << s only in the low s bits, where ~M is clear; rotr(y, s) from
    y >> s only in the high s bits, where M is clear"""
    assert (~M & 0xFFFFFFFF) & ((1 << s) - 1) == 0
    assert M & (((1 << s) - 1) << (32 - s)) == 0
    assert (M << s) & 0xFFFFFFFF == ~M & 0xFFFFFFFF
    y = words()[:, 0]
    np.testing.assert_array_equal(rotr(y, 32 - s) & U32(~M & 0xFFFFFFFF), (y & U32(M)) << U32(s))
    np.testing.assert_array_equal(rotr(y, s) & U32(M), (y >> U32(s)) & U32(M))


@pytest.mark.parametrize("s,M", STAGES)
def test_stage(s, M):
    v = words()
    np.testing.assert_array_equal(stage_new(v, s, M), stage_former(v, s, M))


def test_whole_transpose():
    v = words()
    a, b = v.copy(), v.copy()
    for s, M in STAGES:
        a, b = stage_former(a, s, M), stage_new(b, s, M)
    np.testing.assert_array_equal(b, a)
    # and it is the 16 x 16 bit transpose of both halves: lane l bit j <- lane j bit l
    bits = (v[:, :, None] >> np.arange(32, dtype=U32)) & U32(1)            # [case, lane, bit]
    want = np.zeros_like(v)
    for half in (0, 16):
        t = bits[:, :, half:half + 16].transpose(0, 2, 1)                   # [case, lane l, bit j] = lane j bit l
        want |= (t.astype(np.uint64) << (np.arange(16, dtype=np.uint64) + np.uint64(half))).sum(axis=2).astype(U32)
    np.testing.assert_array_equal(b, want)
