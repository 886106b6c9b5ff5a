"""Cheaper instruction forms in the per-mask kernel: each replaced expression
restated in numpy next to its former form, and the compiled C2 kernel checked for what the change
claims.

  * the SPC flip of the generated ops (polar_sc_jit.cpp): the select of a bit or 0 -> the condition
    shifted into place, for every lane position, both parities, every key nibble and word index;
    the per-plane form too
  * the SPC row decoder of the leaves (polar_sc_device.h leaf_spc): equality of 19-bit keys
  * the +1 / -1 multiplier of the multiply-add G and REP words (plane_pm1): every bit position, both
    halves, the whole 16-bit range of a half
  * the channel byte's sign (sm8_of_byte), every byte at every LLR width
  * 32-bit frame indices, store predicates and element offsets against the 64-bit computation, up
    to the largest batch the host accepts
"""
import os
import re
import sys

import numpy as np
import pytest

import util

U32 = np.uint32
FORMER = ("POLAR_PM1_MASK", "POLAR_SPC_FLIP_SELECT", "POLAR_LEAF_SPC_SELECT", "POLAR_MASK_ADDR64", "POLAR_SM8_SELECT",
          "POLAR_LANE_SELECT")


def u32(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64).astype(U32)


# ---- the SPC flip -----------------------------------------------------------------------------
def _flip_cases():
    """every (lane position code br, key nibble of lo / hi, parity of lo / hi)"""
    br, nlo, nhi, plo, phi = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), (0, 1), (0, 1), indexing="ij")
    par = (plo.astype(np.int64) << 15) | (phi.astype(np.int64) << 31)
    return u32(br.ravel()), u32(nlo.ravel()), u32(nhi.ravel()), u32(par.ravel())


@pytest.mark.parametrize("pos", [0, 5, 12])
def test_spc_flip_one_plane(pos):
    """n <= 16 words (one plane at bit offset pos, pos + n <= 16): the condition as 0 / 1 shifted to
    bit pos + word index, against the select of "1 << s" or 0"""
    br, nlo, nhi, par = _flip_cases()
    for ilo in range(16 - pos):
        for ihi in (0, ilo, 15 - pos):
            klo, khi = nlo | U32(ilo << 4) | U32(0x2400), nhi | U32(ihi << 4) | U32(0x0C00)   # (|lambda| above)
            flo = ((par & U32(0x8000)) != 0) & ((klo & U32(15)) == br)
            fhi = ((par & U32(0x80000000)) != 0) & ((khi & U32(15)) == br)
            ref = np.where(flo, U32(1) << U32(pos + ilo), U32(0)) | np.where(fhi, U32(0x10000) << U32(pos + ihi), U32(0))
            got = (flo.astype(U32) << U32(pos + ilo)) | (fhi.astype(U32) << U32(16 + pos + ihi))
            np.testing.assert_array_equal(got, ref)


def test_spc_flip_planes():
    """n > 16 words: per plane k the condition "flip, and the word index names plane k" shifted to
    the word's bit inside the plane"""
    br, nlo, nhi, par = _flip_cases()
    for planes in (2, 4, 8):
        for ilo, ihi in [(i, (7 * i + 3) % (16 * planes)) for i in range(16 * planes)]:
            klo, khi = nlo | U32(ilo << 4), nhi | U32(ihi << 4)
            flo = ((par & U32(0x8000)) != 0) & ((klo & U32(15)) == br)
            fhi = ((par & U32(0x80000000)) != 0) & ((khi & U32(15)) == br)
            for k in range(planes):
                ref = np.where(flo & ((ilo >> 4) == k), U32(1) << U32(ilo & 15), U32(0)) | \
                    np.where(fhi & ((ihi >> 4) == k), U32(0x10000) << U32(ihi & 15), U32(0))
                got = ((flo & ((ilo >> 4) == k)).astype(U32) << U32(ilo & 15)) | \
                    ((fhi & ((ihi >> 4) == k)).astype(U32) << U32(16 + (ihi & 15)))
                np.testing.assert_array_equal(got, ref)


def test_leaf_spc_flip():
    """leaf_spc: the lane whose key is the row minimum; keys are (15-bit magnitude << 4) | position"""
    rng = np.random.default_rng(11)
    own = u32(rng.integers(0, 1 << 19, 1 << 16))
    mn = own.copy()
    d = rng.integers(0, 3, own.size)
    mn[d == 1] = u32(rng.integers(0, 1 << 19, int((d == 1).sum())))
    mn[d == 2] ^= U32(1) << u32(rng.integers(0, 19, int((d == 2).sum())))   # (one bit apart)
    own[:4], mn[:4] = u32([0, 0, 0x7FFFF, 0x7FFFF]), u32([0, 1, 0x7FFFF, 0x7FFFE])
    for par in (0, 0x8000, 0x80000000, 0x80008000):
        par = U32(par)
        ref_lo, ref_hi = np.where(mn == own, par & U32(0x8000), U32(0)), np.where(mn == own, par & U32(0x80000000), U32(0))
        z = (mn ^ own) - U32(1)
        np.testing.assert_array_equal((z >> U32(16)) & par & U32(0x8000), ref_lo)
        np.testing.assert_array_equal(z & par & U32(0x80000000), ref_hi)


# ---- the +1 / -1 multiplier -------------------------------------------------------------------
@pytest.mark.parametrize("I", range(16))
def test_plane_pm1(I):
    lo = np.arange(1 << 16, dtype=np.int64)
    for hi in (lo, lo[::-1], (lo * 40503 + 7) & 0xFFFF):
        p = u32(lo | (hi << 16))
        # plane_mask<I>(p) | 0x00010001: per half (x << (15 - I)) as i16 >> 15, then OR 1
        ml = np.where((lo >> I) & 1, 0xFFFF, 0x0001)
        mh = np.where((hi >> I) & 1, 0xFFFF, 0x0001)
        ref = u32(ml | (mh << 16))
        b = (p >> U32(I)) & U32(0x00010001)
        prod = b.astype(np.uint64) * np.uint64(0xFFFE)
        assert int(b.max()) < 1 << 24 and int(prod.max()) < 1 << 32   # (a 24-bit multiply, no wrap)
        np.testing.assert_array_equal(u32(prod + np.uint64(0x00010001)), ref)


@pytest.mark.parametrize("q", [5, 6, 7, 8, 9])
def test_sm8_sign(q):
    qp = 1 << q
    t = np.arange(256, dtype=np.int64) & (qp - 1)
    ref = np.where(t >= qp // 2 + 1, 0x80, 0)
    np.testing.assert_array_equal((u32(qp // 2 - t) >> U32(24)) & U32(0x80), ref)


# ---- 32-bit frame indices, predicates and offsets ---------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 8, 9, 33, 67, 65536, 0x7FFFFFF1, 0x7FFFFFF8])
@pytest.mark.parametrize("stride", [8, 64, 67])
def test_frame_index_and_offsets_32bit(batch, stride):
    nw64 = (batch + 7) // 8
    nw = int(u32(batch) + U32(7)) >> 3
    assert nw == nw64
    waves = sorted(w for w in {0, 1, nw64 // 2, nw64 - 2, nw64 - 1} if 0 <= w < nw64)   # (others return at once)
    for w in waves:
        f0 = u32(w) * U32(8)
        for f in range(8):   # the fetch clamp
            fr = int(np.minimum(f0 + U32(f), u32(batch) - U32(1)))
            assert fr == min(w * 8 + f, batch - 1)
        nf = u32(batch) - f0
        for row in range(4):
            assert bool(U32(row) < nf) == (w * 8 + row < batch)
            assert bool(U32(row) + U32(4) < nf) == (w * 8 + row + 4 < batch)
            for word in (0, 15, 16, stride - 1):
                lw = int(U32(row) * U32(stride) + U32(word & 15))   # the lane's 32-bit element offset
                base = int(f0) * stride + (word & ~15)                # the uniform 64-bit part
                assert base + lw == (w * 8 + row) * stride + word
                assert base + 4 * stride + lw == (w * 8 + row + 4) * stride + word
    # the largest lane offset in bytes stays far below 2^32 for every plan of the per-mask kernel
    assert 2 * (3 * 4 * ((64 + 3) // 4) + 15) < 1 << 16


# ---- the compiled C2 kernel -------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(pkg):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import pair_census as pc
    import rtc_isa_check as ric
    src = pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()
    return pc, ric, src


def test_c2_budget(c2):
    _, ric, src = c2
    co = ric.clang_compile(src)
    kd = ric.kernel_descriptors(co)["polar_sc_mask_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_kernel"]
    assert kd["regs_unified"] <= 128 and meta["vgpr_count"] <= 128 and not meta["agpr_count"], (kd, meta)
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0 and meta["private_segment_fixed_size"] == 0


def test_c2_forms_and_census(c2):
    """Outside the exact REP fallback bodies and the byte copy of an unaligned input the kernel has
    no select on VCC and no 64-bit compare or add on the vector ALU, and its cost-weighted census
    is below that of the same tree built with every former-form switch."""
    pc, _, src = c2
    assert src.count("if (!al_) {") == 1 and src.count("if (rep_any_zero(acc_)) {") >= 4
    new = pc.cycles_census(pc.drop_unaligned_copy(src), no_rep_fallback=True)
    forms = {}
    for cls in new[3].values():
        for f, (n, _) in cls.items():
            forms[f] = forms.get(f, 0) + n
    bad = {f: n for f, n in forms.items() if f == "v_cndmask_b32_e32" or f.startswith("v_lshl_add_u64")
           or re.match(r"v_cmpx?_\w+_[iu]64", f)}
    assert not bad, bad
    assert forms.get("v_mad_u32_u24", 0) >= 100 and forms.get("v_pk_mad_u16", 0) >= 100, forms
    old = pc.cycles_census(pc.drop_unaligned_copy(src), defines=FORMER, no_rep_fallback=True)
    print("census: new %.0f cycles (%d priced VALU, unpriced %s); former forms %.0f cycles (%d priced VALU, unpriced %s)"
          % (new[0], new[1], new[2], old[0], old[1], old[2]))
    for total, priced, unpriced, _ in (new, old):
        assert sum(unpriced.values()) <= 0.03 * priced, unpriced   # (the comparison is of priced forms)
    assert new[0] < old[0], (new[0], old[0])
