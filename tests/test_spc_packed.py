"""The packed SPC epilogue of the per-mask kernel (polar_sc_jit.cpp kMaskFormsSrc, Gen::op; DESIGN.md
3.1) restated in numpy next to the form it replaces, and the compiled C2 kernel checked for what
the change claims (tests/test_out_transpose.py has the output transpose).

  * the SPC node epilogue with both frames packed (POLAR_SPC_PACKED) against the 32-bit one: a row
    of 16 lanes, nodes of 1, 2, 4, 8 and 16 words (a per-mask kernel has no wider SPC node: at most
    64 words, and a child of the root is never one), LLR_BITS 5..7 where the bound holds; even and
    odd parity, all-equal magnitudes, magnitudes at the G clamp, ties in the word and in the
    position; the mask "own key is the minimum" for every key below 0x8000
  * the bound itself as the generated source states it: LLR_BITS 8 and 9 keep the 32-bit epilogue
  * the compiled C2 kernel: no compare and no select in an SPC node of one word, registers and
    scratch, the census below that of the former forms
"""
import os
import re
import sys
import tempfile

import numpy as np
import pytest

import util

U32 = np.uint32
SWITCHES = ("POLAR_SPC_EPILOGUE32", "POLAR_OUT_TRANSPOSE6")


def u32(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64).astype(U32)


def pk(f, a, b):
    """f on the 16-bit halves of a and b, modulo 2^16"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    return u32((f(a & 0xFFFF, b & 0xFFFF) & 0xFFFF) | ((f(a >> 16, b >> 16) & 0xFFFF) << 16))


def pk_sra15(a):
    a = a.astype(np.int64)
    return u32(np.where(a & 0x8000, 0xFFFF, 0) | (np.where(a & 0x80000000, 0xFFFF, 0) << 16))


def row(f, v):
    """butterfly over the 16 lanes (axis 1) at distance 8, 4, 2, 1: every lane ends with the row's f"""
    for h in (8, 4, 2, 1):
        v = f(v, v[:, np.arange(16) ^ h])
    return v


def popc16(x):
    x = x.astype(np.int64)
    return sum((x >> i) & 1 for i in range(16))


BR = u32([int("{:04b}".format(p)[::-1], 2) for p in range(16)])   # bitrev4 of the lane's position


def gsat(q):
    return (1 << (q - 2)) - 1


def packed_ok(q, n):
    """POLAR_SPC_PACKED(n) of the generated source, and its static_assert"""
    return n <= 16 and ((gsat(q) << 10) | ((n - 1) << 4) | 15) < 0x8000


def node_inputs(rng, cases, n, q):
    """[cases, 16 lanes, n words] clamped G magnitudes and hard decisions of both frames, tie-heavy"""
    g = gsat(q)
    vals = np.array([0, 1, g - 1, g, g, g // 2], np.int64)
    l = rng.choice(vals, size=(2, cases, 16, n))
    l[:, : cases // 8] = rng.choice(vals, size=(2, cases // 8, 1, 1))            # all equal: ties in word and position
    l[:, cases // 8: cases // 4, :, :] = rng.choice(vals, size=(2, cases // 8, 16, 1))   # equal inside a lane
    h = rng.integers(0, 2, size=(2, cases, 16, n))
    return l, h


def epilogue_inputs(l, h, n):
    i = np.arange(n, dtype=np.int64)
    key = ((l << 10) | (i << 4)).min(axis=3)                     # kk_ per half
    kk = u32(key[0] | (key[1] << 16))
    hb = (h << i).sum(axis=3)                                     # the hard decisions, word i at bit i
    par = u32(hb[0] | (hb[1] << 16))
    return kk, par


def epilogue32(kk, par, n, sh):
    """the 32-bit epilogue (-DPOLAR_SPC_EPILOGUE32): the flip word of every lane"""
    klo, khi = kk & U32(0xFFFF), kk >> U32(16)
    p = u32(((popc16(par & U32(0xFFFF)) & 1) << 15) | ((popc16(par >> U32(16)) & 1) << 31))
    p = row(np.bitwise_xor, p)
    klo, khi = row(np.minimum, klo | BR), row(np.minimum, khi | BR)
    ilo, ihi = (klo >> U32(4)) & U32(63), (khi >> U32(4)) & U32(63)
    flo = ((p & U32(0x8000)) != 0) & ((klo & U32(15)) == BR)
    fhi = ((p & U32(0x80000000)) != 0) & ((khi & U32(15)) == BR)
    return (flo.astype(U32) << (U32(sh) + ilo)) | (fhi.astype(U32) << (U32(16 + sh) + ihi))


def epilogue_packed(kk, par, n, sh):
    """the packed epilogue as Gen::op emits it"""
    if n == 1:
        p = row(np.bitwise_xor, par << U32(sh))                  # the hard decision at the word's bit
    else:
        p = row(np.bitwise_xor, u32(popc16(par & U32(0xFFFF)) | (popc16(par >> U32(16)) << 16)))
    k0 = kk | BR | (BR << U32(16))
    km = row(lambda a, b: pk(np.minimum, a, b), k0)
    ne = pk_sra15(pk(np.subtract, km, k0))
    if n == 1:
        return p & ~ne & U32(0x00010001 << sh)
    s = (km >> U32(4)) & U32(0x000F000F)
    return pk(lambda a, b: a << b, p & ~ne & U32(0x00010001), s) << U32(sh)


@pytest.mark.parametrize("q", [5, 6, 7])
@pytest.mark.parametrize("n", [1, 2, 4, 8, 16])
def test_packed_epilogue_matches(n, q):
    assert packed_ok(q, n)
    rng = np.random.default_rng(1100 + 16 * q + n)
    l, h = node_inputs(rng, 20000, n, q)
    kk, par = epilogue_inputs(l, h, n)
    assert int((kk & U32(0xFFFF)).max()) <= (gsat(q) << 10) | ((n - 1) << 4)
    for sh in sorted({0, 16 - n, (16 - n) // n // 2 * n}):        # the node's place in its partial-sum word
        if n < 16:
            par_m = par & U32(((1 << n) - 1) * 0x00010001)
        else:
            par_m = par
        ref = epilogue32(kk, par_m, n, sh)
        got = epilogue_packed(kk, par if n == 1 else par_m, n, sh)
        np.testing.assert_array_equal(got, ref)
    # both parities, per frame, and exactly one lane flips where the parity is odd
    odd = (popc16(ref & U32(0xFFFF)).sum(axis=1) == 1)
    assert odd.any() and (~odd).any()
    assert set(np.unique(popc16(ref & U32(0xFFFF)).sum(axis=1))) == {0, 1}
    assert set(np.unique(popc16(ref >> U32(16)).sum(axis=1))) == {0, 1}


def test_one_word_exhaustive_small():
    """n = 1, magnitudes from {0, GSAT} in every lane pattern of one frame against three of the other"""
    lanes = ((np.arange(1 << 16)[:, None] >> np.arange(16)) & 1).astype(np.int64)
    for q in (5, 7):
        for other in (0, gsat(q), 1):
            l = np.stack([lanes * gsat(q), np.full_like(lanes, other)])[:, :, :, None]
            for hbit in (lanes, 1 - lanes, np.ones_like(lanes)):
                h = np.stack([hbit, lanes])[:, :, :, None]
                kk, par = epilogue_inputs(l, h, 1)
                np.testing.assert_array_equal(epilogue_packed(kk, par, 1, 11), epilogue32(kk, par & U32(0x00010001), 1, 11))


def test_minimum_mask_every_key():
    """ne_ = sign of (minimum - own key) per half: clear exactly where they are equal, for every own
    key below 0x8000 against minima at and below it"""
    k0 = np.arange(0x8000, dtype=np.int64)
    for km in (k0, k0 - 1, k0 >> 1, k0 & ~15, np.zeros_like(k0), k0 - (k0 & 15)):
        km = np.clip(km, 0, None)
        a, b = u32(km | (k0 << 16)), u32(k0 | (km << 16))         # (own key, minimum) in either half
        ne = pk_sra15(pk(np.subtract, a, b))
        np.testing.assert_array_equal(ne & U32(0xFFFF), u32(np.where(km != k0, 0xFFFF, 0)))
        ne = pk_sra15(pk(np.subtract, u32(km | (km << 16)), u32(k0 | (k0 << 16))))
        np.testing.assert_array_equal(ne, u32(np.where(km != k0, 0xFFFFFFFF, 0)))
    # past the bound the sign no longer tells (0 - 0x8001 = 0x7FFF): the reason for the static_assert
    assert int(pk_sra15(pk(np.subtract, u32([0]), u32([0x8001])))[0]) & 0xFFFF == 0


def test_bound_restated():
    for q in (5, 6, 7):
        for n in (1, 2, 4, 8, 16):
            assert packed_ok(q, n)
        assert not packed_ok(q, 32) and not packed_ok(q, 64)       # (hybrid subtrees: not built with these forms)
    for q in (8, 9):
        assert not any(packed_ok(q, n) for n in (1, 2, 4, 8, 16))   # keys reach 0xFFFF at GSAT = 63


def test_bound_in_the_source(pkg):
    src = pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()
    assert "#define POLAR_SPC_GSAT_ ((1 << (POLAR_Q - 2)) - 1)" in src
    assert "#define POLAR_SPC_PACKED(n) ((n) <= 16 && ((POLAR_SPC_GSAT_ << 10) | (((n) - 1) << 4) | 15) < 0x8000)" in src
    for n in (1, 4, 8):
        assert "#if POLAR_SPC_PACKED(%d)\n    static_assert(((GSAT << 10) | %du) < 0x8000u" % (n, ((n - 1) << 4) | 15) in src
    cfg = pkg.default_config()
    cfg.llr_bits = 8
    src8 = pkg.Decoder(util.mask("FB_N1024_K512"), config=cfg).kernel_source()
    assert "#define POLAR_Q 8\n" in src8 and "#if POLAR_SPC_PACKED(1)" in src8   # (false there: the #else branch)


# ---- the compiled C2 kernel -------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2(pkg):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import pair_census as pc
    import rtc_isa_check as ric
    return pc, ric, pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()


def test_c2_budget(c2):
    _, ric, src = c2
    co = ric.clang_compile(src)
    kd = ric.kernel_descriptors(co)["polar_sc_mask_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_kernel"]
    print("C2: %d VGPRs, %d AGPRs, private %d B" % (meta["vgpr_count"], meta["agpr_count"], meta["private_segment_fixed_size"]))
    assert meta["vgpr_count"] <= 98 and not meta["agpr_count"], (kd, meta)
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0 and meta["private_segment_fixed_size"] == 0


def test_c2_spc_n1_has_no_compare_and_the_census_falls(c2):
    pc, _, src = c2
    assert src.count("// SPC n 1 ") == 4 and src.count("#if POLAR_SPC_PACKED(1)") == 4
    plain = pc.drop_unaligned_copy(src)
    marked, _ = pc.mark_mask_kernel(pc.drop_rep_fallback(plain))
    with tempfile.TemporaryDirectory() as tmp:
        asm = pc.compile_asm(marked, tmp)
    blocks = re.findall(r";@@ SPC n1\n(.*?)(?=;@@ )", asm, flags=re.S)
    assert len(blocks) == 4
    for b in blocks:
        ins = re.findall(r"^\s+(v_\w+)", b, flags=re.M)
        assert 30 <= len(ins) <= 45, len(ins)
        assert not [i for i in ins if i.startswith("v_cmp") or i.startswith("v_cndmask")], ins
    out = re.findall(r";@@ output\n(.*?)(?=\.Lfunc_end)", asm, flags=re.S)
    # four chunks x four stages, one rotate each (the select is v_bfi_b32 or v_bitop3_b32)
    assert len(out) == 1 and out[0].count("v_alignbit_b32") == 16
    assert len(re.findall(r"^\s+v_\w+", out[0], flags=re.M)) <= 150
    new = pc.cycles_census(plain, no_rep_fallback=True)
    old = pc.cycles_census(plain, defines=SWITCHES, no_rep_fallback=True)
    print("census: new %.0f cycles (%d priced VALU, unpriced %s); former forms %.0f cycles (%d priced VALU, unpriced %s)"
          % (new[0], new[1], new[2], old[0], old[1], old[2]))
    # v_alignbit_b32 is not priced: counted at the single-issue price of a 3-source VOP3
    extra = new[2].get("v_alignbit_b32", 0) * pc.SINGLE[pc.WAVES.index(4)]
    assert new[0] + extra < old[0] - 200, (new[0], extra, old[0])
