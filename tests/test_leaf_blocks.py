"""SPC and REP sub-blocks of the 16-LLR leaf decided directly (polar_sc_device.h leaf_ms,
DESIGN.md 3.1), on the CPU:

  * the two rules against a numpy restatement of the recursion (F = min / XOR; G the exact
    sign-magnitude add, ties -> sign(a'), -0 kept): exhaustively at W = 4, seeded random at W = 8
    and W = 4 up to the largest magnitude a block can see, a good third of it among ties
  * the packed 16-bit expressions as shipped (SPC key, minimum and flip mask; REP bias, 32-bit adds
    of two halves, carried sign) against the rules over the whole static bound, LLR_BITS 5..9
  * the compiled C2 kernel: the leaf class is cheaper than with -DPOLAR_LEAF_RECURSE and the kernel
    keeps its register and scratch budget
"""
import os
import sys

import numpy as np
import pytest

import util

U32 = np.uint32


# ---- the recursion (leaf_ms semantics) --------------------------------------------------------
def F(a, b):
    return a[0] ^ b[0], np.minimum(a[1], b[1])


def G(a, b, u):
    """exact: a' = a with sign ^ u; same signs add, else |difference|; sign(b) if |a| < |b| else sign(a')"""
    sa = a[0] ^ u
    x = sa ^ b[0]
    lt = a[1] < b[1]
    return b[0] ^ (x & ~lt), np.where(x, np.abs(a[1] - b[1]), a[1] + b[1])


def leaf(lam, fb):
    """lam = (s bool [n, W], m int [n, W]); fb = list of W frozen flags (1 = information)"""
    s, m = lam
    W = len(fb)
    if not any(fb):
        return np.zeros_like(s)
    if all(fb):
        return s.copy()
    if W == 2:
        if fb == [1, 0]:
            return np.stack([s[:, 0] ^ s[:, 1], np.zeros_like(s[:, 0])], axis=1)
        u1 = np.where(m[:, 0] < m[:, 1], s[:, 1], s[:, 0])
        return np.stack([u1, u1], axis=1)
    H = W // 2
    a, b = (s[:, :H], m[:, :H]), (s[:, H:], m[:, H:])
    xa = leaf(F(a, b), fb[:H])
    xb = leaf(G(a, b, xa), fb[H:])
    return np.concatenate([xa ^ xb, xb], axis=1)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


# ---- the two rules ----------------------------------------------------------------------------
def spc_rule(lam):
    s, m = lam
    n, W = s.shape
    br = np.array([bitrev(j, W.bit_length() - 1) for j in range(W)])
    x = s.copy()
    odd = (s.sum(axis=1) & 1).astype(bool)
    j = ((m * W) + (W - 1 - br)[None, :]).argmin(axis=1)   # smallest |lambda|, ties: largest bitrev
    x[np.arange(n), j] ^= odd
    return x


def rep_rule(lam):
    s, m = lam
    n, W = s.shape
    t = np.where(s, -m, m)
    bit = s[:, 0].copy()            # every partial sum 0: the sign bit of position 0 (may be -0)
    step = W
    while step >= 1:                # the later sum (smaller step) overrides where it is not 0
        p = t[:, ::step].sum(axis=1)
        bit = np.where(p != 0, p < 0, bit)
        step //= 2
    return np.repeat(bit[:, None], W, axis=1)


def exhaustive(W, mmax):
    v = np.arange((2 * (mmax + 1)) ** W)
    cols = []
    for _ in range(W):
        cols.append(v % (2 * (mmax + 1)))
        v = v // (2 * (mmax + 1))
    c = np.stack(cols, axis=1)
    return (c & 1).astype(bool), (c >> 1).astype(np.int64)


def tie_heavy(rng, n, W, mmax):
    """a good third from magnitudes <= 2, a third exponential, the rest uniform up to mmax"""
    k = n // 3 + 1
    m = np.concatenate([rng.integers(0, 3, (k, W)), np.minimum(rng.exponential(3.0, (k, W)).astype(np.int64), mmax),
                        rng.integers(0, mmax + 1, (n - 2 * k, W))])
    return rng.integers(0, 2, (n, W)).astype(bool), m.astype(np.int64)


SPC = {4: [0, 1, 1, 1], 8: [0] + [1] * 7}
REP = {4: [0, 0, 0, 1], 8: [0] * 7 + [1]}
CASES = [("exhaustive", 4, 7), ("random", 8, 62), ("random", 4, 124), ("random", 8, 3)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-W%d-m%d" % c)
def blocks(request):
    kind, W, mmax = request.param
    if kind == "exhaustive":
        return W, exhaustive(W, mmax)
    return W, tie_heavy(np.random.default_rng(1000 * W + mmax), 300000, W, mmax)


def test_spc_rule_is_the_recursion(blocks):
    W, lam = blocks
    np.testing.assert_array_equal(spc_rule(lam), leaf(lam, SPC[W]))
    s, m = lam
    odd = (s.sum(axis=1) & 1).astype(bool)
    tied = (np.sort(m, axis=1)[:, 0] == np.sort(m, axis=1)[:, 1]) & odd
    assert tied.mean() > 0.1, tied.mean()   # (the tie order is exercised)


def test_rep_rule_is_the_recursion(blocks):
    W, lam = blocks
    np.testing.assert_array_equal(rep_rule(lam), leaf(lam, REP[W]))
    zero = np.where(lam[0], -lam[1], lam[1]).sum(axis=1) == 0
    assert zero.mean() > 0.01, zero.mean()  # (zero totals are exercised)


# ---- the packed halves as shipped -------------------------------------------------------------
def pk(f):
    def g(a, b):
        lo = f(a & U32(0xFFFF), b & U32(0xFFFF)) & U32(0xFFFF)
        hi = f(a >> U32(16), b >> U32(16)) & U32(0xFFFF)
        return lo | (hi << U32(16))
    return g


pk_add = pk(lambda a, b: a + b)
pk_sub = pk(lambda a, b: a - b)
pk_min = pk(np.minimum)
pk_sra15 = pk(lambda a, _: np.where(a & U32(0x8000), U32(0xFFFF), U32(0)))


def pk_mad(a, b, c):
    return pk_add(pk(lambda x, y: x * y)(a, b), c)


def pack(lo, hi):
    return lo.astype(U32) | (hi.astype(U32) << U32(16))


def two_frames(lam):
    """split operands of a block: frame i in the low halves, a permuted frame in the high halves"""
    s, m = lam
    perm = np.random.default_rng(5).permutation(len(s))
    return pack(m, m[perm]), pack(s * 0xFFFF, s[perm] * 0xFFFF), perm


def partner(v, H):
    return v[:, np.arange(v.shape[1]) ^ H]


def spc_packed(M, S, W, B):
    nbr = np.array([15 - bitrev(B + j, 4) for j in range(W)], dtype=U32) * U32(0x00010001)   # Lanes::nbr
    assert W in (4, 8)
    par, H = S.copy(), W // 2
    while H:
        par = par ^ partner(par, H)
        H //= 2
    k0 = pk_mad(M, U32(0x00100010), nbr[None, :])
    k, H = k0.copy(), W // 2
    while H:
        k = pk_min(k, partner(k, H))
        H //= 2
    return S ^ (par & ~pk_sra15(pk_sub(k, k0), 0))


def rep_packed(M, S, W, bias):
    bias = U32(bias * 0x00010001)                             # LeafBlock<W>::BIAS in both halves
    v = pk_mad(M, S | U32(0x00010001), bias)
    m, H, K = S.copy(), W // 2, 1
    while H:
        v = v + partner(v, H)                                 # one 32-bit add of both halves
        m = pk_sra15(pk_sub(pk_add(v, m), U32(int(bias) << K)), 0)
        H //= 2
        K += 1
    return np.repeat(m[:, :1], W, axis=1)                     # row_bcast of the block's first lane


def bound_cases(W, mmax):
    """the whole bound: every sign pattern at the largest magnitude and at 0, the exhaustive small
    cases scaled to the bound, random magnitudes up to it and tie-heavy ones"""
    rng = np.random.default_rng(77 * W + mmax)
    sg = ((np.arange(1 << W)[:, None] >> np.arange(W)[None, :]) & 1).astype(bool)
    parts = [(sg, np.full(sg.shape, mmax, np.int64)), (sg, np.zeros(sg.shape, np.int64))]
    if W == 4:
        es, em = exhaustive(4, 3)
        parts.append((es, np.minimum(em * ((mmax + 2) // 3), mmax)))
    parts.append(tie_heavy(rng, 60000, W, mmax))
    edge = rng.integers(0, 2, (20000, W)).astype(bool), mmax - rng.integers(0, 2, (20000, W))
    parts.append(edge)
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def leaf_block(q, p16, W):
    """LeafBlock<W> of polar_sc_device.h: (MMAX, BIAS, SPC_OK, REP_OK). A leaf's inputs are <= QMAG at
    PAR <= 16 and <= QMAG * PAR / 16 in the last word of a PAR 32 / 64 word (exact G above the words)"""
    qmag = (1 << (q - 1)) - 1
    mmax = qmag * p16 * 16 // W
    bias = (1 << (q + 2)) * p16
    spc_ok = ((mmax << 4) | 15) < 0x8000
    rep_ok = bias > mmax + 1 and W * (bias + mmax) < 0x10000 and W * mmax + 1 < 0x8000
    return mmax, bias, spc_ok, rep_ok


def test_leaf_block_bounds():
    """where the halves do not hold the bound the device takes the recursion: exactly these"""
    bad = {(q, p16, W, kind) for q in (5, 6, 7, 8, 9) for p16 in (1, 2, 4) for W in (4, 8)
           for kind, ok in zip(("spc", "rep"), leaf_block(q, p16, W)[2:]) if not ok}
    assert bad == {(9, 4, 4, "spc"), (9, 4, 8, "rep")}, bad


@pytest.mark.parametrize("p16", [1, 2, 4])
@pytest.mark.parametrize("q", [5, 6, 7, 8, 9])
@pytest.mark.parametrize("W", [4, 8])
def test_packed_halves(q, W, p16):
    mmax, bias, spc_ok, rep_ok = leaf_block(q, p16, W)
    lam = bound_cases(W, mmax)
    M, S, perm = two_frames(lam)
    for ok, ref, got in ((spc_ok, spc_rule, lambda: [spc_packed(M, S, W, B) for B in range(0, 16, W)]),
                         (rep_ok, rep_rule, lambda: [rep_packed(M, S, W, bias)])):
        if not ok:      # (test_leaf_block_bounds, test_par64_blocks_take_the_recursion)
            continue
        r = ref(lam)
        want = pack(r * 0xFFFF, r[perm] * 0xFFFF)
        for g in got():
            np.testing.assert_array_equal(g, want)


def test_bound_is_needed():
    """the halves do fail beyond the bound: the block sizes LeafBlock turns away are not spurious"""
    mmax, bias, spc_ok, rep_ok = leaf_block(9, 4, 4)
    lam = bound_cases(4, mmax)
    M, S, perm = two_frames(lam)
    r = spc_rule(lam)
    assert not spc_ok and (spc_packed(M, S, 4, 12) != pack(r * 0xFFFF, r[perm] * 0xFFFF)).any()


PROBE = """#define POLAR_LANE_REMAP 0
#define POLAR_Q %d
#define POLAR_LPAR %d
#include "polar_sc_device.h"
using namespace polar;
extern "C" __global__ void k(const u32 *in, u32 *out) {
  Lanes ln; ln.init(threadIdx.x & 15u);
  out[threadIdx.x] = leaf_ms<0x%xu, %d, %d>(in[threadIdx.x], in[threadIdx.x + 64], ln); }
"""


@pytest.mark.parametrize("q,lpar,fb,B,W,direct", [(9, 6, 0xE000, 12, 4, False),
                                                  (9, 6, 0x8000, 12, 4, True), (9, 6, 0xFE00, 8, 8, True),
                                                  (9, 5, 0xE000, 12, 4, True), (6, 6, 0x8000, 8, 8, True)])
def test_par64_blocks_take_the_recursion(pkg, tmp_path, q, lpar, fb, B, W, direct):
    """inside a PAR 64 word at LLR_BITS 9 the SPC of width 4 compiles to the recursion (the same code
    as with -DPOLAR_LEAF_RECURSE; a REP of width 8 recurses once and decides its REP of width 4);
    the blocks that fit are decided directly"""
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import pair_census as pc
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    src = PROBE % (q, lpar, fb, B, W)

    def text(asm):
        return [line for line in asm.split("\n") if "__hip_cuid_" not in line]

    same = text(pc.compile_asm(src, str(a))) == text(pc.compile_asm(src, str(b), ["-DPOLAR_LEAF_RECURSE"]))
    assert same != direct


def test_extended_0_keeps_the_recursion(pkg, tmp_path):
    """EXTENDED = 0 (the G inside the leaf clamps): the same machine code with and without the switch"""
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import pair_census as pc
    cfg = pkg.default_config()
    cfg.extended = 0
    src = pkg.Decoder(util.mask("FB_N1024_K512"), config=cfg).kernel_source()
    assert "#define POLAR_EXT 0\n" in src
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()

    def text(asm):   # (the compile unit's id hashes the command line)
        return [line for line in asm.split("\n") if "__hip_cuid_" not in line]

    assert text(pc.compile_asm(src, str(a))) == text(pc.compile_asm(src, str(b), ["-DPOLAR_LEAF_RECURSE"]))
    cfg.extended = 1   # (and the switch is live where the blocks are decided directly)
    src = pkg.Decoder(util.mask("FB_N1024_K512"), config=cfg).kernel_source()
    assert text(pc.compile_asm(src, str(a))) != text(pc.compile_asm(src, str(b), ["-DPOLAR_LEAF_RECURSE"]))


# ---- the compiled C2 kernel -------------------------------------------------------------------
def test_c2_leaf_census_and_budget(pkg):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import pair_census as pc
    import rtc_isa_check as ric
    src = pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()
    new = pc.cycles_census(pc.drop_unaligned_copy(src), no_rep_fallback=True)
    old = pc.cycles_census(pc.drop_unaligned_copy(src), defines=("POLAR_LEAF_RECURSE",), no_rep_fallback=True)

    def leaf_class(res):
        forms = res[3]["leaf"]
        return sum(n for n, c in forms.values() if c is not None), sum(n * c for n, c in forms.values() if c is not None)

    (nv, nc), (ov, oc) = leaf_class(new), leaf_class(old)
    print("leaf class: %d priced VALU, %.0f cycles; with POLAR_LEAF_RECURSE %d, %.0f; kernel %.0f against %.0f cycles"
          % (nv, nc, ov, oc, new[0], old[0]))
    assert nv < ov and nc < oc, ((nv, nc), (ov, oc))
    assert new[0] < old[0], (new[0], old[0])
    for res in (new, old):
        assert sum(res[2].values()) <= 0.03 * res[1], res[2]
    co = ric.clang_compile(src)
    kd = ric.kernel_descriptors(co)["polar_sc_mask_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_kernel"]
    assert kd["regs_unified"] <= 128 and meta["vgpr_count"] <= 128 and not meta["agpr_count"], (kd, meta)
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0 and meta["private_segment_fixed_size"] == 0
