"""Runs of frozen-left levels of the 16-LLR leaf as an exact-add chain (polar_sc_device.h leaf_ms,
DESIGN.md 3.1), on the CPU:

  * the rule against the numpy restatement of the recursion in tests/test_leaf_blocks.py (F = min /
    XOR; G the exact sign-magnitude add, ties -> sign(a'), -0 kept): exhaustively at W = 4
    up to |lambda| = 7, 300 k tie-heavy random cases at W = 8 and W = 16, and rows of all zeros, of
    equal magnitudes and of the largest magnitude under every sign pattern (-0 at position 0 too)
  * the packed 16-bit expressions as shipped (bias, 32-bit adds of two halves, carried sign, |total|)
    over the whole static bound at LLR_BITS 5..9 and PAR 16 / 32 / 64
  * the compiled C2 kernel: register and scratch budget, fewer priced issue cycles than with the
    switch, and with the switch the machine code this change started from
"""
import os
import sys

import numpy as np
import pytest

import util
import test_leaf_blocks as tlb
from test_leaf_blocks import U32, leaf, pack, partner, pk_add, pk_sub, pk_mad, pk_sra15

pk_abs_i16 = tlb.pk(lambda a, _: np.where(a & U32(0x8000), U32(0x10000) - a, a))


def bits(pattern):
    return [int(c) for c in pattern]


def add_levels(fb):
    """leaf_add_levels: the run of all-frozen left halves from the top of the block"""
    k = 0
    while len(fb) >= 2 and not any(fb[:len(fb) // 2]):
        fb = fb[len(fb) // 2:]
        k += 1
    return k


# ---- the rule ----------------------------------------------------------------------------------
def add_chain_rule(lam, fb):
    """K frozen-left levels above a child of width WC: the child's input at position j is the sum of
    the positions = j mod WC; a zero sum keeps the sign of the last partial sum that is not 0 in the
    order position j, + j + W/2, + the two at distance W/4, ..; the child's bits repeat W / WC times"""
    s, m = lam
    n, W = s.shape
    K = add_levels(fb)
    WC = W >> K
    t = np.where(s, -m, m)
    neg = s[:, :WC].copy()
    step = W
    while step > WC:
        step //= 2
        p = np.stack([t[:, j::step].sum(axis=1) for j in range(WC)], axis=1)   # positions = j mod step
        neg = np.where(p != 0, p < 0, neg)
    tot = np.stack([t[:, j::WC].sum(axis=1) for j in range(WC)], axis=1)
    if WC == 1:
        return np.repeat(neg, W, axis=1)
    return np.tile(leaf((neg, np.abs(tot)), fb[W - WC:]), (1, W // WC))


RUNS = {4: ["0011", "0001"],
        8: ["00000111", "00000011", "00000110", "00001011", "00001111", "00000001"],
        16: ["0000000000000111", "0000000000010111", "0000000000000011", "0000000001111111",
             "0000000000000110", "0000000000001111", "0000000001101111", "0000000000000001"]}


def edge_rows(W, mmax):
    """every sign pattern on all-zero rows (-0 at position 0 among them), on one equal magnitude and on
    the largest; and rows whose halves cancel exactly"""
    sg = ((np.arange(1 << W)[:, None] >> np.arange(W)[None, :]) & 1).astype(bool)
    parts = [(sg, np.full(sg.shape, v, np.int64)) for v in (0, 1, mmax)]
    rng = np.random.default_rng(31 * W + mmax)
    m = rng.integers(0, mmax + 1, (20000, W // 2))
    s = rng.integers(0, 2, (20000, W // 2)).astype(bool)
    parts.append((np.concatenate([s, ~s], axis=1), np.concatenate([m, m], axis=1)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.fixture(scope="module", params=[("exhaustive", 4, 7), ("random", 8, 62), ("random", 8, 3),
                                        ("random", 16, 31), ("random", 16, 2), ("edges", 8, 62), ("edges", 16, 31)],
                ids=lambda c: "%s-W%d-m%d" % c)
def rows(request):
    kind, W, mmax = request.param
    if kind == "exhaustive":
        return W, tlb.exhaustive(W, mmax)
    if kind == "edges":
        return W, edge_rows(W, mmax)
    return W, tlb.tie_heavy(np.random.default_rng(2000 * W + mmax), 300000, W, mmax)


def test_add_chain_rule_is_the_recursion(rows):
    W, lam = rows
    for pattern in RUNS[W]:
        fb = bits(pattern)
        assert add_levels(fb) >= 1
        np.testing.assert_array_equal(add_chain_rule(lam, fb), leaf(lam, fb), err_msg=pattern)
    t = np.where(lam[0], -lam[1], lam[1])
    zero = (t[:, :W // 2] + t[:, W // 2:] == 0).any(axis=1)
    assert zero.mean() > 0.01, zero.mean()   # (zero sums are exercised)


# ---- the packed halves as shipped -------------------------------------------------------------
def unpack(v):
    return (v & U32(0xFFFF)).astype(np.int64), (v >> U32(16)).astype(np.int64)


def add_chain_packed(M, S, fb, bias):
    """leaf_ms on rows of W lanes: the chain, then the child on the first WC lanes (restated by the
    recursion on each half) and copy_block"""
    W = len(fb)
    K = add_levels(fb)
    WC = W >> K
    b2 = U32(bias * 0x00010001)
    v = pk_mad(M, S | U32(0x00010001), b2)
    m, H = S.copy(), W // 2
    for k in range(1, K + 1):
        v = v + partner(v, H)                                 # one 32-bit add of both halves
        m = pk_sra15(pk_sub(pk_add(v, m), U32(((bias << k) * 0x00010001) & 0xFFFFFFFF)), 0)
        H //= 2
    if WC == 1:
        return np.repeat(m[:, :1], W, axis=1)                 # row_bcast of the block's first lane
    d = pk_sub(v, U32(((bias << K) * 0x00010001) & 0xFFFFFFFF))
    Mc = pk_abs_i16(d, d)
    out = []
    for mc, mm in zip(unpack(Mc[:, :WC]), unpack(m[:, :WC])):
        assert set(np.unique(mm)) <= {0, 0xFFFF}
        out.append(leaf((mm != 0, mc), fb[W - WC:]))
    x = pack(out[0] * 0xFFFF, out[1] * 0xFFFF)
    return np.tile(x, (1, W // WC))


def add_ok(q, p16, W, n):
    """LeafBlock<W>::add_ok(n) of polar_sc_device.h"""
    mmax, bias = tlb.leaf_block(q, p16, W)[:2]
    return bias > mmax + 1 and n * (bias + mmax) < 0x10000 and n * mmax + 1 < 0x8000


def test_bounds():
    """where the halves do not hold n summands the device takes the recursion: n * BIAS * (1 + 2 / W)
    reaches 2^16 only for whole-word runs inside a PAR 32 / 64 word at LLR_BITS 8 / 9 and for runs of 8
    inside a PAR 64 word at LLR_BITS 9 (REP_OK is add_ok(W))"""
    bad = {(q, p16, W, n) for q in (5, 6, 7, 8, 9) for p16 in (1, 2, 4) for W in (4, 8, 16)
           for n in (2, 4, 8, 16) if n <= W and not add_ok(q, p16, W, n)}
    assert bad == {(9, 4, 16, 8), (9, 4, 16, 16), (9, 4, 8, 8), (9, 2, 16, 16), (8, 4, 16, 16)}, bad
    for q in (5, 6, 7, 8, 9):
        for p16 in (1, 2, 4):
            for W in (4, 8):
                assert add_ok(q, p16, W, W) == tlb.leaf_block(q, p16, W)[3]


def bound_rows(W, mmax):
    lam = tlb.bound_cases(W, mmax) if W <= 8 else tlb.tie_heavy(np.random.default_rng(55 + mmax), 40000, W, mmax)
    es, em = edge_rows(W, mmax) if W <= 8 else edge_rows(8, mmax)
    if W == 16:     # (2^16 sign patterns are in the rule test; here the 2^8 of each half, doubled)
        es, em = np.concatenate([es, es], axis=1), np.concatenate([em, em], axis=1)
        top = np.random.default_rng(56 + mmax).integers(0, 2, (20000, W)).astype(bool), np.full((20000, W), mmax, np.int64)
        es, em = np.concatenate([es, top[0]]), np.concatenate([em, top[1]])
    return np.concatenate([lam[0], es]), np.concatenate([lam[1], em])


@pytest.mark.parametrize("p16", [1, 2, 4])
@pytest.mark.parametrize("q", [5, 6, 7, 8, 9])
@pytest.mark.parametrize("W", [4, 8, 16])
def test_packed_chain(q, W, p16):
    mmax, bias = tlb.leaf_block(q, p16, W)[:2]
    lam = bound_rows(W, mmax)
    M, S, perm = tlb.two_frames(lam)
    done = 0
    for pattern in RUNS[W][:4] + RUNS[W][-1:]:
        fb = bits(pattern)
        if not add_ok(q, p16, W, 1 << add_levels(fb)):     # (test_bounds: the device recurses)
            continue
        r = leaf(lam, fb)
        np.testing.assert_array_equal(add_chain_packed(M, S, fb, bias), pack(r * 0xFFFF, r[perm] * 0xFFFF), err_msg=pattern)
        done += 1
    assert done >= 2


def test_bound_is_needed():
    """beyond add_ok the 32-bit add does carry into the other half: a run LeafBlock turns away fails"""
    q, p16, W, fb = 9, 4, 16, bits("0000000000000001")
    assert not add_ok(q, p16, W, 16)
    mmax, bias = tlb.leaf_block(q, p16, W)[:2]
    lam = bound_rows(W, mmax)
    M, S, perm = tlb.two_frames(lam)
    r = leaf(lam, fb)
    assert (add_chain_packed(M, S, fb, bias) != pack(r * 0xFFFF, r[perm] * 0xFFFF)).any()


# ---- the compiled kernels ---------------------------------------------------------------------
PARENT_C2_KEY = 0xC1E4CF71552C91A4   # code_key of the C2 kernel before this change
SWITCH = "POLAR_LEAF_ADD_RECURSE"


@pytest.fixture(scope="module")
def c2(pkg):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import pair_census as pc
    import rtc_isa_check as ric
    return pc, ric, pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()


def test_c2_budget_and_former_form(c2):
    from test_rep_carry import code_key
    _, ric, src = c2
    co = ric.clang_compile(src)
    kd = ric.kernel_descriptors(co)["polar_sc_mask_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_kernel"]
    assert meta["vgpr_count"] <= 98 and not meta["agpr_count"], (kd, meta)
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0 and meta["private_segment_fixed_size"] == 0
    former = ric.clang_compile("#define %s\n" % SWITCH + src)
    assert code_key(ric, former)[0] == PARENT_C2_KEY, "%016x" % code_key(ric, former)[0]
    assert code_key(ric, co)[0] != PARENT_C2_KEY


def test_c2_priced_cycles_fall(c2):
    pc, _, src = c2
    plain = pc.drop_unaligned_copy(src)
    new = pc.cycles_census(plain, no_rep_fallback=True)
    old = pc.cycles_census(plain, defines=(SWITCH,), no_rep_fallback=True)
    print("kernel %d priced VALU, %.0f cycles; with the switch %d, %.0f" % (new[1], new[0], old[1], old[0]))
    assert new[0] < old[0] and new[1] < old[1], (new[:2], old[:2])
    for res in (new, old):
        assert sum(res[2].values()) <= 0.03 * res[1], res[2]


PROBE = """#define POLAR_LANE_REMAP 1
#include "polar_sc_device.h"
using namespace polar;
extern "C" __global__ void k(const u32 *in, u32 *out) {
  Lanes ln; ln.init(threadIdx.x & 15u);
  out[threadIdx.x] = leaf_ms<0x%xu, %d, %d>(in[threadIdx.x], in[threadIdx.x + 64], ln); }
"""


@pytest.mark.parametrize("fb,B,W,live", [(0xE000, 0, 16, True), (0xC0, 0, 8, True), (0xC000, 12, 4, True), (0x6A, 0, 8, False)])
def test_the_switch_is_live(c2, tmp_path, fb, B, W, live):
    """a block with a run compiles to other code with the switch; a block without one (0101 0110) to
    the same"""
    pc = c2[0]
    src = PROBE % (fb, B, W)

    def text(tag, defines):
        d = tmp_path / tag
        d.mkdir()
        return [line for line in pc.compile_asm(src, str(d), defines).split("\n") if "__hip_cuid_" not in line]

    assert (text("own", ["-D" + SWITCH]) != text("base", [])) == live
