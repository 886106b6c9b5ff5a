"""REP nodes of the generated kernels whose total is 0 (polar_sc_jit.cpp, the REP case of Gen::op
and its prelude): the two's complement value chain on 16-bit halves, and the sign-magnitude sign
of a zero total from the last word alone, carried as a mask through that word's butterfly and the
last accumulate step (the kernel computes it when some frame of the wave has a zero total; a total
that is not 0 keeps its sign under it). Restated in numpy on uint16 halves (wrapping, as the packed
instructions do) and checked against the oracle's REP:

  * oracle.rep_add_tree16 (the exact pair tree of a word accumulated with the 511 clamp), chained
    over the words of a node;
  * oracle.decode_fsm on whole frames: in a code of 64 n LLRs with only bit 16 n - 1 unfrozen the
    first quarter is one REP node of n words (the children of the root are never pruned nodes, so
    the node sits one level below them), and the decoded codeword is the decision repeated over
    that quarter.
"""
import itertools

import numpy as np
import pytest

U16 = np.uint16
BIAS = 0x200          # per element, every LLR_BITS (the prelude's bounds say why it may be fixed)


def sat(q, par=16):
    """REPSAT of SIGMAG: 2^(Q + log2 PAR - 1) - 1"""
    return (1 << (q + par.bit_length() - 2)) - 1


def sra15(v):
    """per half: arithmetic shift right by 15 (0xFFFF where bit 15 is set)"""
    return np.where(v & U16(0x8000), U16(0xFFFF), U16(0)).astype(U16)


def carried(fs, fm, q=6, par=16, acc0=None):
    """decision (0 / 1) of a REP node from its F values: fs, fm [B, n, 16] sign bits and magnitudes
    (position order). acc0: the accumulator before word 0 (the kernel starts at 0; the bound
    tests start at +-REPSAT)."""
    B, n, _ = fs.shape
    rs = sat(q, par)
    pm1 = np.where(fs != 0, U16(0xFFFF), U16(1)).astype(U16)
    val = (fm.astype(U16) * pm1 + U16(BIAS)).astype(U16)          # REP_FSB: |F| x (+1 / -1) + 512
    acc = np.zeros(B, U16) if acc0 is None else np.asarray(acc0).astype(np.int16).view(U16).copy()
    for w in range(n - 1):                                        # row_sum_biased + rep_acc
        tot = val[:, w].sum(axis=1, dtype=np.uint32)
        assert int(tot.max()) < 0x10000                           # (no carry into the other half)
        t = (acc + tot.astype(U16) - U16(0x2000)).astype(U16).view(np.int16)
        acc = np.clip(t, -rs, rs).astype(np.int16).view(U16)
    v = val[:, n - 1].copy()
    m = np.where(fs[:, n - 1] != 0, U16(0xFFFF), U16(0)).astype(U16)   # plane_mask: the F sign bit
    pos = np.arange(16)
    for K, H in ((1, 8), (2, 4), (3, 2), (4, 1)):                 # rep_carry_level<H, K>
        assert int(v.astype(np.uint32).max()) * 2 < 0x10000
        v = (v + v[:, pos ^ H]).astype(U16)
        m = sra15((v + m - U16((BIAS << K) & 0xFFFF)).astype(U16))
    acc = (acc + v[:, 0] - U16(0x2000)).astype(U16)               # the last step, unclamped
    nz = acc != 0                                                 # (the kernel's plain sign where no total is 0)
    assert (sra15(acc)[nz] == sra15((acc + m[:, 0]).astype(U16))[nz]).all()
    return (sra15((acc + m[:, 0]).astype(U16)) & U16(1)).astype(np.uint8)


def sm_pattern(s, m, q):
    return (s.astype(np.uint32) << (q - 1)) | m.astype(np.uint32)


def oracle_chain(oracle_mod, fs, fm, q=6):
    """decision by oracle.rep_add_tree16 chained over the words (PAR 16: an 11-bit accumulator at
    LLR_BITS 6, sign in its top bit)"""
    W = q + 5
    out = np.zeros(len(fs), np.uint8)
    pat = sm_pattern(fs, fm, q)
    for b in range(len(fs)):
        acc = 0
        for w in range(fs.shape[1]):
            acc = oracle_mod.rep_add_tree16(pat[b, w], acc)
        out[b] = (acc >> (W - 1)) & 1
    return out


# ---- the packed bounds, LLR_BITS 5..9, PAR 16..64 ------------------------------------------------
@pytest.mark.parametrize("q", [5, 6, 7, 8, 9])
@pytest.mark.parametrize("par", [16, 32, 64])
def test_packed_bounds(q, par):
    qmag, rs = (1 << (q - 1)) - 1, sat(q, par)
    assert BIAS > qmag + 1                      # an element with the carried -1 stays positive
    assert 16 * (BIAS + qmag) < 0x10000         # 16 elements do not carry into the other half
    assert 16 * qmag + 1 < 0x8000               # sum + m - K x BIAS keeps its sign in 16 bits
    assert rs + 16 * qmag + 1 < 0x8000          # acc + T + m keeps its sign in 16 bits
    # the extremes through the model: every element +-QMAG on an accumulator at +-REPSAT
    for n in (1, 2):
        for sgn in (0, 1):
            fs = np.full((2, n, 16), sgn, np.int32)
            fm = np.full((2, n, 16), qmag, np.int32)
            T = (-16 if sgn else 16) * qmag
            exp = []
            for acc in (rs, -rs):
                for _ in range(n - 1):
                    acc = max(-rs, min(rs, acc + T))
                assert acc + T != 0
                exp.append(int(acc + T < 0))
            np.testing.assert_array_equal(carried(fs, fm, q, par, acc0=np.array([rs, -rs])), exp)


# ---- one word, exhaustive over small values and -0 at positions 0, 1, 2, 4, 8 ---------------------
def test_one_word_exhaustive(oracle_mod):
    vals = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]      # (sign, magnitude): +0, -0, +-1, +-2
    combos = list(itertools.product(range(6), repeat=5))
    fs = np.zeros((len(combos), 1, 16), np.int32)
    fm = np.zeros((len(combos), 1, 16), np.int32)
    for c, combo in enumerate(combos):
        for p, k in zip((0, 1, 2, 4, 8), combo):
            fs[c, 0, p], fm[c, 0, p] = vals[k]
    got = carried(fs, fm)
    ref = oracle_chain(oracle_mod, fs, fm)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, (bad[:5], [combos[i] for i in bad[:5]])
    assert 0 < ref.sum() < len(ref)


# ---- the chain of rep_add_tree16 on a sample of the random cases ---------------------------------
def _tie_heavy(rng, B, n, q=6):
    """F values: mostly small with -0, some words all zero, some frames saturating"""
    qmag = (1 << (q - 1)) - 1
    fm = rng.choice(np.array([0, 0, 0, 1, 1, 2]), size=(B, n, 16)).astype(np.int32)
    fs = rng.integers(0, 2, size=(B, n, 16)).astype(np.int32)
    kind = rng.integers(0, 8, B)
    big = kind == 0                                               # saturating totals: |acc| reaches REPSAT
    fm[big] = rng.integers(qmag - 2, qmag + 1, size=(int(big.sum()), n, 16))
    fs[big] = rng.integers(0, 2, size=(int(big.sum()), 1, 1))
    fs[big, n - 1] = rng.integers(0, 2, size=(int(big.sum()), 16))
    if n > 1:
        fm[big, n - 1] = rng.choice(np.array([0, 1]), size=(int(big.sum()), 16))
    zw = rng.random((B, n)) < 0.3                                 # all-zero words (+0 and -0)
    fm[zw] = 0
    return fs, fm


@pytest.mark.parametrize("n", [1, 2, 4, 8, 32])
def test_chain_against_rep_add_tree16(oracle_mod, n):
    rng = np.random.default_rng(7100 + n)
    fs, fm = _tie_heavy(rng, 4000 // n + 200, n)
    got, ref = carried(fs, fm), oracle_chain(oracle_mod, fs, fm)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, bad[:8]


# ---- whole frames through decode_fsm: 300 k cases -------------------------------------------------
def rep_mask(n):
    """N = 64 n: the first quarter is a REP node of n words, the rest is frozen"""
    m = np.zeros(64 * n, np.uint8)
    m[16 * n - 1] = 1
    return m


def node_f(util, llr, n, q=6):
    """the F values the REP node reads: F of F of the channel quarters, as [B, n, 16] signs and magnitudes"""
    s, m = util.sm_from_llr(llr, q)
    h = 32 * n
    s, m = util.F((s[:, :h], m[:, :h]), (s[:, h:], m[:, h:]))
    h = 16 * n
    s, m = util.F((s[:, :h], m[:, :h]), (s[:, h:], m[:, h:]))
    return s.reshape(-1, n, 16), m.reshape(-1, n, 16)


def _frames(rng, B, n, q=6):
    """channel frames whose F values are tie-heavy: LLRs in {-2 .. 2, the channel's +0 pattern}; an
    eighth of the frames saturate the accumulator"""
    top = (1 << (q - 1)) - 1
    small = np.array([-2, -1, 0, 1, 2, -(1 << (q - 1))])
    llr = rng.choice(small, size=(B, 64 * n))
    big = rng.integers(0, 8, B) == 0
    nb = int(big.sum())
    sgn = rng.choice(np.array([-1, 1]), size=(nb, 1))
    llr[big] = sgn * rng.integers(top - 1, top + 1, size=(nb, 64 * n))
    for k in range(4):                                                         # the last word decides ties
        llr[big, 16 * n * k + 16 * (n - 1):16 * n * (k + 1)] = rng.choice(small, size=(nb, 16))
    zw = np.repeat(rng.random((B, n)) < 0.25, 16, axis=1)                      # all-zero words
    left = llr[:, :16 * n]
    left[zw] = 0
    return llr.astype(np.int16 if q > 8 else np.int8)


@pytest.mark.parametrize("n,B", [(1, 100000), (2, 80000), (4, 60000), (8, 40000), (32, 20000)])
def test_whole_frames_against_decode_fsm(oracle_mod, n, B):
    import util
    rng = np.random.default_rng(7200 + n)
    llr = _frames(rng, B, n)
    mask = rep_mask(n)
    h = 16 * n
    fs, fm = node_f(util, llr, n)
    got = carried(fs, fm)
    ref = oracle_mod.decode_fsm(mask, llr)
    assert (ref[:, h:] == 0).all() and (ref[:, :h] == ref[:, :1]).all()
    bad = np.nonzero(got != ref[:, 0])[0]
    assert bad.size == 0, "%d of %d decisions differ (first %s)" % (bad.size, B, bad[:8])
    # the cases the carry exists for are there: zero totals, zero last words, saturated accumulators
    tot = np.where(fs != 0, -fm, fm).reshape(B, n, 16).sum(axis=2)
    # (n - 1 words of at most 16 x 31 reach the clamp from 3 words on)
    assert (tot[:, -1] == 0).mean() > 0.02 and (np.abs(tot[:, :-1].sum(axis=1)) >= 511).any() == (n >= 4)
    assert 0.1 < ref[:, 0].mean() < 0.9


@pytest.mark.parametrize("q", [5, 8, 9])
def test_whole_frames_other_widths(oracle_mod, q):
    import util
    rng = np.random.default_rng(7300 + q)
    n, B = 4, 6000
    llr = _frames(rng, B, n, q)
    fs, fm = node_f(util, llr, n, q)
    got = carried(fs, fm, q)
    ref = oracle_mod.decode_fsm(rep_mask(n), llr, llr_bits=q)
    np.testing.assert_array_equal(got, ref[:, 0])


# ---- the compiled C2 kernel -------------------------------------------------------------------
PARENT_C2_KEY = 0xF0BCFE2DB4F5B1B7   # code_key of the C2 kernel before this change (profiles/r09_ab/summary.txt)


def code_key(ric, co):
    """polar_sc_jit.cpp code_key: FNV-1a over the executable sections and .rodata; and the bytes of
    the executable sections"""
    secs, shstrndx = ric.elf_sections(co)
    names = secs[shstrndx]
    h, text = 1469598103934665603, 0
    for s in secs:
        name = co[names[4] + s[0]:].split(b"\0", 1)[0]
        if s[1] == 1 and ((s[2] & 4) or name == b".rodata"):
            text += s[5] if s[2] & 4 else 0
            for b in co[s[4]:s[4] + s[5]]:
                h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h, text


@pytest.fixture(scope="module")
def c2(pkg):
    import os
    import sys
    import util
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import rtc_isa_check as ric
    return ric, pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()


def test_c2_budget_and_former_form(c2):
    """no scratch, no AGPRs, fewer registers and less code than the former form, which
    -DPOLAR_REP_FALLBACK still builds: the parent's machine code"""
    ric, src = c2
    co = ric.clang_compile(src)
    kd = ric.kernel_descriptors(co)["polar_sc_mask_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_kernel"]
    assert meta["vgpr_count"] <= 104 and kd["regs_unified"] <= 104 and not meta["agpr_count"], (kd, meta)
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0 and meta["private_segment_fixed_size"] == 0
    assert meta["max_flat_workgroup_size"] == 256
    former = ric.clang_compile("#define POLAR_REP_FALLBACK\n" + src)
    key, text = code_key(ric, former)
    assert key == PARENT_C2_KEY, "%016x" % key
    assert ric.metadata(former)["polar_sc_mask_kernel"]["vgpr_count"] > meta["vgpr_count"]
    print("executable bytes: %d, former form %d" % (code_key(ric, co)[1], text))
    assert code_key(ric, co)[1] < 0.85 * text


def test_c2_no_exact_chain(c2, tmp_path):
    import subprocess
    ric, src = c2
    assert src.count("if (rep_any_zero(acc_)) {") == 14 and src.count("rep_carry_level<8, 1>") == 7
    p = tmp_path / "k.hip"
    p.write_text("#include <hip/hip_runtime.h>\n" + src)
    pre = subprocess.run([ric.CLANG, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-w",
                          "-I" + ric.CSRC, "-E", "-P", str(p)], check=True, capture_output=True, text=True).stdout
    kernel = pre[pre.index("polar_sc_mask_kernel("):]
    assert "row_add_tree" not in kernel and "G_sm<REPSAT>" not in kernel
    assert kernel.count("rep_any_zero(acc_)") == 7 and kernel.count("rep_carry_level<8, 1>") == 7
