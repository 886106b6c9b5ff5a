"""G on split words as one multiply-add (polar_sc_device.h G_split).

The split-word G takes the magnitudes ma, mb of a' and b per 16-bit half, and x = sign(a') ^
sign(b). It returns min(|lambda|, GSAT) and the flag LT = |a| < |b|; the caller's output sign is
sign(b) ^ (x & ~LT), so LT matters only where x is set. Two forms:

  select (-DPOLAR_G_BSEL): d = ma - mb, LT = d < 0, magnitude = x ? |d| : ma + mb
  multiply-add:            t = mb * (x ? -1 : +1) + ma (mod 2^16), LT = t < 0, magnitude = |t|

Restated here in numpy on 16-bit halves, every ma, mb of the magnitude range and both x: equal
magnitudes everywhere, equal LT wherever x = 1, hence equal output signs for either sign(b). The
second case set is the widest stage magnitude (9-bit CA2, 511) with its clamp; the sum ma + mb
stays below 2^15, so |t| = t there. The compiled kernel is checked too: the C2 code object keeps
its register budget and carries the multiply-add (and the collected root sign planes).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import util


def _abs_i16(v):
    """v_pk_max_i16(v, -v) on one half: |v| of the two's complement value (0x8000 stays)"""
    s = v.astype(np.int16)
    return np.maximum(s, (-s.astype(np.int32)).astype(np.int16)).astype(np.uint16)


def g_select(ma, mb, x, gsat):
    d = (ma - mb).astype(np.uint16)
    xm = np.where(x, np.uint16(0xFFFF), np.uint16(0))
    m = (_abs_i16(d) & xm) | ((ma + mb).astype(np.uint16) & ~xm)
    return np.minimum(m, np.uint16(gsat)), d >> 15


def g_mad(ma, mb, x, gsat):
    mult = np.where(x, np.uint16(0xFFFF), np.uint16(0)) | np.uint16(1)   # -1 / +1
    t = (mb.astype(np.uint32) * mult + ma).astype(np.uint16)              # v_pk_mad_u16: modulo 2^16
    return np.minimum(_abs_i16(t), np.uint16(gsat)), t >> 15


@pytest.mark.parametrize("top,gsat", [(255, 15), (255, 63), (511, 255)])
def test_g_mad_equals_select(top, gsat):
    v = np.arange(top + 1, dtype=np.uint16)
    ma, mb = np.meshgrid(v, v, indexing="ij")
    for x in (0, 1):
        xs = np.full(ma.shape, bool(x))
        m0, lt0 = g_select(ma, mb, xs, gsat)
        m1, lt1 = g_mad(ma, mb, xs, gsat)
        np.testing.assert_array_equal(m1, m0, err_msg="magnitude, x = %d" % x)
        # what the kernels read of LT: the output sign sign(b) ^ (x & ~LT), for either sign(b)
        np.testing.assert_array_equal(x & ~lt1 & 1, x & ~lt0 & 1, err_msg="sign term, x = %d" % x)
        if x:
            np.testing.assert_array_equal(lt1, lt0, err_msg="LT where x = 1")
            np.testing.assert_array_equal(lt0, ma < mb)
        else:
            assert not lt1.any()   # t = ma + mb >= 0: the don't-care bits come out 0


def test_g_mad_halves_independent():
    """the packed form: two halves in one register, no carry from the low half's product or sum
    into the high half (v_pk_mad_u16 works per half)"""
    rng = np.random.default_rng(5)
    ma, mb = rng.integers(0, 256, (2, 2, 4096)).astype(np.uint16)
    x = rng.integers(0, 2, (2, 4096)).astype(bool)
    for h in range(2):
        m0, lt0 = g_select(ma[h], mb[h], x[h], 15)
        m1, lt1 = g_mad(ma[h], mb[h], x[h], 15)
        np.testing.assert_array_equal(m1, m0)
        np.testing.assert_array_equal(lt1[x[h]], lt0[x[h]])
    # the same through 32-bit words: per-half results packed equal the packed per-half inputs' results
    pack = lambda lo, hi: lo.astype(np.uint32) | (hi.astype(np.uint32) << 16)
    mult = pack(np.where(x[0], 0xFFFF, 1).astype(np.uint16), np.where(x[1], 0xFFFF, 1).astype(np.uint16))
    a, b = pack(ma[0], ma[1]), pack(mb[0], mb[1])
    t_lo = ((b & 0xFFFF) * (mult & 0xFFFF) + (a & 0xFFFF)) & 0xFFFF
    t_hi = ((b >> 16) * (mult >> 16) + (a >> 16)) & 0xFFFF
    np.testing.assert_array_equal(t_lo >> 15, g_mad(ma[0], mb[0], x[0], 15)[1])
    np.testing.assert_array_equal(t_hi >> 15, g_mad(ma[1], mb[1], x[1], 15)[1])


def test_c2_code_object_budget_and_mad(pkg):
    """The headline plan (N = 1024 K = 512, per-mask kernel) as the ROCm clang driver builds it:
    at most 128 registers per lane (4 waves per SIMD), no scratch, and one v_pk_mad_u16 per
    split-word G at least (the REP words use it too)."""
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import rtc_isa_check as ric
    dec = pkg.Decoder(util.mask("FB_N1024_K512"))
    info = dec.launch_info(65536)
    assert info["kernel"] == 1 and 0 < info["regs"] <= 128 and info["waves_per_block"] == 4, info
    src = dec.kernel_source()
    # (the root's sign planes are collected over 8 registers each and rebuilt by one v_perm_b32
    # per plane: two planes per 16 packed root registers)
    assert src.count("__builtin_amdgcn_perm(sa_[1], sa_[0], ") == 4, "root sign planes"
    co = ric.clang_compile(src)
    kd = ric.kernel_descriptors(co)["polar_sc_mask_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_kernel"]
    assert kd["regs_unified"] <= 128 and meta["vgpr_count"] <= 128 and not meta["agpr_count"], (kd, meta)
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0, kd
    assert meta["private_segment_fixed_size"] == 0, meta
    objdump = os.path.join(os.path.dirname(ric.CLANG), "llvm-objdump")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        asm = subprocess.run([objdump, "-d", f.name], capture_output=True, text=True, check=True).stdout
    n_g = src.count("G_split<")
    assert n_g > 100 and asm.count("v_pk_mad_u16") >= n_g, (n_g, asm.count("v_pk_mad_u16"))
