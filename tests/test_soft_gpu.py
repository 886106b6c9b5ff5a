"""Float channel values on the GPU: the quantizer kernel against three lines of
numpy, and decode_soft -- fused per-mask kernel or quantizer + decode -- against decode() of the
numpy-quantized frames and the oracle. The inputs carry every value at which the reference's
(short)(v * beta) can go wrong: signed zeros, k / beta and its neighbours, truncation toward zero,
the clamp's edges, values that wrap, infinities and NaN."""
import functools

import numpy as np
import pytest

from sc_polar_decoder_hls_amd import _plansets

DTYPES = _plansets.SOFT_DTYPES


def quant_np(v, beta, lo, hi):
    """sc_quantizer.h:76-80 on fp32 values: (short)(v * beta) as x86-64 converts it, clamped"""
    p = v.astype(np.float32) * np.float32(beta)
    ok = (p > np.float32(-2147483648.0)) & (p < np.float32(2147483648.0))       # (NaN: neither)
    i32 = np.where(ok, np.trunc(np.where(ok, p, 0)), -2147483648.0).astype(np.int64).astype(np.int32)
    return np.clip(i32.astype(np.int16), lo, hi)


def edge_values(beta):
    b = np.float32(beta)
    out = [0.0, -0.0, -0.2, 7.75, -7.75, 8.0, -8.0, 1e4, -1e4, np.inf, -np.inf, np.nan]
    for k in (1, 31, 32):
        x = np.float32(k) / b
        for s in (1, -1):
            out += [s * x, s * np.nextafter(x, np.float32(0)), s * np.nextafter(x, np.float32(np.inf))]
    return np.array(out, np.float32)


@functools.lru_cache(maxsize=None)
def soft_values(n, dtype, beta=4, seed=0):
    """(torch CPU tensor of `dtype`, its values as fp32): AWGN BPSK soft values at 2 dB (rate 1/2) with the
    edge values at random places, rounded to `dtype`"""
    import torch
    rng = np.random.default_rng(1000 * n + seed)
    sigma = 1.0 / np.sqrt(10.0 ** 0.2)
    v = (rng.choice([-1.0, 1.0], n) + sigma * rng.standard_normal(n)).astype(np.float32)
    e = rng.permutation(edge_values(beta))[:n]
    v[rng.choice(n, e.size, replace=False)] = e
    t = torch.from_numpy(v).to(getattr(torch, dtype))
    return t, t.float().numpy()


def check_quantize(pkg, torch, dtype, bits, beta, lim, n, in_off, out_off):
    t, v = soft_values(n, dtype, beta)
    src = torch.zeros(n + in_off, dtype=t.dtype, device="cuda")
    src[in_off:] = t.cuda()
    dst = torch.full((n + out_off + 1,), 77, dtype=torch.int8 if bits == 8 else torch.int16, device="cuda")
    got = pkg.quantize(src[in_off:], beta, -lim, lim, bits=bits, out=dst[out_off:out_off + n])
    np.testing.assert_array_equal(got.cpu().numpy(), quant_np(v, beta, -lim, lim))
    guard = dst.cpu().numpy()
    assert guard[-1] == 77 and (out_off == 0 or guard[0] == 77)      # nothing written outside


@pytest.mark.gpu
@pytest.mark.parametrize("out_off", [0, 1])
@pytest.mark.parametrize("in_off", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 1000])
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_against_numpy(pkg, cuda, dtype, bits, n, in_off, out_off):
    check_quantize(pkg, cuda, dtype, bits, 4, 31, n, in_off, out_off)


@pytest.mark.gpu
def test_quantize_int16_bounds(pkg, cuda):
    check_quantize(pkg, cuda, "float32", 16, 64, 255, 1000, 0, 1)


@functools.lru_cache(maxsize=None)
def frames(name, dtype, batch, beta=4, lim=31):
    """(float frames as a torch CPU tensor [batch, N], their numpy-quantized int16 frames)"""
    N = _plansets.soft_mask(name).size
    t, v = soft_values(batch * N, dtype, beta)
    return t.view(batch, N), quant_np(v, beta, -lim, lim).reshape(batch, N)


def check_decode(pkg, torch, oracle_mod, dec, name, dtype, batch, beta=4, lim=31, offset=0, llr_bits=6):
    t, q = frames(name, dtype, batch, beta, lim)
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device="cuda")
    buf[offset:] = t.reshape(-1).cuda()
    got = dec.decode_soft(buf[offset:].view(batch, dec.N), beta, -lim, lim)
    q_t = torch.from_numpy(q.astype(np.int8) if llr_bits <= 8 else q).cuda()
    np.testing.assert_array_equal(got.cpu().numpy(), dec.decode(q_t).cpu().numpy())
    ref = oracle_mod.decode_fsm(dec.mask, q[:8] if llr_bits > 8 else q[:8].astype(np.int8), llr_bits=llr_bits)
    np.testing.assert_array_equal(pkg.unpack_bits(got.cpu().numpy()[:8], dec.N), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 19, 67])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _plansets.SOFT_FUSED_MASKS)
def test_fused_decode(pkg, cuda, oracle_mod, name, dtype, batch):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    assert dec.soft_info(dtype, batch)["fused"] == 1
    check_decode(pkg, cuda, oracle_mod, dec, name, dtype, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_decode_unaligned_input(pkg, cuda, oracle_mod, dtype):
    dec = pkg.Decoder(_plansets.soft_mask("FB_N256_K128"))
    assert dec.soft_info(dtype, 19)["fused"] == 1
    check_decode(pkg, cuda, oracle_mod, dec, "FB_N256_K128", dtype, 19, offset=1)


@pytest.mark.gpu
def test_fused_decode_8_bit_llrs(pkg, cuda, oracle_mod):
    cfg = pkg.default_config()
    cfg.llr_bits = 8
    dec = pkg.Decoder(_plansets.soft_mask("FB_N128_K64"), cfg)
    assert dec.soft_info("float32", 19)["fused"] == 1
    check_decode(pkg, cuda, oracle_mod, dec, "FB_N128_K64", "float32", 19, beta=16, lim=127, llr_bits=8)


@pytest.mark.gpu
@pytest.mark.parametrize("name,llr_bits,tuning,beta,lim", [
    ("FB_N128_K64", 6, {"kernel": 1}, 4, 31), ("frozen_n_2048_k_1024", 6, None, 4, 31),
    ("frozen_n_2048_k_1024", 9, None, 32, 255)])
def test_two_launch_decode(pkg, cuda, oracle_mod, name, llr_bits, tuning, beta, lim):
    cfg = pkg.default_config()
    cfg.llr_bits = llr_bits
    dec = pkg.Decoder(_plansets.soft_mask(name), cfg, tuning=tuning)
    assert dec.soft_info("float16", 5) == {"fused": 0, "regs": 0, "code_key": "%016x" % 0,
                                           "workspace_bytes": 5 * dec.N * (2 if llr_bits == 9 else 1)}
    check_decode(pkg, cuda, oracle_mod, dec, name, "float16", 5, beta, lim, llr_bits=llr_bits)


@pytest.mark.gpu
def test_fused_decode_in_a_graph(pkg, cuda):
    torch = cuda
    dec = pkg.Decoder(_plansets.soft_mask("FB_N128_K64"))
    t, _ = frames("FB_N128_K64", "bfloat16", 19)
    v = t.cuda()
    eager = dec.decode_soft(v).cpu().numpy()                  # (warm-up: loads the kernel)
    out = torch.zeros((19, dec.words), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_soft(v, out=out, stream=s)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), eager)
