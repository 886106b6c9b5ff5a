"""Soft-output (SCAN) decoding on the GPU: decode_scan against tests/scan_ref.py on
every extrinsic value and every hard bit. Frames per case as in tests/test_list_precoded_gpu.py (9 at
N <= 128, 5 at N = 1024: a partial block): AWGN at 1 dB on random codewords; an all-zero frame (every f
is 0); +127 everywhere (the right spine doubles alpha per level: the clamp is reached at N = 1024);
+-127 on a codeword with -128 sprinkled in."""
import functools

import numpy as np
import pytest

import scan_ref
import util
from sc_polar_decoder_hls_amd import _plansets

MASKS = ("spc_n32", "FB_N128_K64", "FB_N1024_K512", "frozen_n_1024_k_922")
GUARD = 0x5A5A


def sent(mask, n, seed):
    """n random information rows [n, K] and their codewords [n, N]"""
    u = np.zeros((n, mask.size), dtype=np.uint8)
    bits = np.random.default_rng(seed).integers(0, 2, size=(n, int(mask.sum())), dtype=np.uint8)
    u[:, mask.astype(bool)] = bits
    return bits, util.encode_np(u)


@functools.lru_cache(maxsize=None)
def frames(name):
    mask, rng = _plansets.soft_mask(name), np.random.default_rng(13)
    x = sent(mask, 5 if mask.size == 1024 else 9, seed=mask.size + 1)[1]
    sigma = 1.0 / np.sqrt(2.0 * mask.sum() / mask.size * 10.0 ** 0.1)
    llr = np.clip(np.trunc(4.0 * (np.where(x == 1, -1.0, 1.0) + sigma * rng.standard_normal(x.shape))), -31, 31).astype(np.int8)
    llr[-3] = 0
    llr[-2] = 127
    llr[-1] = np.where(x[-1] == 1, np.where(rng.random(mask.size) < 0.3, -128, -127), 127)
    llr.setflags(write=False)
    return llr


def run(cuda, dec, llr, iterations):
    """decode_scan into buffers with a guard row: (ext [B, N] int64, hard bits [B, N] uint8)"""
    B = llr.shape[0]
    ext = cuda.full((B + 1, dec.N), GUARD, dtype=cuda.int16, device="cuda")
    hard = cuda.full((B + 1, dec.words), GUARD, dtype=cuda.int64, device="cuda")
    dec.decode_scan(cuda.from_numpy(np.array(llr)).cuda(), iterations, out=ext[:B], hard=hard[:B])
    assert (ext[B] == GUARD).all() and (hard[B] == GUARD).all()                # nothing past the batch
    bits = np.unpackbits(hard[:B].cpu().numpy().view(np.uint8), axis=1, bitorder="little")
    assert not bits[:, dec.N:].any()
    return ext[:B].cpu().numpy().astype(np.int64), bits[:, :dec.N], hard[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("name", MASKS)
def test_parity(pkg, cuda, name, iterations):
    mask = _plansets.soft_mask(name)
    want_ext, want_hard = scan_ref.scan(mask, frames(name), iterations)
    ext, hard, _ = run(cuda, pkg.Decoder(mask), frames(name), iterations)
    np.testing.assert_array_equal(ext, want_ext)
    np.testing.assert_array_equal(hard, want_hard)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MASKS)
def test_noiseless_round_trip(pkg, cuda, name):
    mask = _plansets.soft_mask(name)
    dec, (bits, x) = pkg.Decoder(mask), sent(mask, 5, seed=3)
    _, hard, rows = run(cuda, dec, np.where(x == 1, -31, 31).astype(np.int8), 1)
    np.testing.assert_array_equal(hard, x)
    info = dec.extract_info(rows.contiguous()).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(pkg.unpack_bits(info, dec.K), bits)


@pytest.mark.gpu
@pytest.mark.parametrize("fill,want", [(0, scan_ref.INF), (1, 0)])
def test_all_frozen_and_all_info(pkg, cuda, fill, want):
    llr = np.random.default_rng(5).integers(-128, 128, size=(3, 64)).astype(np.int8)
    ext, _, _ = run(cuda, pkg.Decoder(np.full(64, fill, np.uint8)), llr, 2)
    assert (ext == want).all()


@pytest.mark.gpu
def test_graph_replay(pkg, cuda):
    """two iterations captured into a graph after prepare: three replays against the eager result"""
    dec = pkg.Decoder(_plansets.soft_mask("FB_N128_K64"))
    x = cuda.from_numpy(np.array(frames("FB_N128_K64"))).cuda()
    dec.prepare(x.shape[0])
    eager = [t.clone() for t in dec.decode_scan(x, 2)]
    out, hard = (cuda.empty_like(t) for t in eager)
    s, g = cuda.cuda.Stream(), cuda.cuda.CUDAGraph()
    s.wait_stream(cuda.cuda.current_stream())
    with cuda.cuda.stream(s), cuda.cuda.graph(g, stream=s):
        dec.decode_scan(x, 2, out=out, hard=hard, stream=s)
    for _ in range(3):
        out.fill_(0x33)
        hard.fill_(0x33)
        g.replay()
        cuda.cuda.synchronize()
        assert cuda.equal(out, eager[0]) and cuda.equal(hard, eager[1])
