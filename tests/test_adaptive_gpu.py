"""Adaptive CRC-aided decoding on the GPU: crc_check against the bit-by-bit CRC on
rows whose verdict is known by construction, and decode_adaptive against the rule restated in plain
Python: successive cancellation from the oracle, the CRC from crc_bits, tests/list_ref.py on the
failing frames only; every information word, the rank and the stage.

Frames per case (67 at N <= 128: a 64-frame wave of the check and a partial one; 9 at N = 1024),
clipped to +-31: AWGN at Eb/N0 = 1 dB, then an all-zero frame (SC gives the zero payload, which
passes), a noise-free codeword of a crc_attach payload (passes) and a noise-free codeword whose
last check bit was flipped before encoding (SC returns exactly that payload: it fails and goes to
the list decoder), so that every case holds both stages."""
import functools

import numpy as np
import pytest

import list_ref
import util
from sc_polar_decoder_hls_amd import _plansets

MASKS = ("spc_n32", "FB_N128_K64", "FB_N1024_K512")
CRCS = {"crc8": (0x07, 8), "crc24": (0x864CFB, 24)}
GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def frames(pkg, name, crc_name, kind="mixed"):
    """kind "mixed": as above; "pass" / "fail": 65 noise-free codewords, none / all with the flipped bit"""
    mask, crc = _plansets.soft_mask(name), CRCS[crc_name]
    K, n = int(mask.sum()), 65 if kind != "mixed" else 9 if mask.size == 1024 else 67
    rng = np.random.default_rng(mask.size + crc[1])
    words = pkg.crc_attach(pkg.pack_bits(rng.integers(0, 2, size=(n, K - crc[1]), dtype=np.uint8)), K, *crc)
    u = np.zeros((2, n, mask.size), dtype=np.uint8)
    u[:, :, mask.astype(bool)] = pkg.unpack_bits(words, K)
    u[1, :, np.flatnonzero(mask)[-1]] ^= 1                      # the last check bit
    good, bad = (np.where(util.encode_np(v) == 1, -31, 31).astype(np.int8) for v in u)
    if kind != "mixed":
        llr = good if kind == "pass" else bad
    else:
        sigma = 1.0 / np.sqrt(2.0 * K / mask.size * 10.0 ** 0.1)
        llr = np.clip(np.trunc(4.0 * (good / 31.0 + sigma * rng.standard_normal(good.shape))), -31, 31).astype(np.int8)
        llr[-3], llr[-2], llr[-1] = 0, good[-2], bad[-1]
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def sc_reference(pkg, oracle_mod, name, crc_name, kind):
    """(SC information bits [B, K], stage [B]) of the case's frames"""
    mask, (poly, c) = _plansets.soft_mask(name), CRCS[crc_name]
    sc = util.encode_np(oracle_mod.decode_fsm(mask, np.array(frames(pkg, name, crc_name, kind))))[:, mask.astype(bool)]
    stage = [pkg.crc_bits(r[:r.size - c], poly, c) != list(r[r.size - c:]) for r in sc]
    return sc, np.array(stage, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def reference(pkg, oracle_mod, name, crc_name, L, kind="mixed"):
    sc, stage = sc_reference(pkg, oracle_mod, name, crc_name, kind)
    info, rank, bad = sc.copy(), np.zeros(len(sc), dtype=np.uint8), np.flatnonzero(stage)
    if bad.size:
        info[bad], rank[bad] = list_ref.decode(_plansets.soft_mask(name), frames(pkg, name, crc_name, kind)[bad], L,
                                               *CRCS[crc_name])
    return info, rank, stage


def run_adaptive(pkg, torch, dec, llr, L, crc):
    """decode_adaptive into rows followed by guard rows; (info words, rank, stage) as numpy"""
    B = llr.shape[0]
    buf = torch.full((B + 1, dec.info_words), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    rank, stage = (torch.full((B + 1,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2))
    dec.decode_adaptive(torch.from_numpy(np.array(llr)).cuda(), L, crc, out=buf[:B], rank=rank[:B], stage=stage[:B])
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[B] == 0x5A5A5A5A5A5A5A5A).all() and int(rank[B]) == GUARD and int(stage[B]) == GUARD
    return got[:B], rank.cpu().numpy()[:B], stage.cpu().numpy()[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("crc_name", list(CRCS))
@pytest.mark.parametrize("name", MASKS)
def test_crc_check(pkg, cuda, name, crc_name):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    K, (poly, c) = dec.K, CRCS[crc_name]
    if c >= K:
        with pytest.raises(pkg.PolarError) as e:
            dec.crc_check(cuda.zeros((131, dec.info_words), dtype=cuda.int64, device="cuda"), (poly, c))
        assert e.value.rc == -22
        return
    rng = np.random.default_rng(K + c)
    good = pkg.unpack_bits(pkg.crc_attach(pkg.pack_bits(rng.integers(0, 2, size=(65, K - c), dtype=np.uint8)), K, poly, c), K)
    good[0] = 0                                                 # the zero row passes
    bad = np.concatenate([good, good[1:2]])                     # 66 rows, one bit flipped in each
    bad[np.arange(66), rng.integers(0, K, size=66)] ^= 1
    bad[0] = 0
    bad[0, K - 1] = 1                                           # differs from the zero row in bit K - 1 only
    order = rng.permutation(131)
    bits, expect = np.concatenate([good, bad])[order], np.concatenate([np.ones(65, np.uint8), np.zeros(66, np.uint8)])[order]
    assert [int(pkg.crc_bits(r[:K - c], poly, c) == list(r[K - c:])) for r in bits] == list(expect)
    words = pkg.pack_bits(bits)
    if K % 64:
        words[::3, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(K % 64)    # bits past K are ignored
    out = cuda.full((132,), GUARD, dtype=cuda.uint8, device="cuda")
    dec.crc_check(cuda.from_numpy(words.view(np.int64)).cuda(), (poly, c), out=out[:131])
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:131], expect)
    assert got[131] == GUARD


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 8])
@pytest.mark.parametrize("name,crc_name", [(n, "crc8") for n in MASKS] + [("FB_N1024_K512", "crc24")])
def test_adaptive_parity(pkg, cuda, oracle_mod, name, crc_name, L):
    ref_info, ref_rank, ref_stage = reference(pkg, oracle_mod, name, crc_name, L)
    assert (ref_stage == 0).any() and (ref_stage == 1).any()
    assert ref_stage[-3] == 0 and ref_stage[-2] == 0 and ref_stage[-1] == 1     # the constructed frames
    dec = pkg.Decoder(_plansets.soft_mask(name))
    info, rank, stage = run_adaptive(pkg, cuda, dec, frames(pkg, name, crc_name), L, CRCS[crc_name])
    np.testing.assert_array_equal(stage, ref_stage)
    np.testing.assert_array_equal(info, pkg.pack_bits(ref_info))
    np.testing.assert_array_equal(rank, ref_rank)


@pytest.mark.gpu
def test_adaptive_all_and_none(pkg, cuda, oracle_mod):
    name, crc_name, L = "FB_N128_K64", "crc8", 4
    dec = pkg.Decoder(_plansets.soft_mask(name))
    for kind in ("pass", "fail"):
        ref_info, ref_rank, ref_stage = reference(pkg, oracle_mod, name, crc_name, L, kind)
        assert (ref_stage == (kind == "fail")).all()
        llr = frames(pkg, name, crc_name, kind)
        info, rank, stage = run_adaptive(pkg, cuda, dec, llr, L, CRCS[crc_name])
        np.testing.assert_array_equal(stage, ref_stage)
        np.testing.assert_array_equal(info, pkg.pack_bits(ref_info))
        np.testing.assert_array_equal(rank, ref_rank)
    x = cuda.from_numpy(np.array(llr)).cuda()                   # every frame failed: the list decoder's own result
    direct, direct_rank = dec.decode_list(x, L, crc=CRCS[crc_name])
    np.testing.assert_array_equal(info, direct.cpu().numpy().view(np.uint64))
    np.testing.assert_array_equal(rank, direct_rank.cpu().numpy())
    with pytest.raises(ValueError):
        dec.decode_adaptive(x, L, CRCS[crc_name], workspace=cuda.empty(dec.adaptive_workspace(65) - 16, dtype=cuda.uint8,
                                                                       device="cuda"))


@pytest.mark.gpu
def test_adaptive_in_a_graph(pkg, cuda, oracle_mod):
    """captured after one warm call: kernels only, the count zeroed by a kernel in every replay"""
    torch, name = cuda, "FB_N128_K64"
    dec = pkg.Decoder(_plansets.soft_mask(name))
    x = torch.from_numpy(np.array(frames(pkg, name, "crc8"))).cuda()
    eager = [t.cpu().numpy() for t in dec.decode_adaptive(x, 8, CRCS["crc8"])]
    np.testing.assert_array_equal(eager[2], reference(pkg, oracle_mod, name, "crc8", 8)[2])
    out = torch.zeros((x.shape[0], dec.info_words), dtype=torch.int64, device="cuda")
    rank, stage = (torch.zeros((x.shape[0],), dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.empty(dec.adaptive_workspace(x.shape[0]), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_adaptive(x, 8, CRCS["crc8"], out=out, rank=rank, stage=stage, workspace=ws, stream=s)
    for _ in range(3):
        for t in (out, rank, stage):
            t.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip((out, rank, stage), eager):
            np.testing.assert_array_equal(got.cpu().numpy(), want)
