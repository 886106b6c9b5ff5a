"""List decoding with 16 and 32 paths on the GPU (the wide-list kernel): decode_list
and decode_adaptive against tests/list_ref.py on every bit of the information words and on the rank.

Frames per case as in tests/test_list_gpu.py (9 at N <= 128, 5 at N = 1024: a partial block, a wave
count that is no multiple of the block): AWGN at 1 dB; an all-zero frame (every metric ties: the
(rank, bit) tie-break fills all the ranks); +-127 with -128 sprinkled in (G clamps, the metric is
near its bound: the top bits of the key); and last a frame whose CRC-8 passes first on a rank in the
upper half of the list (UPPER_SEED, found by searching seeds with list_ref), which no list of 8 returns."""
import functools

import numpy as np
import pytest

import list_ref
import util
from sc_polar_decoder_hls_amd import _plansets

MASKS = ("spc_n32", "FB_N128_K64", "FB_N1024_K512")
CRCS = {"none": None, "crc8": (0x07, 8), "crc24": (0x864CFB, 24)}
UPPER_SEED = {("spc_n32", 16): 2066, ("spc_n32", 32): 2123, ("FB_N128_K64", 16): 2066, ("FB_N128_K64", 32): 2066,
              ("FB_N1024_K512", 16): 2031, ("FB_N1024_K512", 32): 2012}
CASES = [(n, c, L) for n in MASKS for c in ("none", "crc8") for L in (16, 32)] + [("FB_N128_K64", "crc24", 32)]
GUARD = 0x5A


def noisy(pkg, mask, crc, n, seed, ebn0_db=1.0):
    """n frames of a random payload (with its CRC when one is given) through AWGN; (llr, info words, codewords)"""
    rng = np.random.default_rng(seed)
    K = int(mask.sum())
    bits = rng.integers(0, 2, size=(n, K), dtype=np.uint8)
    words = pkg.pack_bits(bits) if crc is None else pkg.crc_attach(pkg.pack_bits(bits[:, :K - crc[1]]), K, *crc)
    u = np.zeros((n, mask.size), dtype=np.uint8)
    u[:, mask.astype(bool)] = pkg.unpack_bits(words, K)
    x = util.encode_np(u)
    sigma = 1.0 / np.sqrt(2.0 * K / mask.size * 10.0 ** (ebn0_db / 10.0))
    y = np.where(x == 1, -1.0, 1.0) + sigma * rng.standard_normal(x.shape)
    return np.clip(np.trunc(4.0 * y), -31, 31).astype(np.int8), words, x


@functools.lru_cache(maxsize=None)
def case(pkg, name, crc_name, L):
    """(frames, reference information bits, reference ranks) of a parity case"""
    mask, crc = _plansets.soft_mask(name), CRCS[crc_name]
    llr, _, x = noisy(pkg, mask, crc, 5 if mask.size == 1024 else 9, seed=mask.size + 7)
    llr[-3] = 0
    sprinkle = np.random.default_rng(3).random(mask.size) < 0.3
    llr[-2] = np.where(x[-2] == 1, np.where(sprinkle, -128, -127), 127)
    llr[-1] = noisy(pkg, mask, CRCS["crc8"], 1, UPPER_SEED[name, L])[0][0]
    llr.setflags(write=False)
    return (llr,) + list_ref.decode(mask, llr, L, *(crc or (0, 0)))


@pytest.mark.gpu
@pytest.mark.parametrize("name,crc_name,L", CASES)
def test_wide_parity(pkg, cuda, name, crc_name, L):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    llr, ref_info, ref_rank = case(pkg, name, crc_name, L)
    if crc_name == "crc8":
        assert L // 2 <= ref_rank[-1] < L, "UPPER_SEED no longer gives the case"
    B = llr.shape[0]
    buf = cuda.full((B + 1, dec.info_words), 0x5A5A5A5A5A5A5A5A, dtype=cuda.int64, device="cuda")
    rank = cuda.full((B + 1,), GUARD, dtype=cuda.uint8, device="cuda")
    dec.decode_list(cuda.from_numpy(np.array(llr)).cuda(), L, crc=CRCS[crc_name], out=buf[:B], rank=rank[:B])
    got = buf.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[:B], pkg.pack_bits(ref_info))
    np.testing.assert_array_equal(rank.cpu().numpy()[:B], ref_rank)
    assert (got[B] == 0x5A5A5A5A5A5A5A5A).all() and int(rank[B]) == GUARD      # nothing past the batch


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["FB_N128_K64", "spc_n32"])
def test_wide_adaptive(pkg, cuda, name):
    """70 frames at 2 dB (more than one 64-frame wave of the check kernel), L = 32, CRC-8: the list
    decoder's rows exactly where decode_to_info's row fails the CRC; and one captured-graph replay"""
    torch, L, crc = cuda, 32, CRCS["crc8"]
    mask = _plansets.soft_mask(name)
    dec = pkg.Decoder(mask)
    llr = noisy(pkg, mask, crc, 70, seed=mask.size + 11, ebn0_db=2.0)[0]
    x = torch.from_numpy(llr).cuda()
    B = x.shape[0]
    sc = dec.decode_to_info(x).cpu().numpy().view(np.uint64)
    bits = pkg.unpack_bits(sc, dec.K)
    ref_stage = np.array([list_ref.crc(r[:dec.K - 8], *crc) != list(r[dec.K - 8:]) for r in bits], dtype=np.uint8)
    assert (ref_stage == 0).any() and (ref_stage == 1).any()
    bad = np.flatnonzero(ref_stage)
    ref_info, ref_rank = sc.copy(), np.zeros(B, dtype=np.uint8)
    info_bad, ref_rank[bad] = list_ref.decode(mask, llr[bad], L, *crc)
    ref_info[bad] = pkg.pack_bits(info_bad)

    buf = torch.full((B + 1, dec.info_words), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    rank, stage = (torch.full((B + 1,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.empty(dec.adaptive_workspace(B), dtype=torch.uint8, device="cuda")
    dec.decode_adaptive(x, L, crc, out=buf[:B], rank=rank[:B], stage=stage[:B], workspace=ws)
    eager = [t.cpu().numpy() for t in (buf, rank, stage)]
    np.testing.assert_array_equal(eager[2][:B], ref_stage)
    np.testing.assert_array_equal(eager[0][:B].view(np.uint64), ref_info)
    np.testing.assert_array_equal(eager[1][:B], ref_rank)
    assert (eager[0][B].view(np.uint64) == 0x5A5A5A5A5A5A5A5A).all() and eager[1][B] == GUARD and eager[2][B] == GUARD

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_adaptive(x, L, crc, out=buf[:B], rank=rank[:B], stage=stage[:B], workspace=ws, stream=s)
    for t in (buf[:B], rank[:B], stage[:B]):
        t.fill_(0x33)
    g.replay()
    torch.cuda.synchronize()
    for got, want in zip((buf, rank, stage), eager):
        np.testing.assert_array_equal(got.cpu().numpy(), want)
