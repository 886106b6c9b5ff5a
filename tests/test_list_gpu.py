"""List decoding on the GPU: decode_list against tests/list_ref.py on every bit of
the information words and on the rank, and a round trip through crc_attach and encode.

Frames per case (9 at N <= 128, 5 at N = 1024: a partial block / a wave count that is no multiple
of the block): AWGN at Eb/N0 = 1 dB so that paths diverge; an all-zero frame (every metric ties: the
rank / bit tie-break decides everything); a noise-free codeword at +-127 with -128 sprinkled in
(N = 1024: G reaches its clamp along the rightmost branch); and a frame whose rank 0 fails the CRC
while a later rank passes (FAIL_SEED, found by searching seeds with list_ref). A 24-bit CRC does
not fit the K = 20 of the N = 32 mask: that case checks the refusal instead."""
import functools

import numpy as np
import pytest

import list_ref
import util
from sc_polar_decoder_hls_amd import _plansets

MASKS = ("spc_n32", "FB_N128_K64", "FB_N1024_K512")
CRCS = {"none": None, "crc8": (0x07, 8), "crc24": (0x864CFB, 24)}
# AWGN seed of the frame whose CRC fails on rank 0 and passes on a later one, for L = 2, 4 and 8
FAIL_SEED = {("spc_n32", "crc8"): 1014, ("FB_N128_K64", "crc8"): 1001, ("FB_N128_K64", "crc24"): 1002,
             ("FB_N1024_K512", "crc8"): 1036, ("FB_N1024_K512", "crc24"): 1141}


def noisy(pkg, mask, crc, n, seed, ebn0_db=1.0):
    """n frames of a random payload (with its CRC when one is given) through AWGN; (llr, info words)"""
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
def case_frames(pkg, name, crc_name):
    mask, crc = _plansets.soft_mask(name), CRCS[crc_name]
    total = 5 if mask.size == 1024 else 9
    fits = crc is None or crc[1] < int(mask.sum())
    llr, _, x = noisy(pkg, mask, crc if fits else None, total, seed=mask.size + 7)
    llr[-3] = 0
    sprinkle = np.random.default_rng(3).random(mask.size) < 0.3
    llr[-2] = np.where(x[-2] == 1, np.where(sprinkle, -128, -127), 127)
    if fits:
        key = (name, crc_name if crc else "crc8")
        llr[-1] = noisy(pkg, mask, CRCS[key[1]], 1, FAIL_SEED[key])[0][0]
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def reference(pkg, name, crc_name, L):
    crc = CRCS[crc_name] or (0, 0)
    return list_ref.decode(_plansets.soft_mask(name), case_frames(pkg, name, crc_name), L, *crc)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 4, 8])
@pytest.mark.parametrize("crc_name", list(CRCS))
@pytest.mark.parametrize("name", MASKS)
def test_list_parity(pkg, cuda, name, crc_name, L):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    crc = CRCS[crc_name]
    x = cuda.from_numpy(np.array(case_frames(pkg, name, crc_name))).cuda()
    if crc is not None and crc[1] >= dec.K:
        with pytest.raises(pkg.PolarError) as e:
            dec.decode_list(x, L, crc=crc)
        assert e.value.rc == -22
        return
    ref_info, ref_rank = reference(pkg, name, crc_name, L)
    if crc is not None and L > 1:      # the constructed frame: rank 0 fails, a later rank passes
        assert 0 < ref_rank[-1] < L, "FAIL_SEED no longer gives the case"
    B = x.shape[0]
    buf = cuda.full((B + 1, dec.info_words), 0x5A5A5A5A5A5A5A5A, dtype=cuda.int64, device="cuda")
    rank = cuda.full((B + 1,), 0x5A, dtype=cuda.uint8, device="cuda")
    dec.decode_list(x, L, crc=crc, out=buf[:B], rank=rank[:B])
    got = buf.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[:B], pkg.pack_bits(ref_info))
    np.testing.assert_array_equal(rank.cpu().numpy()[:B], ref_rank)
    assert (got[B] == 0x5A5A5A5A5A5A5A5A).all() and int(rank[B]) == 0x5A      # nothing past the batch


@pytest.mark.gpu
@pytest.mark.parametrize("name", MASKS)
def test_round_trip(pkg, cuda, name):
    """crc_attach -> encode -> BPSK at +-31 -> decode_list: the payload, rank 0, at every L"""
    dec = pkg.Decoder(_plansets.soft_mask(name))
    crc = CRCS["crc8"]
    payload = np.random.default_rng(dec.N).integers(0, 2, size=(9, dec.K - 8), dtype=np.uint8)
    words = pkg.crc_attach(pkg.pack_bits(payload), dec.K, *crc)
    xw = dec.encode(cuda.from_numpy(words.view(np.int64)).cuda())
    llr = cuda.from_numpy(np.where(pkg.unpack_bits(xw.cpu().numpy(), dec.N) == 1, -31, 31).astype(np.int8)).cuda()
    for L in (1, 2, 4, 8):
        info, rank = dec.decode_list(llr, L, crc=crc)
        np.testing.assert_array_equal(info.cpu().numpy().view(np.uint64), words)
        np.testing.assert_array_equal(pkg.unpack_bits(info.cpu().numpy(), dec.K)[:, :dec.K - 8], payload)
        assert not rank.cpu().numpy().any()
