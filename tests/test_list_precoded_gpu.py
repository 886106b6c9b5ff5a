"""List decoding of convolutionally precoded (PAC) codes on the GPU ("Precoded codes"):
decode_list(precode=...) against tests/list_precoded_ref.py on every bit of the information words and
on the rank, encode(precode=...) against the numpy convolution and transform. Frames per case as in
tests/test_list_wide_gpu.py (9 at N <= 128, 5 at N = 1024: a partial block): AWGN at 1 dB on precoded
codewords that carry a CRC-8; an all-zero frame (every metric ties, and a frozen position that decides
u = 1 must add nothing); +-127 on a precoded codeword with -128 sprinkled in."""
import functools

import numpy as np
import pytest

import list_precoded_ref as ref
import util
from sc_polar_decoder_hls_amd import _plansets

CONVS = {"pac": (0x6D, 7), "full": (0x80C20045, 32)}
CRCS = {"none": None, "crc8": (0x07, 8)}
CASES = [(n, L) for n in ("spc_n32", "FB_N128_K64") for L in (2, 8, 16, 32)] + [("FB_N1024_K512", 8), ("FB_N1024_K512", 32)]
GUARD = 0x5A5A5A5A5A5A5A5A


def sent(pkg, mask, conv, n, seed):
    """n random payloads with a CRC-8: (information words with junk above bit K, precoded codewords)"""
    K = int(mask.sum())
    bits = np.random.default_rng(seed).integers(0, 2, size=(n, K - 8), dtype=np.uint8)
    words = pkg.crc_attach(pkg.pack_bits(bits), K, *CRCS["crc8"])
    v = np.zeros((n, mask.size), dtype=np.uint8)
    v[:, mask.astype(bool)] = pkg.unpack_bits(words, K)
    words[:, -1] |= np.uint64(0xABC << (K % 64) if K % 64 else 0)
    return words, util.encode_np(ref.precode_np(v, *conv))


@functools.lru_cache(maxsize=None)
def frames(pkg, name, conv_name):
    mask, rng = _plansets.soft_mask(name), np.random.default_rng(11)
    x = sent(pkg, mask, CONVS[conv_name], 5 if mask.size == 1024 else 9, seed=mask.size + 7)[1]
    sigma = 1.0 / np.sqrt(2.0 * mask.sum() / mask.size * 10.0 ** 0.1)
    llr = np.clip(np.trunc(4.0 * (np.where(x == 1, -1.0, 1.0) + sigma * rng.standard_normal(x.shape))), -31, 31).astype(np.int8)
    llr[-2] = 0
    llr[-1] = np.where(x[-1] == 1, np.where(rng.random(mask.size) < 0.3, -128, -127), 127)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def ref_paths(pkg, name, conv_name, L):
    """the reference walk, shared by the CRC cases (the CRC only chooses among its paths)"""
    return ref.paths(_plansets.soft_mask(name), frames(pkg, name, conv_name), L, *CONVS[conv_name])


def run(cuda, dec, llr, L, crc, precode):
    """decode_list into buffers with a guard row: (information words, ranks) of the batch"""
    B = llr.shape[0]
    buf = cuda.full((B + 1, dec.info_words), GUARD, dtype=cuda.int64, device="cuda")
    rank = cuda.full((B + 1,), GUARD & 0xFF, dtype=cuda.uint8, device="cuda")
    dec.decode_list(cuda.from_numpy(np.array(llr)).cuda(), L, crc=crc, out=buf[:B], rank=rank[:B], precode=precode)
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[B] == GUARD).all() and int(rank[B]) == GUARD & 0xFF             # nothing past the batch
    return got[:B], rank.cpu().numpy()[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("crc_name", list(CRCS))
@pytest.mark.parametrize("conv_name", list(CONVS))
@pytest.mark.parametrize("name,L", CASES)
def test_parity(pkg, cuda, name, L, conv_name, crc_name):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    ref_info, ref_rank = ref.choose(ref_paths(pkg, name, conv_name, L), *(CRCS[crc_name] or (0, 0)))
    info, rank = run(cuda, dec, frames(pkg, name, conv_name), L, CRCS[crc_name], CONVS[conv_name])
    np.testing.assert_array_equal(info, pkg.pack_bits(ref_info))
    np.testing.assert_array_equal(rank, ref_rank)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [8, 32])
def test_identity_precoder(pkg, cuda, L):
    """(1, 1) is decode_list without the keyword, row for row and rank for rank, on the AWGN frames"""
    dec, llr = pkg.Decoder(_plansets.soft_mask("FB_N128_K64")), frames(pkg, "FB_N128_K64", "pac")[:-2]
    for got, want in zip(run(cuda, dec, llr, L, CRCS["crc8"], (1, 1)), run(cuda, dec, llr, L, CRCS["crc8"], None)):
        np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("conv_name", list(CONVS))
@pytest.mark.parametrize("name", ["spc_n32", "FB_N128_K64", "FB_N1024_K512"])
def test_encode_and_round_trip(pkg, cuda, name, conv_name):
    """encode(precode=...) of 70 rows; then five of those codewords, noiseless, back through decode_list"""
    dec, conv = pkg.Decoder(_plansets.soft_mask(name)), CONVS[conv_name]
    words, x = sent(pkg, _plansets.soft_mask(name), conv, 70, seed=3)
    got = dec.encode(cuda.from_numpy(words.view(np.int64)).cuda(), precode=conv).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, pkg.pack_bits(x))
    info, rank = run(cuda, dec, np.where(x[:5] == 1, -31, 31).astype(np.int8), 4, CRCS["crc8"], conv)
    np.testing.assert_array_equal(pkg.unpack_bits(info, dec.K), pkg.unpack_bits(words[:5], dec.K))
    assert (rank == 0).all()


@pytest.mark.gpu
def test_graph_replay(pkg, cuda):
    """the precoded decode captured into a graph: three replays against the eager result"""
    dec, args = pkg.Decoder(_plansets.soft_mask("FB_N128_K64")), dict(crc=CRCS["crc8"], precode=CONVS["pac"])
    x = cuda.from_numpy(np.array(frames(pkg, "FB_N128_K64", "pac"))).cuda()
    eager = [t.clone() for t in dec.decode_list(x, 32, **args)]
    out, rank = (cuda.empty_like(t) for t in eager)
    s, g = cuda.cuda.Stream(), cuda.cuda.CUDAGraph()
    s.wait_stream(cuda.cuda.current_stream())
    with cuda.cuda.stream(s), cuda.cuda.graph(g, stream=s):
        dec.decode_list(x, 32, out=out, rank=rank, stream=s, **args)
    for _ in range(3):
        out.fill_(0x33)
        rank.fill_(0x33)
        g.replay()
        cuda.cuda.synchronize()
        assert cuda.equal(out, eager[0]) and cuda.equal(rank, eager[1])
