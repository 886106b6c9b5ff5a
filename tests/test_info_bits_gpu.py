"""Information bits on the device (polar_sc_xform.hip): extract_info, encode and
decode_info against numpy (util.encode_np, boolean indexing by the mask, pack_bits), compared
as whole u64 words so that the padding bits count. One case per kernel tier or tier boundary."""
import numpy as np
import pytest

import util


def _mask(name):
    """a fixture mask by name, or 'r<N>_<K>' (random), 'all<N>', 'last<N>' (one bit, at N - 1), 'none<N>'"""
    if name[0] == "r":
        N, K = (int(v) for v in name[1:].split("_"))
        m = np.zeros(N, np.uint8)
        m[np.random.default_rng(N).permutation(N)[:K]] = 1
        return m
    for kind, lo, hi in (("all", 0, None), ("last", -1, None), ("none", 0, 0)):
        if name.startswith(kind):
            m = np.zeros(int(name[len(kind):]), np.uint8)
            m[lo:hi] = 1
            return m
    return util.mask(name)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


CASES = [("r32_13", 1), ("r32_13", 67), ("all64", 5), ("FB_N128_K64", 67), ("FB_N1024_K512", 1), ("FB_N1024_K512", 67),
         ("last1024", 3), ("frozen_n_2048_k_1844", 3), ("frozen_n_4096_k_3686", 3), ("frozen_n_65536_k_32768", 2),
         ("r131072_43691", 2), ("r1048576_524287", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,batch", CASES)
def test_extract_encode_against_numpy(pkg, cuda, name, batch):
    torch = cuda
    mask = _mask(name)
    sel = mask.astype(bool)
    dec = pkg.Decoder(mask)
    N, K = dec.N, dec.K
    rng = np.random.default_rng(N + batch)
    # extraction of random codeword rows into a pre-filled buffer
    xbits = rng.integers(0, 2, size=(batch, N), dtype=np.uint8)
    xw = pkg.pack_bits(xbits)
    if N == 32:
        xw |= np.uint64(0xDEADBEEF) << np.uint64(32)      # the unused half of the row is ignored
    out = torch.full((batch, dec.info_words), -1, dtype=torch.int64, device="cuda")
    got = dec.extract_info(torch.from_numpy(xw.view(np.int64)).cuda(), out=out)
    assert got is out
    np.testing.assert_array_equal(_u64(got), pkg.pack_bits(util.encode_np(xbits)[:, sel]))
    # encoding of random information words, garbage above bit K included
    iw = rng.integers(0, 1 << 64, size=(batch, dec.info_words), dtype=np.uint64)
    ibits = pkg.unpack_bits(iw, K)
    u = np.zeros((batch, N), np.uint8)
    u[:, sel] = ibits
    cw = dec.encode(torch.from_numpy(iw.view(np.int64)).cuda(),
                    out=torch.full((batch, dec.words), -1, dtype=torch.int64, device="cuda"))
    np.testing.assert_array_equal(_u64(cw), pkg.pack_bits(util.encode_np(u)))
    np.testing.assert_array_equal(_u64(dec.extract_info(cw)), pkg.pack_bits(ibits))


@pytest.mark.gpu
def test_decode_info_is_decode_then_extract(pkg, cuda):
    torch = cuda
    mask = util.mask("FB_N1024_K512")
    dec = pkg.Decoder(mask)
    llr = torch.from_numpy(util.synth_frames(mask, 67, ebn0_db=2.5)[0]).cuda()
    ref = dec.decode(llr)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    xhat = torch.full((67, dec.words), -1, dtype=torch.int64, device="cuda")
    with torch.cuda.stream(s):
        info = dec.decode_info(llr, xhat=xhat, stream=s)
    s.synchronize()
    np.testing.assert_array_equal(_u64(xhat), _u64(ref))
    np.testing.assert_array_equal(_u64(info), pkg.pack_bits(dec.codeword_to_info(_u64(ref))))


@pytest.mark.gpu
def test_no_information_bits(pkg, cuda):
    dec = pkg.Decoder(_mask("none64"))
    x = cuda.ones((3, 1), dtype=cuda.int64, device="cuda")
    assert tuple(dec.extract_info(x).shape) == (3, 0)
    assert not dec.encode(cuda.empty((3, 0), dtype=cuda.int64, device="cuda")).any()
