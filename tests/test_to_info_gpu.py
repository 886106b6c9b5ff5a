"""Channel values straight to information words: decode_to_info against the
information words computed in numpy from this decoder's own decode / decode_soft of the same
input, and for the first frames from the oracle. The input is AWGN at 1.0 dB, so x^ is not a
codeword; the shapes are the smallest at which each part of the epilogue can go wrong (G = 2 and
one dword, half a row of lanes, one register, one and two register stages, K no multiple of 32
with pieces that straddle dwords)."""
import functools

import numpy as np
import pytest

import util
from sc_polar_decoder_hls_amd import _plansets
from test_soft_gpu import frames as soft_frames

SENTINEL = 0x5A5A5A5A5A5A5A5A


@functools.lru_cache(maxsize=None)
def llr_frames(name, batch):
    return util.synth_frames(_plansets.soft_mask(name), batch, ebn0_db=1.0, seed=batch)[0]


def info_words(pkg, dec, xhat):
    """u^ = x^ F^{(x)n} at the information positions, packed"""
    u = util.encode_np(pkg.unpack_bits(xhat, dec.N))
    return pkg.pack_bits(u[:, dec.mask.astype(bool)])


def check(pkg, torch, oracle_mod, dec, x, xhat, q, **kw):
    """decode_to_info(x) into rows followed by a guard row; xhat: this decoder's x^ of x, q: the int8 frames"""
    B = x.shape[0]
    buf = torch.full((B + 1, dec.info_words), SENTINEL, dtype=torch.int64, device="cuda")
    dec.decode_to_info(x, out=buf[:B], **kw)
    got = buf.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[:B], info_words(pkg, dec, xhat.cpu().numpy()))
    assert (got[B] == SENTINEL).all()
    ref = util.encode_np(oracle_mod.decode_fsm(dec.mask, q[:8]))[:, dec.mask.astype(bool)]
    np.testing.assert_array_equal(pkg.unpack_bits(got[:min(B, 8)], dec.K), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 19, 67])
@pytest.mark.parametrize("name", _plansets.INFO_INT8_MASKS)
def test_int8_to_info(pkg, cuda, oracle_mod, name, batch):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    assert dec.to_info_path(cuda.int8, batch)["fused"] == 1
    q = llr_frames(name, batch)
    x = cuda.from_numpy(q).cuda()
    check(pkg, cuda, oracle_mod, dec, x, dec.decode(x), q)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", _plansets.SOFT_DTYPES)
@pytest.mark.parametrize("name", _plansets.INFO_FLOAT_MASKS)
def test_float_to_info(pkg, cuda, oracle_mod, name, dtype):
    dec = pkg.Decoder(_plansets.soft_mask(name))
    assert dec.to_info_path(dtype, 19)["fused"] == 1
    t, q = soft_frames(name, dtype, 19)
    x = t.cuda()
    check(pkg, cuda, oracle_mod, dec, x, dec.decode_soft(x), q.astype(np.int8))


@pytest.mark.gpu
def test_workspace_path(pkg, cuda, oracle_mod):
    dec = pkg.Decoder(util.mask("frozen_n_2048_k_1024"))
    assert dec.to_info_path(cuda.int8, 19) == {"fused": 0, "regs": 0, "code_key": "%016x" % 0,
                                               "workspace_bytes": 19 * 32 * 8}
    assert dec.to_info_path("float16", 19)["workspace_bytes"] == 19 * 32 * 8 + 19 * 2048
    q = util.synth_frames(dec.mask, 19, ebn0_db=1.0, seed=19)[0]
    x = cuda.from_numpy(q).cuda()
    check(pkg, cuda, oracle_mod, dec, x, dec.decode(x), q)


@pytest.mark.gpu
def test_no_information_bit(pkg, cuda):
    dec = pkg.Decoder(np.zeros(128, np.uint8))
    assert dec.to_info_path(cuda.int8, 19)["fused"] == 0
    out = dec.decode_to_info(cuda.zeros((19, 128), dtype=cuda.int8, device="cuda"))
    assert tuple(out.shape) == (19, 0)


@pytest.mark.gpu
def test_to_info_in_a_graph(pkg, cuda):
    torch = cuda
    dec = pkg.Decoder(_plansets.soft_mask("FB_N128_K64"))
    x = torch.from_numpy(llr_frames("FB_N128_K64", 19)).cuda()
    eager = dec.decode_to_info(x).cpu().numpy()                 # (warm-up: loads the kernel)
    out = torch.zeros((19, dec.info_words), dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            dec.decode_to_info(x, out=out, stream=s)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), eager)
