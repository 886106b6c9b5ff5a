"""Wide-list decoding without a GPU: the argument rules of
polar_sc_decode_list_wide_to_info and polar_sc_decode_adaptive_wide_to_info, judged before the device
is touched, and the LDS accounting of the wide-list kernel."""
import numpy as np
import pytest

import util
from sc_polar_decoder_hls_amd import _plansets


def wide_list(pkg, dec, L, poly, length, batch=0):
    return pkg.lib().polar_sc_decode_list_wide_to_info(dec._plan, None, batch, L, poly, length, None, None, None)


def wide_adaptive(pkg, dec, L, poly, length, batch=0):
    return pkg.lib().polar_sc_decode_adaptive_wide_to_info(dec._plan, None, batch, L, poly, length, None, None, None,
                                                           None, None)


@pytest.mark.parametrize("call", [wide_list, wide_adaptive])
def test_argument_validation(pkg, call):
    dec = pkg.Decoder(util.mask("FB_N128_K64"))
    for L in (1, 2, 4, 8, 16, 32):
        assert call(pkg, dec, L, 0x07, 8) == 0 and call(pkg, dec, L, 0x864CFB, 24) == 0, L
    for L, poly, length in ((0, 0x07, 8), (3, 0x07, 8), (64, 0x07, 8), (-16, 0x07, 8), (32, 0x07, 0), (32, 0x07, 33),
                            (32, 0x07, -1), (16, 0x1FF, 8), (32, 0x07, 64)):
        assert call(pkg, dec, L, poly, length) == -22, (L, poly, length)
    assert call(pkg, dec, 32, 0, 0) == (0 if call is wide_list else -22)        # the CRC is optional for the list only
    assert call(pkg, pkg.Decoder(_plansets.soft_mask("spc_n32")), 32, 0x864CFB, 24) == -22   # K = 20
    assert call(pkg, dec, 32, 0x07, 8, batch=4) == -22                          # frames without pointers
    c9 = pkg.default_config()
    c9.llr_bits = 9
    for d in (pkg.Decoder(util.mask("FB_N2048_K1024")), pkg.Decoder(util.mask("FB_N1024_K512"), config=c9)):
        assert call(pkg, d, 16, 0x07, 8) == -95 and call(pkg, d, 32, 0x07, 8) == -95
    assert wide_list(pkg, pkg.Decoder(np.zeros(64, np.uint8)), 32, 0, 0, batch=4) == 0   # K = 0: no launch


def test_null_plan(pkg):
    assert pkg.lib().polar_sc_decode_list_wide_to_info(None, None, 0, 32, 0, 0, None, None, None) == -22
    assert pkg.lib().polar_sc_decode_adaptive_wide_to_info(None, None, 0, 32, 0x07, 8, None, None, None, None, None) == -22


@pytest.mark.parametrize("N,L,waves", [(1024, 32, 1), (1024, 16, 2), (512, 32, 2), (128, 32, 4), (32, 16, 4)])
def test_shape(pkg, N, L, waves):
    """R (N int16) + L arrays of N bytes (levels 1 .. log2 N - 2) + L partial-sum arrays + two copies of
    six dwords per rank; 4 waves per block where they fit 64 KB, else as many as fit"""
    psum = 4 * (4 + N // 32 + N // 32)         # levels 0 .. 4 and their pad, levels 5 .. log2 N - 1, level log2 N
    lds = 2 * N + L * N + L * psum + 2 * 6 * 4 * L
    assert pkg.list_shape(N, L) == (lds, waves) and waves == min(4, 65536 // lds) and lds * waves <= 65536
    if N == 1024:
        assert lds == {32: 45056, 16: 23552}[L]
