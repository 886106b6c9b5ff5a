"""Adaptive decoding without a GPU: the argument rules of polar_sc_crc_check,
polar_sc_adaptive_workspace and polar_sc_decode_adaptive_to_info, judged before the device is
touched (NULL or made-up device pointers)."""
import ctypes

import util
from sc_polar_decoder_hls_amd import _plansets


def adaptive(pkg, dec, L, poly, length, batch=0, llr=None, ws=None, info=None):
    return pkg.lib().polar_sc_decode_adaptive_to_info(dec._plan, llr, batch, L, poly, length, ws, info, None, None, None)


def check(pkg, dec, poly, length, batch=0):
    return pkg.lib().polar_sc_crc_check(dec._plan, None, batch, poly, length, None, None)


def test_argument_validation(pkg):
    dec = pkg.Decoder(util.mask("FB_N128_K64"))
    assert adaptive(pkg, dec, 8, 0x07, 8) == 0 and adaptive(pkg, dec, 1, 0x864CFB, 24) == 0 and check(pkg, dec, 0x07, 8) == 0
    for L, poly, length in ((3, 0x07, 8), (16, 0x07, 8), (0, 0x07, 8), (8, 0, 0), (8, 0x07, 0), (8, 0x07, 33),
                            (8, 0x07, -1), (8, 0x1FF, 8)):
        assert adaptive(pkg, dec, L, poly, length) == -22, (L, poly, length)
    for poly, length in ((0, 0), (0x07, 33), (0x07, -1), (0x1FF, 8)):
        assert check(pkg, dec, poly, length) == -22, (poly, length)
    small = pkg.Decoder(_plansets.soft_mask("spc_n32"))          # K = 20: no room for a 24-bit CRC
    assert adaptive(pkg, small, 8, 0x864CFB, 24) == -22 and check(pkg, small, 0x864CFB, 24) == -22
    # frames without pointers; a missing and a misaligned workspace
    p = ctypes.c_void_p
    assert adaptive(pkg, dec, 8, 0x07, 8, batch=4) == -22 and check(pkg, dec, 0x07, 8, batch=4) == -22
    assert adaptive(pkg, dec, 8, 0x07, 8, batch=4, llr=p(256), info=p(256)) == -22
    assert adaptive(pkg, dec, 8, 0x07, 8, batch=4, llr=p(256), info=p(256), ws=p(264)) == -22
    size = ctypes.c_size_t(0)
    big = pkg.Decoder(util.mask("FB_N2048_K1024"))
    c9 = pkg.default_config()
    c9.llr_bits = 9
    for d in (big, pkg.Decoder(util.mask("FB_N1024_K512"), config=c9)):
        assert adaptive(pkg, d, 8, 0x07, 8) == -95 and check(pkg, d, 0x07, 8) == -95
        assert pkg.lib().polar_sc_adaptive_workspace(d._plan, 4, ctypes.byref(size)) == -95
    assert pkg.lib().polar_sc_decode_adaptive_to_info(None, None, 0, 8, 0x07, 8, None, None, None, None, None) == -22
    assert pkg.lib().polar_sc_crc_check(None, None, 0, 0x07, 8, None, None) == -22
    assert pkg.lib().polar_sc_adaptive_workspace(dec._plan, 4, None) == -22


def test_workspace_grows_with_the_batch(pkg):
    dec = pkg.Decoder(util.mask("FB_N128_K64"))
    # the index list rounded up to 16 bytes, the count in 16 bytes of its own, nothing for the SC stage
    assert [dec.adaptive_workspace(b) for b in (0, 1, 4, 5, 64, 65)] == [16, 32, 32, 48, 272, 288]
