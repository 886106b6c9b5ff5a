"""Precoded (PAC) codes without a GPU ("Precoded codes"): the argument rules of
polar_sc_decode_list_precoded_to_info and polar_sc_encode_precoded, judged before the device is touched."""
import numpy as np

import util
from sc_polar_decoder_hls_amd import _plansets

PAC, FULL = (0x6D, 7), (0x80C20045, 32)
# length outside 1 .. 32, tap 0 clear, the top tap clear, taps at or above the length
BAD_CONV = ((0x6D, 0), (0x6D, 33), (0x6D, -1), (0x6C, 7), (0x2D, 7), (0x6D, 6), (0x16D, 7), (0, 1), (3, 1))


def decode(pkg, dec, L, conv, poly=0, length=0, batch=0):
    return pkg.lib().polar_sc_decode_list_precoded_to_info(dec and dec._plan, None, batch, L, *conv, poly, length, None, None,
                                                           None)


def encode(pkg, dec, conv, batch=0):
    return pkg.lib().polar_sc_encode_precoded(dec and dec._plan, None, None, batch, *conv, None)


def test_argument_validation(pkg):
    dec, big = pkg.Decoder(util.mask("FB_N128_K64")), pkg.Decoder(util.mask("FB_N2048_K1024"))
    for conv in (PAC, FULL, (1, 1)):
        assert encode(pkg, dec, conv) == 0
        for L in (1, 2, 4, 8, 16, 32):
            assert decode(pkg, dec, L, conv) == 0 and decode(pkg, dec, L, conv, 0x864CFB, 24) == 0, (L, conv)
    for conv in BAD_CONV:
        assert decode(pkg, dec, 8, conv) == decode(pkg, dec, 32, conv, 0x07, 8) == encode(pkg, dec, conv) == -22, conv
    for L, poly, length in ((0, 0x07, 8), (3, 0x07, 8), (64, 0x07, 8), (32, 0x07, 0), (32, 0x07, 33), (32, 0x07, -1),
                            (16, 0x1FF, 8), (8, 0x07, 64)):
        assert decode(pkg, dec, L, PAC, poly, length) == -22, (L, poly, length)
    assert decode(pkg, pkg.Decoder(_plansets.soft_mask("spc_n32")), 32, PAC, 0x864CFB, 24) == -22   # K = 20
    assert decode(pkg, dec, 32, PAC, 0x07, 8, batch=4) == encode(pkg, dec, PAC, batch=4) == -22      # frames without pointers
    c9 = pkg.default_config()
    c9.llr_bits = 9
    for d in (big, pkg.Decoder(util.mask("FB_N1024_K512"), config=c9)):
        assert decode(pkg, d, 8, PAC, 0x07, 8) == decode(pkg, d, 32, FULL) == -95
    assert encode(pkg, big, PAC) == -95
    assert decode(pkg, pkg.Decoder(np.zeros(64, np.uint8)), 32, PAC, batch=4) == 0   # K = 0: no launch
    assert decode(pkg, None, 32, PAC) == encode(pkg, None, PAC) == -22              # null plan
