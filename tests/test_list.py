"""List decoding without a GPU: the argument rules of
polar_sc_decode_list_to_info, and crc_attach against the bit-by-bit CRC of tests/list_ref.py."""
import numpy as np
import pytest

import list_ref
import util


def call(pkg, dec, L, poly, length, batch=0):
    return pkg.lib().polar_sc_decode_list_to_info(dec._plan, None, batch, L, poly, length, None, None, None)


def test_argument_validation(pkg):
    dec = pkg.Decoder(util.mask("FB_N128_K64"))
    assert call(pkg, dec, 8, 0, 0) == 0 and call(pkg, dec, 1, 0x07, 8) == 0 and call(pkg, dec, 4, 0x864CFB, 24) == 0
    for L, poly, length in ((3, 0, 0), (16, 0, 0), (0, 0, 0), (8, 0x07, 0), (8, 0x07, 33), (8, 0x07, -1),
                            (8, 0x07, 64), (8, 0x1FF, 8)):
        assert call(pkg, dec, L, poly, length) == -22, (L, poly, length)
    assert call(pkg, dec, 8, 0, 0, batch=4) == -22               # frames without pointers
    assert call(pkg, pkg.Decoder(util.mask("FB_N2048_K1024")), 8, 0x07, 8) == -95
    c9 = pkg.default_config()
    c9.llr_bits = 9
    assert call(pkg, pkg.Decoder(util.mask("FB_N1024_K512"), config=c9), 8, 0x07, 8) == -95
    assert call(pkg, pkg.Decoder(np.zeros(64, np.uint8)), 8, 0, 0, batch=4) == 0   # K = 0: no launch
    assert pkg.lib().polar_sc_decode_list_to_info(None, None, 0, 8, 0, 0, None, None, None) == -22


@pytest.mark.parametrize("K,poly,length", [(64, 0x07, 8), (512, 0x864CFB, 24), (20, 0x07, 8), (97, 0x04C11DB7, 32),
                                           (5, 0x1, 1)])
def test_crc_attach(pkg, K, poly, length):
    bits = np.random.default_rng(K).integers(0, 2, size=(3, K - length), dtype=np.uint8)
    junk = np.concatenate([bits, np.ones((3, (-(K - length)) % 64), np.uint8)], axis=1)   # bits past the message
    words = pkg.crc_attach(pkg.pack_bits(junk), K, poly, length)
    assert words.shape == (3, (K + 63) // 64) and words.dtype == np.uint64
    got = pkg.unpack_bits(words, 64 * words.shape[1])
    assert not got[:, K:].any()
    for row, msg in zip(got, bits):
        assert list(row[:K - length]) == list(msg)
        assert list(row[K - length:K]) == list_ref.crc(msg, poly, length)
    with pytest.raises(ValueError):
        pkg.crc_attach(words, K, poly, K)
