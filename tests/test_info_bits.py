"""Information bits on the host (include/polar_sc.h): polar_info_to_codeword is the encoder
x = u F^(x)n, polar_codeword_to_info inverts it; the device entry points validate their plan."""
import numpy as np
import pytest

import util


def _masks():
    m32 = np.zeros(32, np.uint8)
    m32[np.random.default_rng(32).permutation(32)[:13]] = 1
    return {"FB_N128_K64": util.mask("FB_N128_K64"), "random_n32_k13": m32}


@pytest.mark.parametrize("name", ["FB_N128_K64", "random_n32_k13"])
def test_info_to_codeword_is_the_encoder_and_inverts(pkg, name):
    mask = _masks()[name]
    dec = pkg.Decoder(mask)
    info = np.random.default_rng(5).integers(0, 2, size=(7, dec.K), dtype=np.uint8)
    u = np.zeros((7, mask.size), np.uint8)
    u[:, mask.astype(bool)] = info
    x = dec.info_to_codeword(info)
    assert x.dtype == np.uint64 and dec.info_words == (dec.K + 63) // 64
    np.testing.assert_array_equal(x, pkg.pack_bits(util.encode_np(u)))
    np.testing.assert_array_equal(dec.codeword_to_info(x), info)


def test_device_entry_points_reject_null_plan(pkg):
    lib = pkg.lib()
    assert lib.polar_sc_extract_info(None, None, None, 1, None) == -22
    assert lib.polar_sc_encode(None, None, None, 1, None) == -22
    assert lib.polar_sc_decode_info(None, None, None, None, 1, None) == -22
    assert lib.polar_info_to_codeword(None, None, None, 1) == -22
