"""Soft-output (SCAN) decoding without a GPU: the argument rules of polar_sc_decode_scan,
judged before the device is touched, the kernel's LDS accounting, and the entry's declaration."""
import ctypes
import os

import pytest

import util

PTR = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before any launch


def scan(pkg, dec, llr, batch, iterations, ext, hard=None):
    return pkg.lib().polar_sc_decode_scan(dec._plan if dec else None, llr, batch, iterations, ext, hard, None)


def test_argument_validation(pkg):
    dec = pkg.Decoder(util.mask("FB_N128_K64"))
    for it in range(1, 9):
        assert scan(pkg, dec, None, 0, it, None) == 0                      # an empty batch needs no pointers
    for it in (0, 9, -1):
        assert scan(pkg, dec, PTR, 0, it, PTR) == -22
    assert scan(pkg, None, PTR, 0, 1, PTR) == -22
    for llr, ext, hard in ((None, PTR, None), (PTR, None, None), (ctypes.c_void_p(0x1002), PTR, None),
                           (PTR, ctypes.c_void_p(0x1002), None), (PTR, PTR, ctypes.c_void_p(0x1004))):
        assert scan(pkg, dec, llr, 3, 1, ext, hard) == -22
    assert scan(pkg, dec, PTR, (1 << 31) - 7, 1, PTR) == -22
    c9 = pkg.default_config()
    c9.llr_bits = 9
    for d in (pkg.Decoder(util.mask("FB_N2048_K1024")), pkg.Decoder(util.mask("FB_N1024_K512"), config=c9)):
        assert scan(pkg, d, None, 0, 1, None) == -95


@pytest.mark.parametrize("iterations", [1, 2, 8])
def test_shape(pkg, iterations):
    """channel + beta (N int16 each) + the alpha levels 6 .. log2 N - 1; more than one iteration keeps
    N/2 beta_R per level; four waves per block, inside a block's 64 KB and a CU's 160 KB"""
    for logn in range(5, 11):
        N = 1 << logn
        lds = 4 * N + 2 * (N - min(N, 64)) + (logn * N if iterations > 1 else 0)
        assert pkg.scan_shape(N, iterations) == (lds, 4) and 4 * lds <= 65536
    for N, it in ((16, 1), (2048, 1), (96, 1), (0, 1), (128, 0), (128, 9)):
        assert pkg.scan_shape(N, it) == (0, 0)


def test_declared_and_exported(pkg):
    with open(os.path.join(util.ROOT, "include", "polar_sc.h")) as f:
        header = f.read()
    assert "polar_sc_decode_scan" in pkg.EXPORTS and "int polar_sc_decode_scan(" in header
    assert "void polar_sc_scan_shape(" in header and hasattr(pkg.lib(), "polar_sc_scan_shape")
