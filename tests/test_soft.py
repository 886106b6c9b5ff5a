"""Float channel values, host side: the argument rules of polar_sc_quantize /
polar_sc_decode_soft and what polar_sc_soft_info_get reports for each kind of plan. No GPU: the
arguments are judged, and the fused kernels compiled, before the device is touched."""
import ctypes

import pytest

from sc_polar_decoder_hls_amd import _plansets

EINVAL = -22
PTR = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before any launch


def _decoder(pkg, name, llr_bits=6, tuning=None):
    cfg = pkg.default_config()
    cfg.llr_bits = llr_bits
    return pkg.Decoder(_plansets.soft_mask(name), cfg, tuning=tuning)


# (dtype, beta, vsatn, vsatp) that the int8 channel refuses
BAD = [(3, 4, -31, 31), (-1, 4, -31, 31), (0, 0, -31, 31), (0, 256, -31, 31), (0, 4, 5, 4), (0, 4, -129, 31),
       (0, 4, -31, 128)]


@pytest.mark.parametrize("dtype,beta,lo,hi", BAD)
def test_arguments_refused(pkg, dtype, beta, lo, hi):
    L = pkg.lib()
    assert L.polar_sc_quantize(PTR, dtype, 16, beta, lo, hi, PTR, 8, None) == EINVAL
    dec = _decoder(pkg, "FB_N128_K64", tuning={"kernel": 1})
    assert L.polar_sc_decode_soft(dec._plan, PTR, dtype, beta, lo, hi, PTR, PTR, 1, None) == EINVAL


def test_bounds_follow_the_channel_type(pkg):
    L = pkg.lib()
    assert L.polar_sc_quantize(PTR, 0, 16, 4, -31, 31, PTR, 12, None) == EINVAL          # bits
    assert L.polar_sc_quantize(PTR, 0, 16, 4, -32769, 255, PTR, 16, None) == EINVAL
    assert L.polar_sc_quantize(PTR, 0, 0, 64, -255, 255, PTR, 16, None) == 0            # n == 0
    d8, d9 = _decoder(pkg, "FB_N128_K64", 8, {"kernel": 1}), _decoder(pkg, "frozen_n_2048_k_1024", 9)
    assert L.polar_sc_decode_soft(d8._plan, PTR, 0, 16, -255, 255, PTR, PTR, 1, None) == EINVAL   # int8 channel
    assert L.polar_sc_decode_soft(d9._plan, PTR, 0, 32, -255, 255, PTR, PTR, 0, None) == 0        # int16; batch == 0
    # a plan that needs the workspace: NULL or not 16-byte aligned
    for ws in (None, ctypes.c_void_p(0x1008)):
        assert L.polar_sc_decode_soft(d8._plan, PTR, 0, 16, -127, 127, ws, PTR, 1, None) == EINVAL


@pytest.mark.parametrize("dtype", _plansets.SOFT_DTYPES)
@pytest.mark.parametrize("name", ["spc_n32", "FB_N128_K64", "FB_N1024_K512"])
def test_per_mask_plans_fuse(pkg, name, dtype):
    info = _decoder(pkg, name).soft_info(dtype, 67)
    assert info["fused"] == 1 and info["workspace_bytes"] == 0
    assert 0 < info["regs"] <= 128
    assert int(info["code_key"], 16) != 0


@pytest.mark.parametrize("name,llr_bits,tuning,per_value", [
    ("FB_N128_K64", 6, {"kernel": 1}, 1), ("frozen_n_2048_k_1024", 6, None, 1), ("frozen_n_2048_k_1024", 9, None, 2)])
def test_other_plans_take_two_launches(pkg, name, llr_bits, tuning, per_value):
    dec = _decoder(pkg, name, llr_bits, tuning)
    info = dec.soft_info("float16", 5)
    assert info == {"fused": 0, "regs": 0, "workspace_bytes": 5 * dec.N * per_value, "code_key": "%016x" % 0}
