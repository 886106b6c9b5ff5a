"""Channel values straight to information words, host side: the new entry points
are declared and refuse bad arguments before the device is touched, the x^ kernels' sources are
what they were, and the one-launch kernel of the headline shape compiles within the x^ kernel's
registers. No GPU."""
import ctypes
import hashlib
import os
import sys

import pytest

import util

EINVAL = -22
PTR = ctypes.c_void_p(0x1000)      # never dereferenced: every call below returns before any launch
# sha256 of Decoder(FB_N1024_K512).kernel_source() at the commit before the information-bit epilogue
C2_SOURCE_SHA256 = "ffb1406716f08119117b8fb91ff5acf4f534eca0b2dfebdc7d2d42c14b4fdbc3"
NEW = ("polar_sc_to_info_get", "polar_sc_decode_to_info", "polar_sc_decode_soft_to_info")


def test_symbols_declared_and_exported(pkg):
    with open(os.path.join(util.ROOT, "include", "polar_sc.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in pkg.EXPORTS and "int %s(" % name in header and hasattr(pkg.lib(), name)
    assert "POLAR_SC_I8 = 3" in header and pkg.POLAR_SC_I8 == 3
    assert pkg.lib().polar_sc_abi_version() == 5


@pytest.mark.parametrize("args", [
    lambda p: ("polar_sc_decode_to_info", (p, None, None, PTR, 1, None)),
    lambda p: ("polar_sc_decode_to_info", (p, PTR, None, None, 1, None)),
    lambda p: ("polar_sc_decode_to_info", (None, PTR, None, PTR, 1, None)),
    lambda p: ("polar_sc_decode_to_info", (p, PTR, None, PTR, (1 << 31) - 7, None)),
    lambda p: ("polar_sc_decode_soft_to_info", (p, None, 0, 4, -31, 31, None, PTR, 1, None)),
    lambda p: ("polar_sc_decode_soft_to_info", (p, PTR, 0, 4, -31, 31, None, None, 1, None)),
    lambda p: ("polar_sc_decode_soft_to_info", (p, PTR, 3, 4, -31, 31, None, PTR, 1, None)),     # int8 is not a float type
    lambda p: ("polar_sc_decode_soft_to_info", (p, PTR, 0, 0, -31, 31, None, PTR, 1, None)),     # beta
    lambda p: ("polar_sc_decode_soft_to_info", (p, ctypes.c_void_p(0x1002), 0, 4, -31, 31, None, PTR, 1, None)),
    lambda p: ("polar_sc_to_info_get", (p, 4, 1, PTR)),
    lambda p: ("polar_sc_to_info_get", (p, -1, 1, PTR)),
    lambda p: ("polar_sc_to_info_get", (p, 3, 1, None)),
])
def test_arguments_refused(pkg, args):
    dec = pkg.Decoder(util.mask("FB_N128_K64"))
    fn, a = args(dec._plan)
    assert getattr(pkg.lib(), fn)(*a) == EINVAL


def test_empty_batch_and_workspace_rules(pkg):
    L = pkg.lib()
    dec = pkg.Decoder(util.mask("FB_N128_K64"), tuning={"kernel": 1})      # the interpreter: the workspace path
    assert L.polar_sc_decode_to_info(dec._plan, None, None, None, 0, None) == 0
    assert dec.to_info_path("int8", 5) == {"fused": 0, "regs": 0, "workspace_bytes": 5 * 2 * 8, "code_key": "%016x" % 0}
    assert dec.to_info_path("bfloat16", 5)["workspace_bytes"] == 5 * 2 * 8 + 5 * 128
    for ws in (None, ctypes.c_void_p(0x1008)):
        assert L.polar_sc_decode_to_info(dec._plan, PTR, ws, PTR, 1, None) == EINVAL


def test_xhat_kernel_source_unchanged(pkg):
    src = pkg.Decoder(util.mask("FB_N1024_K512")).kernel_source()
    assert hashlib.sha256(src.encode()).hexdigest() == C2_SOURCE_SHA256


def test_c2_info_kernel_budget(pkg):
    sys.path.insert(0, os.path.join(util.ROOT, "tools"))
    import check_rtc_registers as crr
    import rtc_isa_check as ric
    dec = pkg.Decoder(util.mask("FB_N1024_K512"))
    path = dec.to_info_path("int8", 65536)
    assert path["fused"] == 1 and path["workspace_bytes"] == 0
    assert 0 < path["regs"] <= dec.launch_info(65536)["regs"]
    cache = os.environ.get("POLAR_SC_RTC_CACHE") or os.path.join(os.path.dirname(pkg._build.LIB), "rtc_cache")
    co = crr.read_code(crr.find_code(cache, path["code_key"]))
    kd = ric.kernel_descriptors(co)["polar_sc_mask_info_kernel"]
    meta = ric.metadata(co)["polar_sc_mask_info_kernel"]
    print("C2 info kernel: %d VGPRs, %d AGPRs, private %d B" % (meta["vgpr_count"], meta["agpr_count"],
                                                                meta["private_segment_fixed_size"]))
    assert not meta["agpr_count"]
    assert kd["private_segment_fixed_size"] == 0 and kd["rsrc2_scratch_en"] == 0 and meta["private_segment_fixed_size"] == 0
