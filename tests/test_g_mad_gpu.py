"""The multiply-add G (polar_sc_device.h G_split) on the GPU: every decoder family that shares it,
bit-exact with the oracle's literal FSM on every frame at Eb/N0 = 1.0 dB, where the G clamp and
the |a| = |b| ties are common (tests/test_g_mad.py has the exhaustive CPU restatement).

  * the per-mask kernel: N = 1024 K = 512 on 67 frames (9 waves, the last one partial, 3 blocks)
    and N = 128 K = 64 on 19 frames
  * the pair kernel's subtree decoders: N = 2048 in SIGMAG, and in CA2 (stage magnitudes up to
    2^(Q-1), G clamp 31)
"""
import numpy as np
import pytest

import util
from test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu


def _run(pkg, torch, oracle_mod, name, batch, seed, **fmt):
    mask = util.mask(name)
    cfg = None
    if fmt:
        cfg = pkg.default_config()
        for k, v in fmt.items():
            setattr(cfg, k, v)
    llr, _ = util.synth_frames(mask, batch, ebn0_db=1.0, seed=seed)
    dec = pkg.Decoder(mask, config=cfg)
    out = dec.decode(torch.from_numpy(np.ascontiguousarray(llr)).cuda())
    torch.cuda.synchronize()
    got = pkg.unpack_bits(out.cpu().numpy(), mask.size)
    _assert_same(got, oracle_mod.decode_fsm(mask, llr, **fmt), "%s x %d %s" % (name, batch, fmt))
    return dec


@pytest.mark.parametrize("name,batch", [("FB_N1024_K512", 67), ("FB_N128_K64", 19)])
def test_mask_kernel_low_snr(pkg, cuda, oracle_mod, name, batch):
    dec = _run(pkg, cuda, oracle_mod, name, batch, seed=4100 + batch)
    info = dec.launch_info(batch)
    assert info["kernel"] == 1 and info["blocks"] == -(-(-(-batch // 8)) // 4), info


@pytest.mark.parametrize("fmt", [{}, {"sigmag": 0}], ids=["sigmag", "ca2"])
def test_pair_kernel_low_snr(pkg, cuda, oracle_mod, fmt):
    dec = _run(pkg, cuda, oracle_mod, "frozen_n_2048_k_1024", 9, seed=4200, **fmt)
    assert dec.stats["kernel"] == 3, dec.stats
