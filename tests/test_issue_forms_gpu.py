"""The cheaper instruction forms of the per-mask kernel (tests/test_issue_forms.py has the CPU
restatements) on the GPU: bit-exact with the oracle's literal FSM on every frame at Eb/N0 = 1.0 dB.

  * N = 1024 K = 512 at 1, 8, 9, 33 and 67 frames: full and partial last waves, so the 32-bit
    frame clamp of the fetch and both store predicates are taken and not taken; and once from an
    input tensor offset by one byte (the byte-copy path next to the clamped fetch)
  * N = 128 K = 64 at 19 frames: frames of fewer than 64 chunks, the lane-masked fetch
  * N = 1024 K = 922 at 9 frames: SPC- and R1-heavy, SPC nodes of up to 32 words (the flip as a
    shifted condition at the word indices of a plane)
  * a hybrid plan whose subtree decoders hold an SPC node of 128 words: the flip over several planes
  * N = 2048 on the pair kernel in SIGMAG and CA2: G_split's multiplier, shared with its subtrees
"""
import numpy as np
import pytest

import util
from sc_polar_decoder_hls_amd import _plansets
from test_gpu_parity import _assert_same

pytestmark = pytest.mark.gpu


def _decode(pkg, torch, oracle_mod, mask, batch, seed, what, tuning=None, offset=0, **fmt):
    cfg = None
    if fmt:
        cfg = pkg.default_config()
        for k, v in fmt.items():
            setattr(cfg, k, v)
    llr, _ = util.synth_frames(mask, batch, ebn0_db=1.0, seed=seed)
    dec = pkg.Decoder(mask, config=cfg, tuning=tuning)
    if offset:
        raw = torch.zeros(llr.size + 64, dtype=torch.int8, device="cuda")
        dev = raw[offset:offset + llr.size].view(batch, mask.size)
        dev.copy_(torch.from_numpy(np.ascontiguousarray(llr)))
        assert dev.data_ptr() % 16 == offset
    else:
        dev = torch.from_numpy(np.ascontiguousarray(llr)).cuda()
    out = dec.decode(dev)
    torch.cuda.synchronize()
    got = pkg.unpack_bits(out.cpu().numpy(), mask.size)
    _assert_same(got, oracle_mod.decode_fsm(mask, llr, **fmt), "%s x %d %s" % (what, batch, fmt))
    return dec


@pytest.mark.parametrize("batch", [1, 8, 9, 33, 67])
def test_c2_partial_waves(pkg, cuda, oracle_mod, batch):
    dec = _decode(pkg, cuda, oracle_mod, util.mask("FB_N1024_K512"), batch, 4300 + batch, "FB_N1024_K512")
    info = dec.launch_info(batch)
    assert info["kernel"] == 1 and info["blocks"] == -(-(-(-batch // 8)) // 4), info


def test_c2_unaligned_input(pkg, cuda, oracle_mod):
    dec = _decode(pkg, cuda, oracle_mod, util.mask("FB_N1024_K512"), 9, 4400, "FB_N1024_K512 + 1 byte", offset=1)
    assert dec.launch_info(9)["kernel"] == 1


def test_n128_masked_fetch(pkg, cuda, oracle_mod):
    dec = _decode(pkg, cuda, oracle_mod, util.mask("FB_N128_K64"), 19, 4500, "FB_N128_K64")
    assert dec.launch_info(19)["kernel"] == 1


def test_high_rate_spc_nodes(pkg, cuda, oracle_mod):
    mask = util.mask("frozen_n_1024_k_922")
    dec = _decode(pkg, cuda, oracle_mod, mask, 9, 4600, "frozen_n_1024_k_922")
    assert dec.launch_info(9)["kernel"] == 1
    spc = [o["n"] for o in dec.schedule() if o["op"] == "SPC"]
    assert len(spc) >= 8 and max(spc) == 16, spc   # (n: words per half of the node)


def test_hybrid_wide_spc_node(pkg, cuda, oracle_mod):
    (_, mask, _, tun), = _plansets.issue_form_items()
    dec = _decode(pkg, cuda, oracle_mod, mask, 9, 4700, "wide_spc4096", tuning=tun)
    assert dec.stats["kernel"] == 2 and "// SPC n 64 " in dec.kernel_source(), dec.stats


@pytest.mark.parametrize("fmt", [{}, {"sigmag": 0}], ids=["sigmag", "ca2"])
def test_pair_kernel_shared_g(pkg, cuda, oracle_mod, fmt):
    dec = _decode(pkg, cuda, oracle_mod, util.mask("frozen_n_2048_k_1024"), 9, 4800, "frozen_n_2048_k_1024", **fmt)
    assert dec.stats["kernel"] == 3, dec.stats
