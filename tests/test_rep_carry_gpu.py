"""REP nodes whose zero totals take their sign from the last word's carried butterfly
(tests/test_rep_carry.py has the CPU restatement), on the GPU: bit-exact with the
oracle's literal FSM on every frame.

  * N = 1024 K = 512 at 1, 3, 4, 5, 8, 9 and 67 frames: waves with absent or clamped frames (whose
    totals take part in the wave's branch), and a partial last wave
  * an input whose pointer is not 16-byte aligned (the byte-copy staging)
  * N = 128 and N = 512: frames shorter than the 64 lanes of a DMA row
  * Eb/N0 = 1.0 dB, and tie-heavy frames (LLRs uniform in {-2, -1, 0, 1, 2, -32}; -32 is the
    channel's +0), where nearly every REP node meets a zero total
  * a hybrid kernel whose generated subtree decoders hold REP nodes
"""
import numpy as np
import pytest

import util
from sc_polar_decoder_hls_amd import _plansets

pytestmark = pytest.mark.gpu

TIES = np.array([-2, -1, 0, 1, 2, -32], np.int8)
C2 = "FB_N1024_K512"


def _assert_same(got, ref, what):
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, "%s: %d/%d frames differ (first %s)" % (what, bad.size, len(ref), bad[:8])


def _decode(pkg, torch, dec, llr_dev, N):
    out = dec.decode(llr_dev)
    torch.cuda.synchronize()
    return pkg.unpack_bits(out.cpu().numpy(), N)


@pytest.fixture(scope="module")
def c2(pkg, cuda, oracle_mod):
    """the C2 decoder, 67 noisy and 67 tie-heavy frames and their oracle decodes (shared, read only)"""
    mask = util.mask(C2)
    noisy, _ = util.synth_frames(mask, 67, ebn0_db=1.0, seed=7400)
    ties = np.random.default_rng(7401).choice(TIES, size=(67, mask.size))
    dec = pkg.Decoder(mask)
    return mask, dec, {"noisy": (noisy, oracle_mod.decode_fsm(mask, noisy)), "ties": (ties, oracle_mod.decode_fsm(mask, ties))}


def test_c2_kernel_is_the_new_form(c2):
    _, dec, _ = c2
    src = dec.kernel_source()
    assert dec.launch_info(67)["kernel"] == 1
    assert src.count("rep_carry_level<8, 1>") == 7 and src.count("// REP n") == 7
    info = dec.launch_info(65536)
    assert info["regs"] <= 104 and info["waves_per_block"] == 4, info


@pytest.mark.parametrize("kind", ["noisy", "ties"])
@pytest.mark.parametrize("batch", [1, 3, 4, 5, 8, 9, 67])
def test_c2_batches(pkg, cuda, c2, batch, kind):
    mask, dec, frames = c2
    llr, ref = frames[kind]
    got = _decode(pkg, cuda, dec, cuda.from_numpy(np.ascontiguousarray(llr[:batch])).cuda(), mask.size)
    _assert_same(got, ref[:batch], "%s %s x %d" % (C2, kind, batch))


@pytest.mark.parametrize("kind", ["noisy", "ties"])
@pytest.mark.parametrize("shift", [1, 7])
def test_c2_unaligned_input(pkg, cuda, c2, shift, kind):
    mask, dec, frames = c2
    llr, ref = frames[kind]
    buf = cuda.zeros(9 * mask.size + 16, dtype=cuda.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + 9 * mask.size].view(9, mask.size)
    view.copy_(cuda.from_numpy(np.ascontiguousarray(llr[:9])))
    assert view.data_ptr() % 16 == shift and view.is_contiguous()
    _assert_same(_decode(pkg, cuda, dec, view, mask.size), ref[:9], "%s %s unaligned by %d" % (C2, kind, shift))


@pytest.mark.parametrize("kind", ["noisy", "ties"])
@pytest.mark.parametrize("name", ["FB_N128_K64", "FB_N512_K256"])
def test_short_frames(pkg, cuda, oracle_mod, name, kind):
    mask = util.mask(name)
    if kind == "noisy":
        llr, _ = util.synth_frames(mask, 19, ebn0_db=1.0, seed=7500 + mask.size)
    else:
        llr = np.random.default_rng(7600 + mask.size).choice(TIES, size=(19, mask.size))
    dec = pkg.Decoder(mask)
    assert dec.launch_info(19)["kernel"] == 1
    got = _decode(pkg, cuda, dec, cuda.from_numpy(np.ascontiguousarray(llr)).cuda(), mask.size)
    _assert_same(got, oracle_mod.decode_fsm(mask, llr), "%s %s" % (name, kind))


@pytest.mark.parametrize("kind", ["noisy", "ties"])
def test_hybrid_subtree_rep_nodes(pkg, cuda, oracle_mod, kind):
    name, mask, _, tun = _plansets.issue_form_items()[0]
    if kind == "noisy":
        llr, _ = util.synth_frames(mask, 19, ebn0_db=1.0, seed=7700)
    else:
        llr = np.random.default_rng(7701).choice(TIES, size=(19, mask.size))
    dec = pkg.Decoder(mask, tuning=tun)
    src = dec.kernel_source()
    assert dec.stats["kernel"] == 2 and src.count("// REP n") >= 4 and "#define POLAR_REP_CARRY 1" in src
    got = _decode(pkg, cuda, dec, cuda.from_numpy(np.ascontiguousarray(llr)).cuda(), mask.size)
    _assert_same(got, oracle_mod.decode_fsm(mask, llr), "%s %s" % (name, kind))
