"""The packed SPC epilogue and the three-instruction output transpose of the per-mask kernel
(tests/test_spc_packed.py and tests/test_out_transpose.py have the CPU
restatements), on the GPU: bit-exact with the oracle's literal FSM on every frame.

  * N = 32, 64, 128 and 256 (sc_polar_decoder_hls_amd/_plansets.py SPC_PACKED_WORDS): the smallest
    codes whose pruned tree has a G+leaf record on the packed root (32), an SPC node of 1 word and
    an R1 node (64), SPC nodes of 1 and 2 words with an R1 node of 2 (128), SPC nodes of 1, 2 and 4
    words with an R1 node of 4 (256: an SPC node is a right child below the root's children, so
    one of 4 words needs a code of 16)
  * N = 1024 K = 512: SPC nodes of 1, 4 and 8 words (64 and 128 LLRs), ten G+leaf records
  * batches of 1, 7, 8, 9 and 67 frames (absent and clamped frames, a partial last wave), and an
    input pointer that is not 16-byte aligned
  * frames at Eb/N0 = 1.0 dB, tie-heavy frames (LLRs uniform in {-2 .. 2}: almost every SPC node
    meets a tied minimum, in the word and in the position), frames saturated at +-31 (every
    magnitude at the G clamp)
"""
import numpy as np
import pytest

import util
from sc_polar_decoder_hls_amd import _plansets

pytestmark = pytest.mark.gpu

C2 = "FB_N1024_K512"
KINDS = ("noisy", "ties", "saturated")
BATCHES = (1, 7, 8, 9, 67)
# (ops the plan must have: (code, words))
EXPECT = {
    "spc_n32": {("GLEAF", 1)},
    "spc_n64": {("SPC", 1), ("R1", 1)},
    "spc_n128": {("SPC", 1), ("SPC", 2), ("GLEAF", 1), ("R1", 2)},
    "spc_n256": {("SPC", 1), ("SPC", 2), ("SPC", 4), ("GLEAF", 1), ("R1", 4)},
    C2: {("SPC", 1), ("SPC", 4), ("SPC", 8), ("GLEAF", 1)},
}


def _mask(name):
    return util.mask(name) if name == C2 else _plansets.spc_packed_mask(name)


def _frames(mask, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "noisy":
        return util.synth_frames(mask, 67, ebn0_db=1.0, seed=seed)[0]
    if kind == "ties":
        return rng.integers(-2, 3, size=(67, mask.size)).astype(np.int8)
    return rng.choice(np.array([-31, 31], np.int8), size=(67, mask.size))


def _assert_same(got, ref, what):
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, "%s: %d/%d frames differ (first %s)" % (what, bad.size, len(ref), bad[:8])


def _decode(pkg, torch, dec, llr_dev, N):
    out = dec.decode(llr_dev)
    torch.cuda.synchronize()
    return pkg.unpack_bits(out.cpu().numpy(), N)


@pytest.fixture(scope="module")
def plans(pkg, cuda, oracle_mod):
    """per code: the mask, its decoder, 67 frames of each kind and their oracle decodes (shared, read only)"""
    out = {}
    for i, name in enumerate(EXPECT):
        mask = _mask(name)
        frames = {}
        for k, kind in enumerate(KINDS):
            llr = _frames(mask, kind, 8100 + 10 * i + k)
            frames[kind] = (llr, oracle_mod.decode_fsm(mask, llr))
        out[name] = (mask, pkg.Decoder(mask), frames)
    return out


@pytest.mark.parametrize("name", list(EXPECT))
def test_plan_has_the_ops_and_the_new_forms(plans, name):
    mask, dec, _ = plans[name]
    assert dec.launch_info(67)["kernel"] == 1
    ops = {(o["op"], o["n"]) for o in dec.schedule()}
    assert EXPECT[name] <= ops, ops
    src = dec.kernel_source()
    assert src.count("#if POLAR_SPC_PACKED(") == sum(1 for o in dec.schedule() if o["op"] == "SPC")
    assert "POLAR_TRANSPOSE16(v) row_transpose16_x(v, ot_)" in src and src.count("POLAR_TRANSPOSE16(to_position_order(") >= 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(EXPECT))
def test_batches(pkg, cuda, plans, name, kind):
    mask, dec, frames = plans[name]
    llr, ref = frames[kind]
    for batch in BATCHES:
        got = _decode(pkg, cuda, dec, cuda.from_numpy(np.ascontiguousarray(llr[:batch])).cuda(), mask.size)
        _assert_same(got, ref[:batch], "%s %s x %d" % (name, kind, batch))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["spc_n128", C2])
def test_unaligned_input(pkg, cuda, plans, name, kind):
    mask, dec, frames = plans[name]
    llr, ref = frames[kind]
    buf = cuda.zeros(9 * mask.size + 16, dtype=cuda.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[5:5 + 9 * mask.size].view(9, mask.size)
    view.copy_(cuda.from_numpy(np.ascontiguousarray(llr[:9])))
    assert view.data_ptr() % 16 == 5 and view.is_contiguous()
    _assert_same(_decode(pkg, cuda, dec, view, mask.size), ref[:9], "%s %s unaligned by 5" % (name, kind))
