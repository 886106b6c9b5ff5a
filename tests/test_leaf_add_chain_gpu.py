"""Runs of frozen-left levels of the leaf as an exact-add chain (tests/test_leaf_add_chain.py has
the CPU restatements) on the GPU: bit-exact with the oracle's literal FSM on every frame.

  * masks whose leaf records hold each new shape: N = 32 with 0000 0000 0000 0111 (two levels above an
    SPC block) and 0000 0000 0001 0111 (one level above a mixed block); N = 64 with 0000 0011 .. (two
    levels above an all-information pair, then a pair (frozen, information) below a non-frozen left
    sibling), a run at a mirrored quad (.. 0011 at positions 12..15) and three levels; N = 128 K = 64;
    N = 1024 K = 512
  * batches of 1, 8, 9 and 67 frames at Eb/N0 = 1.0 dB, tie-heavy frames (LLRs from {-2 .. 2}: almost
    every partial sum of a run meets 0) and saturated frames; an input 5 bytes off a 16-byte boundary
  * N = 2048 on the pair kernel, whose subtree leaves share the header
"""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

C2 = "FB_N1024_K512"
WORDS = {      # 16-LLR words, position 0 first
    "run_n32": ("0000000000000111", "0000000000010111"),
    "run_n64": ("0000000000000011", "0000001101010111", "0000011000110011", "0101011101111111"),
}
KINDS = ("noisy", "ties", "saturated")
BATCHES = (1, 8, 9, 67)


def _mask(name):
    if name in WORDS:
        return np.array([int(c) for w in WORDS[name] for c in w], np.uint8)
    return util.mask(name)


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
    for i, name in enumerate(list(WORDS) + ["FB_N128_K64", C2]):
        mask = _mask(name)
        frames = {}
        for k, kind in enumerate(KINDS):
            llr = _frames(mask, kind, 9100 + 10 * i + k)
            frames[kind] = (llr, oracle_mod.decode_fsm(mask, llr))
        out[name] = (mask, pkg.Decoder(mask), frames)
    return out


def _runs(dec):
    """(levels of frozen-left runs, pairs (frozen, information)) that leaf_ms meets in the plan's leaf
    records below the blocks it decides directly"""
    runs = pairs = 0
    for o in dec.schedule():
        if o["op"] not in ("FLEAF", "GLEAF") or (o["fb"] >> 16) & 7:
            continue
        todo = [(0, 16)]
        while todo:
            b, w = todo.pop()
            sub = (o["fb"] >> b) & ((1 << w) - 1)
            if sub in (0, (1 << w) - 1):
                continue
            if w == 2:
                pairs += sub == 2
            elif w <= 8 and sub in (1 << (w - 1), (1 << w) - 2):
                continue
            else:
                runs += sub & ((1 << (w // 2)) - 1) == 0
                todo += [(b, w // 2), (b + w // 2, w // 2)]
    return runs, pairs


@pytest.mark.parametrize("name,expect", [("run_n32", (3, 0)), ("run_n64", (8, 5)), (C2, (11, 0))])
def test_plan_has_the_shapes(plans, name, expect):
    dec = plans[name][1]
    assert dec.launch_info(67)["kernel"] == 1
    words = {"".join(str((o["fb"] >> i) & 1) for i in range(16)) for o in dec.schedule() if o["op"] in ("FLEAF", "GLEAF")}
    if name in WORDS:
        assert set(WORDS[name]) <= words, words
    assert _runs(dec) == expect, _runs(dec)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(WORDS) + ["FB_N128_K64", C2])
def test_batches(pkg, cuda, plans, name, kind):
    mask, dec, frames = plans[name]
    llr, ref = frames[kind]
    for batch in BATCHES:
        got = _decode(pkg, cuda, dec, cuda.from_numpy(np.ascontiguousarray(llr[:batch])).cuda(), mask.size)
        _assert_same(got, ref[:batch], "%s %s x %d" % (name, kind, batch))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["run_n64", C2])
def test_unaligned_input(pkg, cuda, plans, name, kind):
    mask, dec, frames = plans[name]
    llr, ref = frames[kind]
    buf = cuda.zeros(9 * mask.size + 16, dtype=cuda.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[5:5 + 9 * mask.size].view(9, mask.size)
    view.copy_(cuda.from_numpy(np.ascontiguousarray(llr[:9])))
    assert view.data_ptr() % 16 == 5 and view.is_contiguous()
    _assert_same(_decode(pkg, cuda, dec, view, mask.size), ref[:9], "%s %s unaligned by 5" % (name, kind))


def test_pair_kernel(pkg, cuda, oracle_mod):
    mask = util.mask("frozen_n_2048_k_1024")
    llr, _ = util.synth_frames(mask, 4, ebn0_db=1.0, seed=9300)
    dec = pkg.Decoder(mask)
    got = _decode(pkg, cuda, dec, cuda.from_numpy(np.ascontiguousarray(llr)).cuda(), mask.size)
    assert dec.stats["kernel"] == 3, dec.stats
    _assert_same(got, oracle_mod.decode_fsm(mask, llr), "frozen_n_2048_k_1024 x 4")
