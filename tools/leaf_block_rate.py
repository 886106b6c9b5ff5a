#!/usr/bin/env python3
"""How often a REP sub-block of the 16-LLR leaf has a zero total, and an SPC sub-block a tied
minimum under odd parity (CPU only; DESIGN.md 3.1: the choice between carrying the sign of the
last non-zero partial sum and a wave-uniform fallback to the recursion).

Decodes C-sim frames with the numpy schedule interpreter of tests/util.py, whose leaf recursion
is replaced by an instrumented copy that looks at every REP / SPC sub-block of width 4 and 8 the
device leaf decides directly. A wave of the per-mask kernel carries 8 frames, so a wave-uniform
fallback runs when any of 8 consecutive frames has a zero total in that block.

    python tools/leaf_block_rate.py [--mask FB_N1024_K512] [--frames 4096] [--ebn0 2.5,1.0]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Stats:
    def __init__(self):
        self.rep = []   # per REP block instance: bool [frames], total == 0
        self.spc = []   # per SPC block instance: bool [frames], odd parity and a tied minimum


def instrumented_leaf(util, st):
    def leaf(lam, fb, n=16, count=True):
        s, m = lam
        if count and n in (4, 8) and fb == 1 << (n - 1):
            st.rep.append(np.where(s, -m, m).sum(axis=1) == 0)
            count = False                                  # (its own halves are not blocks of the device leaf)
        if count and n in (4, 8) and fb == (1 << n) - 2:
            srt = np.sort(m, axis=1)
            st.spc.append(((s.sum(axis=1) & 1) == 1) & (srt[:, 0] == srt[:, 1]))
            count = False
        if n == 2:
            f0, f1 = fb & 1, (fb >> 1) & 1
            u0 = (s[:, 0] ^ s[:, 1]) & f0
            sg = np.where(m[:, 0] < m[:, 1], s[:, 1], s[:, 0] ^ u0) & f1
            return np.stack([u0 ^ sg, sg], axis=1)
        h = n // 2
        a, b = (s[:, :h], m[:, :h]), (s[:, h:], m[:, h:])
        xa = leaf(util.F(a, b), fb & ((1 << h) - 1), h, count)
        xb = leaf(util.G(a, b, xa), fb >> h, h, count)
        return np.concatenate([xa ^ xb, xb], axis=1)
    return lambda lam, fb: leaf(lam, fb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mask", default="FB_N1024_K512")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--ebn0", default="2.5,1.0")
    ap.add_argument("--ties", action="store_true", help="LLRs uniform in {-2, -1, 0, 1, 2, -32} instead of C-sim frames")
    args = ap.parse_args()
    import sc_polar_decoder_hls_amd as pkg
    import util
    mask = util.mask(args.mask)
    ops = pkg.Decoder(mask).schedule()
    plain = util.leaf
    for e in [float(x) for x in args.ebn0.split(",")]:
        if args.ties:
            llr = np.random.default_rng(7).choice(np.array([-2, -1, 0, 1, 2, -32], np.int8), (args.frames, mask.size))
        else:
            llr, _ = util.synth_frames(mask, args.frames, ebn0_db=e, seed=0xF0)
        st = Stats()
        util.leaf = instrumented_leaf(util, st)
        try:
            util.run_schedule(ops, mask.size, llr)
        finally:
            util.leaf = plain
        # (run_schedule looks `leaf` up in its module at call time; were that to change, say so)
        assert st.rep and st.spc, "tests/util.run_schedule did not go through the instrumented leaf"
        what = "tie-heavy LLRs" if args.ties else "Eb/N0 %.1f dB" % e
        for name, rows in (("REP zero total", st.rep), ("SPC tied minimum, odd parity", st.spc)):
            z = np.array(rows)                                     # [block instance, frame]
            w = z[:, : z.shape[1] // 8 * 8].reshape(z.shape[0], -1, 8).any(axis=2)
            print("%s, %s, %d frames: %d blocks per frame; %s in %.2f %% of blocks per frame (%.3f blocks per frame); "
                  "any of a wave's 8 frames in %.2f %% of blocks (%.2f blocks per wave, a block-free wave %.1f %%)"
                  % (args.mask, what, z.shape[1], z.shape[0], name, 100 * z.mean(), z.sum(axis=0).mean(),
                     100 * w.mean(), w.sum(axis=0).mean(), 100 * (~w.any(axis=0)).mean()))
        if args.ties:
            break


if __name__ == "__main__":
    main()
