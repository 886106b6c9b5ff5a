#!/usr/bin/env python3
"""Speed of the device information-bit paths (polar_sc_xform.hip): extract_info and
encode on resident rows at the three benchmark shapes, HIP-event timed. Per shape one warm-up of
both directions, then --rounds interleaved rounds (extract, encode, extract, ...) of --steps
launches each; one JSON line per shape and direction with the per-round times, their median, the
bytes a launch has to move ((N + K) / 8 per frame) and that traffic over the median time. Parity
is tests/test_info_bits_gpu.py; nothing is checked here.

usage: python tools/info_bits_speed.py [--steps 1000] [--rounds 3] [--shapes name:frames,...]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "FB_N1024_K512:65536,frozen_n_16384_k_8192:4096,frozen_n_262144_k_131072:64"


def timed(torch, fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    args = ap.parse_args()
    import torch
    import sc_polar_decoder_hls_amd as pkg
    from sc_polar_decoder_hls_amd import _plansets
    if not torch.cuda.is_available():
        raise SystemExit("info_bits_speed: needs a GPU")
    for shape in args.shapes.split(","):
        name, frames = shape.split(":")
        frames = int(frames)
        dec = pkg.Decoder(_plansets.mask(name))        # (plan only: no decode kernel is built)
        gen = torch.Generator(device="cuda").manual_seed(dec.N)
        lim = 1 << 62
        x = torch.randint(-lim, lim, (frames, dec.words), dtype=torch.int64, device="cuda", generator=gen)
        info = torch.randint(-lim, lim, (frames, dec.info_words), dtype=torch.int64, device="cuda", generator=gen)
        xo, io = torch.empty_like(x), torch.empty_like(info)
        runs = {"extract_info": lambda: dec.extract_info(x, out=io), "encode": lambda: dec.encode(info, out=xo)}
        for fn in runs.values():                        # warm-up: table upload, code objects
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                us[k].append(timed(torch, fn, args.steps))
        nbytes = frames * (dec.N + 64 * dec.info_words) // 8
        for k, v in us.items():
            med = statistics.median(v)
            print(json.dumps({"op": k, "mask": name, "N": dec.N, "K": dec.K, "frames": frames, "steps": args.steps,
                              "us_rounds": [round(t, 2) for t in v], "us": round(med, 2), "bytes": nbytes,
                              "gbytes_per_s": round(nbytes / med / 1e3, 1),
                              "info_bits_per_s": frames * dec.K / (med * 1e-6)}), flush=True)
        dec.close()


if __name__ == "__main__":
    main()
