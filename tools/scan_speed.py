#!/usr/bin/env python3
"""Speed of soft-output (SCAN) decoding, HIP-event timed. Per shape: decode_scan at
--iterations (ext and the hard rows written), next to decode_list with L = 1 (the same tree walked bit
by bit through LDS) and decode_to_info (plain SC in the reference datapath) of the same frames for
scale; the three follow different rules, so their outputs are not compared. One warm-up of every way,
then --rounds interleaved rounds of --steps calls each; one JSON line per shape and way with the
per-round times, their median and spread (max - min), frames per second, and for the scan kernel its
LDS per wave and waves per block. Written to --out as well when given (profiles/scan_speed.jsonl).

usage: python tools/scan_speed.py [--steps 10] [--rounds 5] [--shapes name:frames,...] [--iterations 1,2,4]
                                  [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = "FB_N1024_K512:16384,FB_N128_K64:16384"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--iterations", default="1,2,4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sc_polar_decoder_hls_amd as pkg
    from sc_polar_decoder_hls_amd import _plansets
    from soft_speed import timed
    if not torch.cuda.is_available():
        raise SystemExit("scan_speed: needs a GPU")
    lines = []
    for shape in args.shapes.split(","):
        name, frames = shape.split(":")
        frames = int(frames)
        dec = pkg.Decoder(_plansets.mask(name))
        gen = torch.Generator(device="cuda").manual_seed(dec.N)
        sign = torch.randint(0, 2, (frames, dec.N), device="cuda", generator=gen).float() * 2 - 1
        v = pkg.quantize(sign + 0.794 * torch.randn((frames, dec.N), device="cuda", generator=gen), 4, -31, 31)   # 2 dB at rate 1/2
        del sign
        info = torch.empty((frames, dec.info_words), dtype=torch.int64, device="cuda")
        rank = torch.empty((frames,), dtype=torch.uint8, device="cuda")
        ext = torch.empty((frames, dec.N), dtype=torch.int16, device="cuda")
        hard = torch.empty((frames, dec.words), dtype=torch.int64, device="cuda")
        runs = {"decode_to_info": lambda: dec.decode_to_info(v, out=info),
                "decode_list L=1": lambda: dec.decode_list(v, 1, out=info, rank=rank)}
        for it in (int(x) for x in args.iterations.split(",")):
            runs["decode_scan iterations=%d" % it] = lambda it=it: dec.decode_scan(v, it, out=ext, hard=hard)
        for fn in runs.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                us[k].append(timed(torch, fn, args.steps))
        for k, t in us.items():
            med = statistics.median(t)
            rec = {"way": k, "mask": name, "N": dec.N, "K": dec.K, "frames": frames, "steps": args.steps,
                   "us_rounds": [round(x, 2) for x in t], "us": round(med, 2), "spread_us": round(max(t) - min(t), 2),
                   "mframes_per_s": round(frames / med, 3)}
            if k.startswith("decode_scan"):
                lds, wpb = pkg.scan_shape(dec.N, int(k.split("=")[1]))
                rec.update(lds_bytes_per_wave=lds, waves_per_block=wpb)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        dec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
