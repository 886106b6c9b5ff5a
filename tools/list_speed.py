#!/usr/bin/env python3
"""Speed of list decoding, HIP-event timed. Per shape: decode_list at --lists (L = 1
.. 8: the narrow kernel, 16 and 32: the wide-list kernel; with an 8-bit CRC, so that the CRC pass over the candidates is in the time), next to
decode_to_info of the same frames for scale (plain SC in the reference datapath; a different
decoding rule, so the outputs are not compared). One warm-up of every way, then --rounds
interleaved rounds of --steps calls each; one JSON line per shape and way with the per-round
times, their median and spread (max - min), frames per second, and for the list kernel its LDS
per wave and waves per block. Written to --out as well when given
(profiles/list_wide_speed.jsonl). --precode POLY,LEN adds decode_list(precode=(POLY, LEN)) of the same
frames at every L to the same rounds (profiles/list_precoded_speed.jsonl).

usage: python tools/list_speed.py [--steps 10] [--rounds 5] [--shapes name:frames,...] [--lists 1,2,...]
                                  [--precode POLY,LEN] [--out FILE]
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
CRC = (0x07, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--lists", default="1,2,4,8,16,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--precode", default=None, metavar="POLY,LEN",
                    help="also time decode_list(precode=(POLY, LEN)) at every L, next to the plain call in the same "
                         "rounds (DESIGN.md 3.11, Precoded codes; e.g. 0x6D,7)")
    args = ap.parse_args()
    precode = tuple(int(x, 0) for x in args.precode.split(",")) if args.precode else None
    import torch
    import sc_polar_decoder_hls_amd as pkg
    from sc_polar_decoder_hls_amd import _plansets
    from soft_speed import timed
    if not torch.cuda.is_available():
        raise SystemExit("list_speed: needs a GPU")
    lines = []
    for shape in args.shapes.split(","):
        name, frames = shape.split(":")
        frames = int(frames)
        dec = pkg.Decoder(_plansets.mask(name))
        gen = torch.Generator(device="cuda").manual_seed(dec.N)
        sign = torch.randint(0, 2, (frames, dec.N), device="cuda", generator=gen).float() * 2 - 1
        v = pkg.quantize(sign + 0.794 * torch.randn((frames, dec.N), device="cuda", generator=gen), 4, -31, 31)
        del sign
        info = torch.empty((frames, dec.info_words), dtype=torch.int64, device="cuda")
        rank = torch.empty((frames,), dtype=torch.uint8, device="cuda")
        runs = {"decode_to_info": lambda: dec.decode_to_info(v, out=info)}
        for L in (int(x) for x in args.lists.split(",")):
            runs["decode_list L=%d" % L] = lambda L=L: dec.decode_list(v, L, crc=CRC, out=info, rank=rank)
            if precode:     # (the same frames: the time of a walk does not depend on what the bits mean)
                runs["decode_list precoded L=%d" % L] = lambda L=L: dec.decode_list(v, L, crc=CRC, out=info, rank=rank,
                                                                                     precode=precode)
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
            if k != "decode_to_info":
                lds, wpb = pkg.list_shape(dec.N, int(k.split("=")[1]))
                rec.update(lds_bytes_per_wave=lds, waves_per_block=wpb)
                if "precoded" in k:
                    rec.update(conv_poly=precode[0], conv_len=precode[1])
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        dec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
