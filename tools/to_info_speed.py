#!/usr/bin/env python3
"""Speed of decoding straight to information words, HIP-event timed. Per shape
and input (int8 LLRs and the three float types), three ways:
  (a) decode            decode() of int8 frames / decode_soft() of float values: x^ only, the yardstick
  (b) decode+extract    (a), then extract_info() of its x^: the two launches this replaces
  (c) decode_to_info    the library's choice: one kernel on per-mask plans, else (b) through a workspace
One warm-up of all three, then --rounds interleaved rounds (a, b, c, a, ...) of --steps calls each;
one JSON line per shape, input and way with the per-round times, their median and spread
(max - min), and for (c) what to_info_path reports. (b) and (c) are compared once before the
timing. Written to --out as well when given (profiles/<round>_to_info_speed.jsonl).

usage: python tools/to_info_speed.py [--steps 200] [--rounds 5] [--shapes name:frames,...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = "FB_N1024_K512:65536"
BETA, LIM = 4, 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--dtypes", default="int8,float32,float16,bfloat16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sc_polar_decoder_hls_amd as pkg
    from sc_polar_decoder_hls_amd import _plansets
    from soft_speed import timed
    if not torch.cuda.is_available():
        raise SystemExit("to_info_speed: needs a GPU")
    lines = []
    for shape in args.shapes.split(","):
        name, frames = shape.split(":")
        frames = int(frames)
        dec = pkg.Decoder(_plansets.mask(name))
        gen = torch.Generator(device="cuda").manual_seed(dec.N)
        sign = torch.randint(0, 2, (frames, dec.N), device="cuda", generator=gen).float() * 2 - 1
        v32 = sign + 0.794 * torch.randn((frames, dec.N), device="cuda", generator=gen)   # BPSK + AWGN, 2 dB at rate 1/2
        del sign
        xhat = torch.empty((frames, dec.words), dtype=torch.int64, device="cuda")
        info = torch.empty((frames, dec.info_words), dtype=torch.int64, device="cuda")
        for dtype in args.dtypes.split(","):
            v = pkg.quantize(v32, BETA, -LIM, LIM) if dtype == "int8" else v32.to(getattr(torch, dtype))
            path = dec.to_info_path(v.dtype, frames)
            ws = torch.empty(max(16, path["workspace_bytes"]), dtype=torch.uint8, device="cuda")
            if dtype == "int8":
                def decode():
                    return dec.decode(v, out=xhat)
            else:
                sws = torch.empty(max(16, dec.soft_info(v.dtype, frames)["workspace_bytes"]), dtype=torch.uint8,
                                  device="cuda")

                def decode():
                    return dec.decode_soft(v, BETA, -LIM, LIM, out=xhat, workspace=sws)
            runs = {"decode": decode,
                    "decode+extract": lambda: dec.extract_info(decode(), out=info),
                    "decode_to_info": lambda: dec.decode_to_info(v, BETA, -LIM, LIM, out=info, workspace=ws)}
            ref = None
            for k in ("decode+extract", "decode_to_info"):   # warm-up: code objects, allocator; and one comparison
                for _ in range(3):
                    got = runs[k]().clone()
                ref = got if ref is None else ref
                if not torch.equal(got, ref):
                    raise SystemExit("to_info_speed: %s differs from decode+extract at %s %s" % (k, name, dtype))
            torch.cuda.synchronize()
            us = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    us[k].append(timed(torch, fn, args.steps))
            for k, t in us.items():
                rec = {"way": k, "mask": name, "N": dec.N, "K": dec.K, "frames": frames, "dtype": dtype,
                       "steps": args.steps, "us_rounds": [round(x, 2) for x in t], "us": round(statistics.median(t), 2),
                       "spread_us": round(max(t) - min(t), 2)}
                if k == "decode":
                    rec.update(code_key=dec.launch_info(frames)["code_key"] if dtype == "int8"
                               else dec.soft_info(v.dtype, frames)["code_key"])
                if k == "decode_to_info":
                    rec.update(fused=path["fused"], regs=path["regs"], code_key=path["code_key"])
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            del v, ws
        dec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
