#!/usr/bin/env python3
"""Speed of decoding from float channel values, HIP-event timed. Per shape and
input type, four ways to the same hard bits:
  (a) decode            the int8 frames, already quantized: the existing path, the yardstick
  (b) quantize+decode   the stand-alone quantizer kernel into a buffer, then (a)
  (c) decode_soft       the library's choice: the fused per-mask kernel, or (b) through a workspace
  (d) torch+decode      the quantizer as torch expressions (multiply, truncate, clamp, cast), then (a)
One warm-up of all four, then --rounds interleaved rounds (a, b, c, d, a, ...) of --steps calls
each; one JSON line per shape, type and way with the per-round times, their median and spread
(max - min), and for (c) what soft_info reports. The four results are compared once before the
timing. Written to --out as well when given (profiles/<round>_soft_speed.jsonl).

usage: python tools/soft_speed.py [--steps 200] [--rounds 5] [--shapes name:frames,...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "FB_N1024_K512:65536,frozen_n_16384_k_8192:4096"
BETA, LIM = 4, 31


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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--dtypes", default="float32,float16,bfloat16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sc_polar_decoder_hls_amd as pkg
    from sc_polar_decoder_hls_amd import _plansets
    if not torch.cuda.is_available():
        raise SystemExit("soft_speed: needs a GPU")
    lines = []
    for shape in args.shapes.split(","):
        name, frames = shape.split(":")
        frames = int(frames)
        dec = pkg.Decoder(_plansets.mask(name))
        gen = torch.Generator(device="cuda").manual_seed(dec.N)
        sign = torch.randint(0, 2, (frames, dec.N), device="cuda", generator=gen).float() * 2 - 1
        v32 = sign + 0.794 * torch.randn((frames, dec.N), device="cuda", generator=gen)   # BPSK + AWGN, 2 dB at rate 1/2
        del sign
        out = torch.empty((frames, dec.words), dtype=torch.int64, device="cuda")
        q = torch.empty((frames, dec.N), dtype=torch.int8, device="cuda")
        for dtype in args.dtypes.split(","):
            v = v32.to(getattr(torch, dtype))
            info = dec.soft_info(v.dtype, frames)
            ws = torch.empty(max(16, info["workspace_bytes"]), dtype=torch.uint8, device="cuda")
            llr = pkg.quantize(v, BETA, -LIM, LIM)

            def torch_chain():
                return dec.decode((v.float() * BETA).trunc().clamp(-LIM, LIM).to(torch.int8), out=out)

            runs = {"decode": lambda: dec.decode(llr, out=out),
                    "quantize+decode": lambda: dec.decode(pkg.quantize(v, BETA, -LIM, LIM, out=q), out=out),
                    "decode_soft": lambda: dec.decode_soft(v, BETA, -LIM, LIM, out=out, workspace=ws),
                    "torch+decode": torch_chain}
            ref = None
            for k, fn in runs.items():                   # warm-up: code objects, allocator; and one comparison
                for _ in range(3):
                    got = fn().clone()
                ref = got if ref is None else ref
                if not torch.equal(got, ref):
                    raise SystemExit("soft_speed: %s differs from decode at %s %s" % (k, name, dtype))
            torch.cuda.synchronize()
            us = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    us[k].append(timed(torch, fn, args.steps))
            for k, t in us.items():
                rec = {"way": k, "mask": name, "N": dec.N, "frames": frames, "dtype": dtype, "steps": args.steps,
                       "us_rounds": [round(x, 2) for x in t], "us": round(statistics.median(t), 2),
                       "spread_us": round(max(t) - min(t), 2), "input_bytes": v.numel() * v.element_size()}
                if k == "decode_soft":
                    rec.update(fused=info["fused"], regs=info["regs"], code_key=info["code_key"])
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            del v, ws, llr
        dec.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
