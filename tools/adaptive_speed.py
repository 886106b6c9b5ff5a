#!/usr/bin/env python3
"""Speed of adaptive CRC-aided decoding, HIP-event timed. Per shape and Eb/N0:
decode_to_info, crc_check of its result, and per list size of --lists (8, 16, 32) decode_list and
decode_adaptive of the same frames (an 8-bit CRC), with the fraction of frames the adaptive call sent
to the list decoder (stage 1) and the frame errors left at that list size.
The frames are codewords of crc_attach payloads (256 distinct ones, repeated) through BPSK and AWGN,
quantized as the reference's testbench does (beta 4, +-31). One warm-up of every way, a comparison
of decode_adaptive with its two stages run apart, then --rounds interleaved rounds of --steps calls
each; one JSON line per shape, Eb/N0 and way with the per-round times, their median and spread
(max - min), and for decode_adaptive the frame errors and the sum it is expected to sit near: decode_to_info + crc_check
+ stage-1 fraction x decode_list of the same run. Written to --out as well when given
(profiles/adaptive_speed.jsonl).

usage: python tools/adaptive_speed.py [--steps 10] [--rounds 5] [--shapes name:frames,...] [--ebn0 1,2,3] [--lists 8,16,32]
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
CRC = (0x07, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--ebn0", default="1,2,3")
    ap.add_argument("--lists", default="8,16,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import sc_polar_decoder_hls_amd as pkg
    from sc_polar_decoder_hls_amd import _plansets
    from soft_speed import timed
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_speed: needs a GPU")
    lines = []
    for shape in args.shapes.split(","):
        name, frames = shape.split(":")
        frames = int(frames)
        dec = pkg.Decoder(_plansets.mask(name))
        payload = np.random.default_rng(dec.N).integers(0, 2, size=(256, dec.K - CRC[1]), dtype=np.uint8)
        words = np.tile(pkg.crc_attach(pkg.pack_bits(payload), dec.K, *CRC), (-(-frames // 256), 1))[:frames]
        xw = dec.encode(torch.from_numpy(words.view(np.int64)).cuda())
        shifts = torch.arange(64, device="cuda", dtype=torch.int64)
        bpsk = 1.0 - 2.0 * ((xw[:, :, None] >> shifts) & 1).reshape(frames, -1)[:, :dec.N].float()
        gen = torch.Generator(device="cuda").manual_seed(dec.N)
        noise = torch.randn((frames, dec.N), device="cuda", generator=gen)
        info = torch.empty((frames, dec.info_words), dtype=torch.int64, device="cuda")
        sc = torch.empty_like(info)
        rank, stage, ok = (torch.empty((frames,), dtype=torch.uint8, device="cuda") for _ in range(3))
        ws = torch.empty(dec.adaptive_workspace(frames), dtype=torch.uint8, device="cuda")
        for db in (float(x) for x in args.ebn0.split(",")):
            sigma = 1.0 / (2.0 * dec.K / dec.N * 10.0 ** (db / 10.0)) ** 0.5
            v = pkg.quantize(bpsk + sigma * noise, 4, -31, 31)
            lists = [int(x) for x in args.lists.split(",")]
            runs = {"decode_to_info": lambda: dec.decode_to_info(v, out=sc),
                    "crc_check": lambda: dec.crc_check(sc, CRC, out=ok)}
            for L in lists:
                runs["decode_list L=%d" % L] = lambda L=L: dec.decode_list(v, L, crc=CRC, out=info, rank=rank)
                runs["decode_adaptive L=%d" % L] = lambda L=L: dec.decode_adaptive(v, L, CRC, out=info, rank=rank,
                                                                                   stage=stage, workspace=ws)
            for fn in runs.values():
                for _ in range(2):
                    fn()
            # compare decode_adaptive with its stages run apart, and count what it leaves wrong
            frac, frame_errors = {}, {}
            for L in lists:
                runs["decode_adaptive L=%d" % L]()
                listed = dec.decode_list(v, L, crc=CRC)[0]
                if not torch.equal(stage, 1 - ok) or not torch.equal(info, torch.where(ok[:, None] == 1, sc, listed)):
                    raise SystemExit("adaptive_speed: decode_adaptive differs from its stages at %s %.1f dB L=%d"
                                     % (name, db, L))
                frac[L] = float(stage.float().mean())
                frame_errors[L] = int((info != xw.new_tensor(words.view(np.int64))).any(dim=1).sum())
            torch.cuda.synchronize()
            us = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, fn in runs.items():
                    us[k].append(timed(torch, fn, args.steps))
            med = {k: statistics.median(t) for k, t in us.items()}
            for k, t in us.items():
                L = int(k.split("=")[1]) if "=" in k else None
                rec = {"way": k.split(" ")[0], "mask": name, "N": dec.N, "K": dec.K, "frames": frames, "ebn0_db": db, "L": L,
                       "crc": list(CRC), "steps": args.steps, "us_rounds": [round(x, 2) for x in t],
                       "us": round(med[k], 2), "spread_us": round(max(t) - min(t), 2),
                       "stage1_fraction": round(frac[lists[0]], 5)}
                if k.startswith("decode_adaptive"):
                    rec.update(expected_us=round(med["decode_to_info"] + med["crc_check"]
                                                 + frac[L] * med["decode_list L=%d" % L], 2),
                               frame_errors=frame_errors[L], workspace_bytes=ws.numel())
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
        dec.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
