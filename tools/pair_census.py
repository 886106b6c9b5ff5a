#!/usr/bin/env python3
"""Static instruction census of a pair plan's generated subtree decoders (CPU only).

Takes the plan's generated source (Decoder.kernel_source()), puts an asm comment marker in
front of every schedule op of every subtree decoder (`// F n 8`, `// F+leaf ...`, ...), compiles
it to assembly with the ROCm clang driver the library uses, and attributes every instruction
between two markers to that op's class (F / G / REP / R1 / SPC / H / leaf, by node width). The
markers are `asm volatile` comments, so the scheduler cannot move work across them: the counts
are those of a slightly less scheduled build, good to a few per cent.

Weighted by the number of calls of each decoder in the schedule, the totals are the static
VALU count of one frame pair's (or frame's) subtree work -- the serial instruction chain of a
long-block decode.

    python tools/pair_census.py [--mask frozen_n_262144_k_131072] [--tuning k=v,...]

--cycles (per-mask kernels): every VALU instruction weighted by the issue cost of its form at the
plan's occupancy (the table below), per op class with the costliest mnemonics;
forms the microbenchmark has not measured are listed as unpriced, with their count, not guessed.
--no-rep-fallback leaves the exact REP fallback bodies out (they run only when a REP total is 0),
so that the count tracks the executed stream; --defines builds another form of the kernel
(-DPOLAR_... switches) for comparison.

    python tools/pair_census.py --mask FB_N1024_K512 --cycles --no-rep-fallback [--defines POLAR_PM1_MASK,...]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "sc_polar_decoder_hls_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# ---- issue cost per instruction form: SIMD cycles per wave64 instruction at
# 1 / 2 / 4 / 8 waves per SIMD, tools/valu_microbench.hip (profiles/r02_valu_microbench.log,
# r04_valu_microbench_{encoding,forms}.log, r08_valu_microbench_forms.log)
WAVES = (1, 2, 4, 8)
DUAL = (4.8, 2.4, 1.97, 1.45)        # 32- / 16-bit VOP1 / VOP2, VGPR, inline or literal operands (also as _e64)
SINGLE = (5.2, 4.45, 3.25, 2.62)     # v_pk_*, DPP, 3-source VOP3, v_lshlrev_b32, v_min_u32, VOP2 with an SGPR operand
BITOP3 = (5.2, 4.05, 2.93, 2.33)
PERMSWAP = (8.8, 8.3, 6.3, 5.1)
CNDMASK_VCC = (19.0, 16.0, 12.6, 10.7)
DUAL_OPS = {"v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_lshrrev_b32",
            "v_ashrrev_i32", "v_not_b32", "v_min_u16", "v_add_u16", "v_max_i16", "v_add_f32", "v_mov_b32"}
SINGLE_OPS = {"v_bfi_b32", "v_perm_b32", "v_or3_b32", "v_and_or_b32", "v_lshl_or_b32", "v_min3_u32", "v_lshlrev_b32",
              "v_min_u32", "v_cndmask_b32_e64"}
# forms measured for this census (profiles/r08_valu_microbench_forms.log), by mnemonic without its
# encoding suffix. v_cmp_*: the same for a 32- and a 64-bit compare, VCC or SGPR-pair destination,
# VGPR or SGPR operand.
CMP = (8.5, 4.25, 3.99, 2.95)
MEASURED = {
    "v_lshl_add_u64": (5.28, 4.52, 3.27, 2.64), "v_lshlrev_b64": (5.15, 4.45, 3.24, 2.62),
    "v_mad_u32_u24": (5.20, 4.46, 3.25, 2.62), "v_mul_u32_u24": (4.83, 4.35, 3.18, 2.59),
    "v_mul_i32_i24": (4.83, 4.35, 3.18, 2.59), "v_bfe_u32": (5.14, 4.45, 3.24, 2.62),
    "v_add3_u32": (5.20, 4.46, 3.25, 2.62), "v_xad_u32": (5.20, 4.46, 3.25, 2.62),
    "v_lshl_add_u32": (5.20, 4.46, 3.25, 2.62),
}


def form_cost(line):
    """(form name, cost tuple or None) of one VALU instruction line of the assembly"""
    m = re.match(r"^\s+(v_\w+)\s*(.*)$", line)
    ins, ops = m.group(1), m.group(2).split(";")[0]
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", ins)
    if ins in MEASURED or base in MEASURED:
        return ins if ins in MEASURED else base, MEASURED.get(ins, MEASURED.get(base))
    if ins.endswith("_sdwa"):
        return ins, None
    if re.match(r"v_cmp_\w+_[iuf]\d+$", base):
        return ins, CMP
    if ins.endswith("_dpp") or "row_" in ops or "quad_perm" in ops:
        return base + "_dpp", SINGLE
    if ins == "v_cndmask_b32_e32":
        return ins, CNDMASK_VCC
    if base in ("v_bitop3_b32", "v_fma_f32"):
        return base, BITOP3
    if base in ("v_permlane16_swap_b32", "v_permlane32_swap_b32"):
        return base, PERMSWAP
    if base.startswith("v_pk_"):
        return base, SINGLE
    if ins in SINGLE_OPS or base in SINGLE_OPS:
        return base if base in SINGLE_OPS else ins, SINGLE
    if base in DUAL_OPS:
        srcs = ops.split(",")[1:]
        if any(re.match(r"\s*(s\d+|s\[|vcc|exec|m0)", o) for o in srcs):
            return base + " (sgpr operand)", SINGLE
        return base, DUAL
    return ins, None


def drop_rep_fallback(src):
    """the generated source without the exact REP chains (taken only when a REP total is 0): the
    test and the branch stay (the asm comment keeps the emptied body from becoming a select)"""
    src = re.sub(r"(    if \(rep_any_zero\(acc_\)\) \{\n      acc_ = 0u;\n)(?:      acc_ = G_sm<REPSAT>.*\n)+",
                 r'\1      asm volatile("; exact REP chain left out");\n', src)
    # the carried butterfly over the last word (POLAR_REP_CARRY), taken on the same condition
    return re.sub(r"(#if POLAR_REP_CARRY\n    if \(rep_any_zero\(acc_\)\) \{\n)(?:      .*\n)+?(    \}\n#else\n)",
                  r'\1      asm volatile("; REP carry left out");\n\2', src)


def drop_unaligned_copy(src):
    """the per-mask kernel's source without the byte copy of an input that is not 16-byte aligned"""
    return re.sub(r"  if \(!al_\) \{.*?\n  \}\n", "", src, count=1, flags=re.S)


def mask_cycles(asm, waves=4):
    """per op class of the per-mask kernel: {class: {form: [count, cost or None]}}"""
    col = WAVES.index(waves)
    out = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, None]))
    cur, cls = False, "prologue"
    for line in asm.split("\n"):
        if re.match(r"^polar_sc_mask_kernel:", line):
            cur = True
            continue
        if not cur:
            continue
        if re.match(r"^\.Lfunc_end", line):
            break
        m = re.match(r"^\s*;@@ (.*)$", line)
        if m:
            cls = m.group(1).strip()
            continue
        if re.match(r"^\s+v_\w+", line):
            form, cost = form_cost(line)
            e = out[cls][form]
            e[0] += 1
            e[1] = cost[col] if cost else None
    return out


def cycles_census(src, waves=4, defines=(), no_rep_fallback=False):
    """cost-weighted census of a per-mask kernel source: (total priced cycles, priced VALU,
    {unpriced form: count}, per-class table)"""
    if no_rep_fallback:
        src = drop_rep_fallback(src)
    marked, _ = mark_mask_kernel(src)
    with tempfile.TemporaryDirectory() as tmp:
        table = mask_cycles(compile_asm(marked, tmp, ["-D" + d for d in defines]), waves)
    total, priced, unpriced = 0.0, 0, collections.Counter()
    for forms in table.values():
        for form, (n, c) in forms.items():
            if c is None:
                unpriced[form] += n
            else:
                total += n * c
                priced += n
    return total, priced, dict(unpriced), table


def print_cycles(name, waves, res):
    total, priced, unpriced, table = res
    print("%s: per-mask kernel at %d waves per SIMD: %d priced VALU, %.0f issue cycles per wave; unpriced VALU %d"
          % (name, waves, priced, total, sum(unpriced.values())))
    print("%-12s %7s %9s %6s  %s" % ("class", "VALU", "cycles", "%", "costliest forms (count x cycles)"))
    rows = []
    for cls, forms in table.items():
        cyc = sum(n * c for n, c in forms.values() if c is not None)
        top = sorted(((n * c, f, n, c) for f, (n, c) in forms.items() if c is not None), reverse=True)[:4]
        rows.append((cyc, cls, sum(n for n, _ in forms.values()), top))
    for cyc, cls, n, top in sorted(rows, reverse=True):
        print("%-12s %7d %9.0f %5.1f%%  %s" % (cls, n, cyc, 100.0 * cyc / max(total, 1.0),
                                               ", ".join("%s %d x %.2f" % (f, k, c) for _, f, k, c in top)))
    for f, n in sorted(unpriced.items(), key=lambda kv: -kv[1]):
        print("unpriced     %7d            %s" % (n, f))


OPLINE = re.compile(r"^(\s*)(?:u32 x\d+_;\n\s*)?\{ // (.*)$|^(\s*)const u32 (x\d+_) = .*// (H0? n \d)$")


def classify(label):
    """op class from a generated op comment"""
    m = re.match(r"(F\+leaf|G\+leaf|REP|SPC|R1|H0|H|F|G) n (\d+)", label)
    if m:
        kind, n = m.group(1), int(m.group(2))
        if kind == "H0":
            kind = "H"
        return "%s n%s" % (kind, n if n < 8 else "8+" if n < 64 else "64+")
    m = re.match(r"([FG])\+leaf", label)
    if m:
        return "leaf"
    return label.split()[0]


def mark_mask_kernel(src):
    """the per-mask kernel (N <= 1024): markers before every op block of polar_sc_mask_kernel"""
    out, n, inside = [], 0, False
    for line in src.split("\n"):
        if "polar_sc_mask_kernel(" in line:
            inside = True
        m = re.match(r"^  \{ // (\S+)(?: level \d+)? n (\d+)", line) or re.match(r"^  \{ // ([FG]\+leaf)", line)
        if inside and line.startswith("  // END:"):   # the code after the last op: a class of its own
            out.append('  asm volatile(";@@ output"); __builtin_amdgcn_sched_barrier(0);')
            n += 1
        elif inside and m:
            if "leaf" in m.group(1):
                label = "leaf"
            else:
                kind, nn = m.group(1), int(m.group(2))
                label = "%s n%s" % ("H" if kind == "H0" else kind, nn if nn < 8 else "8+")
            out.append('  asm volatile(";@@ %s"); __builtin_amdgcn_sched_barrier(0);' % label)
            n += 1
        out.append(line)
    return "\n".join(out), n


def mask_census(asm):
    valu, allc = collections.Counter(), collections.Counter()
    cur, cls = False, "prologue"
    for line in asm.split("\n"):
        if re.match(r"^polar_sc_mask_kernel:", line):
            cur = True
            continue
        if not cur:
            continue
        if re.match(r"^\.Lfunc_end", line):
            break
        m = re.match(r"^\s*;@@ (.*)$", line)
        if m:
            cls = m.group(1).strip()
            continue
        m = re.match(r"^\s+([sv]_\w+|ds_\w+|global_\w+|buffer_\w+|scratch_\w+|flat_\w+)\b", line)
        if m:
            allc[cls] += 1
            if m.group(1).startswith("v_"):
                valu[cls] += 1
    return valu, allc


def mark(src):
    out, n = [], 0
    in_sub = False
    declared = []
    pending = []   # small-op results defined since the last marker: pinned before the next one
    def pin():
        for x in pending:
            out.append('  asm volatile("" :: "v"(%s));' % x)
        pending.clear()
    for line in src.split("\n"):
        if line.startswith("__device__") and "polar_psub_" in line:
            in_sub = True
        elif line.startswith("}") and in_sub:
            pin()
            out.append('  asm volatile(";@@ END"); __builtin_amdgcn_sched_barrier(0);')
            in_sub = False
        if in_sub:
            m = re.match(r"^\s*\{ // (.*)$", line) or re.match(r"^\s*const u32 x\d+_ = .*// (H0? n \d)\s*$", line)
            if m and not line.startswith("    "):
                label = m.group(1)
                if "leaf" in label:
                    label = label.split(" pos")[0]
                pin()
                pending.extend(declared)   # (declared before its own op's block: pinned after it)
                declared.clear()
                out.append('  asm volatile(";@@ %s"); __builtin_amdgcn_sched_barrier(0);' % classify(label))
                n += 1
        out.append(line)
        if in_sub:
            m = re.match(r"^\s*const u32 (x\d+_) =", line)
            if m:
                pending.append(m.group(1))
            m = re.match(r"^\s*u32 (x\d+_);", line)
            if m:
                declared.append(m.group(1))
    return "\n".join(out), n


def compile_asm(src, tmp, extra=()):
    path = os.path.join(tmp, "k.hip")
    with open(path, "w") as f:
        f.write("#include <hip/hip_runtime.h>\n" + src)
    s = os.path.join(tmp, "k.s")
    subprocess.run([CLANG, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-w",
                    "-I", CSRC, "-S", "-o", s, path] + list(extra), check=True)
    return open(s).read()


def census(asm):
    """per function: Counter(class -> VALU), Counter(class -> all instructions)"""
    funcs = {}
    cur, cls = None, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w*polar_psub_(\d+(?:_[FG])?(?:_L)?)\w*):", line)   # (_F / _G: fused roots; _L: CA2 leftmost)
        if m:
            cur = m.group(2)
            funcs[cur] = (collections.Counter(), collections.Counter())
            cls = "prologue"
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or re.match(r"^\.Lfunc_end", line):
            cur = None
            continue
        m = re.match(r"^\s*;@@ (.*)$", line)
        if m:
            cls = m.group(1).strip()
            continue
        m = re.match(r"^\s+([sv]_\w+|ds_\w+|global_\w+|buffer_\w+|scratch_\w+|flat_\w+)\b", line)
        if m:
            ins = m.group(1)
            valu, allc = funcs[cur]
            allc[cls] += 1
            if ins.startswith("v_"):
                valu[cls] += 1
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mask", default="frozen_n_262144_k_131072")
    ap.add_argument("--tuning", default="")
    ap.add_argument("--source", help="census of this generated source file instead of the plan's")
    ap.add_argument("--config", default="", help="polar_sc_config fields, e.g. sigmag=0,par=64")
    ap.add_argument("--cycles", action="store_true", help="per-mask kernel: VALU weighted by the issue cost of its form")
    ap.add_argument("--waves", type=int, default=4, choices=WAVES, help="waves per SIMD the costs are taken at")
    ap.add_argument("--no-rep-fallback", action="store_true", help="leave the exact REP fallback bodies out")
    ap.add_argument("--defines", default="", help="comma-separated macros for the compile, e.g. POLAR_PM1_MASK")
    args = ap.parse_args()
    import sc_polar_decoder_hls_amd as pkg
    import util
    tun = dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in args.tuning.split(",") if kv)
    cfg = None
    if args.config:
        cfg = pkg.default_config()
        for kv in args.config.split(","):
            setattr(cfg, kv.split("=")[0], int(kv.split("=")[1]))
    dec = pkg.Decoder(util.mask(args.mask), config=cfg, tuning=tun or None)
    src = open(args.source).read() if args.source else dec.kernel_source()
    defines = [d for d in args.defines.split(",") if d]
    if "polar_sc_mask_kernel(" in src and args.cycles:
        print_cycles(args.mask, args.waves, cycles_census(src, args.waves, defines, args.no_rep_fallback))
        return
    if "polar_sc_mask_kernel(" in src:   # per-mask kernel: one straight-line function
        if args.no_rep_fallback:
            src = drop_rep_fallback(src)
        marked, nmark = mark_mask_kernel(src)
        with tempfile.TemporaryDirectory() as tmp:
            tot_v, tot_a = mask_census(compile_asm(marked, tmp, ["-D" + d for d in defines]))
        nv = sum(tot_v.values())
        print("%s: per-mask kernel, %d op markers; VALU per wave %d, all instructions %d"
              % (args.mask, nmark, nv, sum(tot_a.values())))
        for c, v in sorted(tot_v.items(), key=lambda kv: -kv[1]):
            print("%-14s %10d %5.1f%% %10d" % (c, v, 100.0 * v / max(nv, 1), tot_a[c]))
        return
    calls = collections.Counter(re.findall(r"polar_psub_(\d+(?:_[FG])?(?:_L)?)\(c\.slot_ptr", src.split("polar_sc_pair_subtest_kernel")[0]))
    marked, nmark = mark(src)
    with tempfile.TemporaryDirectory() as tmp:
        asm = compile_asm(marked, tmp)
    funcs = census(asm)
    tot_v, tot_a = collections.Counter(), collections.Counter()
    for fid, (valu, allc) in funcs.items():
        k = calls.get(fid, 0)
        for c, v in valu.items():
            tot_v[c] += k * v
        for c, v in allc.items():
            tot_a[c] += k * v
    nv, na = sum(tot_v.values()), sum(tot_a.values())
    print("%s: %d subtree kinds, %d calls, %d op markers" % (args.mask, len(funcs), sum(calls.values()), nmark))
    print("dynamic-weighted (static count x calls) per decode: VALU %d, all instructions %d" % (nv, na))
    print("%-14s %10s %6s %10s" % ("class", "VALU", "%", "all"))
    for c, v in sorted(tot_v.items(), key=lambda kv: -kv[1]):
        print("%-14s %10d %5.1f%% %10d" % (c, v, 100.0 * v / max(nv, 1), tot_a[c]))


if __name__ == "__main__":
    main()
