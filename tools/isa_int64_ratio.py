#!/usr/bin/env python3
"""64-bit non-mad VALU instructions per v_mad_u64_u32 in the hot loops of a kernel, from gfx950 assembly.

The VALU fold kernels are bound by 64-bit issue slots: v_lshl_add_u64, v_lshrrev_b64 and v_mov_b64 run at
the mads' half rate, so each one the compiler adds beside the mads the source states is paid in time
(DESIGN.md §8 item 4). This tool compiles a .hip file to assembly (device only), cuts one kernel into
basic blocks and reports, for its innermost loop (the self-looping block with the most mads) and for the
straight-line code after it up to the enclosing loop's back edge (the peeled last limb block, with the
settle passes), the opcode counts, the ratio and the mads whose addend is the literal 0 (the mark of a
reassociated accumulation), plus the kernel's register and scratch figures from its metadata.

    tools/isa_int64_ratio.py [--src FILE.hip] [--kernel SUBSTRING] [--asm FILE.s]

tests/test_fold_sq_isa.py asserts on k_fold_sq with it. Tool, not product."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dependable-data-storage-csd2017_amd", "csrc")
MAD = "v_mad_u64_u32"
INT64_OTHER = ("v_lshl_add_u64", "v_lshrrev_b64", "v_mov_b64")


def find_hipcc():
    # the compiler csrc/Makefile builds with: $HIPCC, else hipcc on PATH, else under the Makefile's ROCM default
    rocm = os.environ.get("ROCM") or os.environ.get("ROCM_PATH")
    if not rocm:
        m = re.search(r"^ROCM\s*\?=\s*(\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M)
        rocm = m.group(1) if m else ""
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), os.path.join(rocm, "bin", "hipcc") if rocm else None):
        if cand and os.path.exists(cand):
            return cand
    return None


def compile_asm(src, out, hipcc=None, arch="gfx950"):
    """The flags of csrc/Makefile, device side only, assembly out."""
    hipcc = hipcc or find_hipcc()
    if not hipcc:
        raise FileNotFoundError("hipcc")
    cmd = [hipcc, f"--offload-arch={arch}", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
           "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, cwd=os.path.dirname(src), capture_output=True, text=True)
    return out


def kernel_symbol(text, sub):
    names = [m for m in re.findall(r"^(_Z\w+):", text, re.M) if sub in m]
    if len(names) > 1:  # k_fold_unit and k_fold_unit1: a whole identifier (length-prefixed when mangled) wins
        names = [m for m in names if f"{len(sub)}{sub}" in m] or names
    if len(names) != 1:
        raise ValueError(f"{len(names)} kernels match {sub!r}: {names}")
    return names[0]


def blocks_of(text, symbol):
    """[(label, [(opcode, operands)], branch target or None)]: cut at every label and after every branch."""
    body = text[text.index(symbol + ":"):]
    body = body[:body.index(".Lfunc_end")].split("\n")[1:]
    out, label, cur = [], "entry", []
    for line in body:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            out.append((label, cur, None))
            label, cur = m.group(1), []
            continue
        if not line.startswith("\t") or line.startswith("\t.") or line.startswith("\t;"):
            continue
        code = line.split(";")[0].strip()
        if not code:
            continue
        op, _, args = code.partition(" ")
        cur.append((op, args.strip()))
        if op.startswith("s_cbranch") or op == "s_branch":
            out.append((label, cur, args.strip()))
            label, cur = label + "+", []
    out.append((label, cur, None))
    return [b for b in out if b[1]]


def count(instrs):
    c = {MAD: 0, **{k: 0 for k in INT64_OTHER}}
    zero_addend = 0
    for op, args in instrs:
        base = re.sub(r"_e(32|64)$", "", op)
        if base in c:
            c[base] += 1
        if base == MAD and args.split(",")[-1].strip() == "0":
            zero_addend += 1
    other = sum(c[k] for k in INT64_OTHER)
    return {"instructions": len(instrs), **c, "int64_other": other,
            "int64_other_per_mad": round(other / c[MAD], 4) if c[MAD] else None, "mad_zero_addend": zero_addend}


def metadata(text, symbol):
    # the metadata entry of the kernel: the fields around its ".name:" line, up to the next "- ." entry
    chunks = re.split(r"\n  - ", text[text.index("amdhsa.kernels"):])
    mine = [c for c in chunks if re.search(r"\.name:\s+" + re.escape(symbol) + r"\s", c)]
    if len(mine) != 1:
        raise ValueError("kernel metadata not found")
    def field(name):
        return int(re.search(r"\." + name + r":\s+(\d+)", mine[0]).group(1))
    res = {k: field(k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                 "private_segment_fixed_size")}
    body = text[text.index(symbol + ":"):]
    m = re.search(r"; Occupancy: (\d+)", body)
    res["occupancy_waves_per_simd"] = int(m.group(1)) if m else None
    m = re.search(r"; ScratchSize: (\d+)", body)
    res["scratch_size"] = int(m.group(1)) if m else None
    return res


def analyse(text, kernel_sub):
    sym = kernel_symbol(text, kernel_sub)
    blocks = blocks_of(text, sym)
    loops = [i for i, (label, ins, target) in enumerate(blocks) if target == label.rstrip("+") and not label.endswith("+")]
    if not loops:
        raise ValueError("no single-block loop in " + sym)
    inner = max(loops, key=lambda i: count(blocks[i][1])[MAD])
    res = {"kernel": sym, "inner_loop": {"label": blocks[inner][0], **count(blocks[inner][1])}}
    # the straight-line code after the loop up to the next branch: the peeled last block of the row
    if inner + 1 < len(blocks) and blocks[inner + 1][0] == blocks[inner][0] + "+":
        res["after_loop"] = count(blocks[inner + 1][1])
    res["metadata"] = metadata(text, sym)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=os.path.join(CSRC, "ddshe_foldsq.hip"))
    ap.add_argument("--kernel", default="k_fold_sq")
    ap.add_argument("--asm", help="read this assembly file; do not compile")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            text = open(compile_asm(os.path.abspath(a.src), os.path.join(tmp, "kernel.s"))).read()
    print(json.dumps(analyse(text, a.kernel), indent=1))


if __name__ == "__main__":
    sys.exit(main())
