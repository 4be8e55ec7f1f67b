#!/usr/bin/env python3
"""Dependent-load chains of one kernel, read off its gfx950 ISA (needs no GPU).

Compiles one source of nnue-vision_amd/csrc with the flags of csrc/build.py plus `-S --cuda-device-only`, picks the kernel
whose demangled name contains SUBSTRING and prints, in program order and run-length compressed, what decides how many
memory round trips a workgroup pays one after the other: vector memory loads, `s_waitcnt vmcnt(N)`, LDS stores (the usual
first consumer of a staged load), branches and their labels, barriers and MFMA groups -- followed by the kernel's resource
usage.  `load xN; vmcnt(0); load xM` is two serial trips; `load xN; load xM; vmcnt(..)` is one.

  python tools/isa_chains.py ftm_kernels.hip 'ftm_forward_l1_kernel<32, 128'
  python tools/isa_chains.py --asm saved.s optim_kernels.hip sgd_apply_vec_kernel     # reuse a listing
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nnue-vision_amd" / "csrc"

RESOURCE_KEYS = ("NumVgprs", "NumAgprs", "TotalNumVgprs", "TotalNumSgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def build_flags():
    spec = importlib.util.spec_from_file_location("nnue_csrc_build", CSRC / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FLAGS, os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_asm(source: str, out: Path) -> None:
    flags, hipcc = build_flags()
    subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", str(CSRC / source), "-o", str(out)], check=True)


def demangle(names):
    if not names:
        return []
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if tool is None:
        return list(names)  # match against the mangled names
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return res.stdout.splitlines()


def kernels(text: str):
    """{mangled name: (body lines, resource dict)} of every kernel (.amdhsa_kernel) in a listing"""
    lines = text.splitlines()
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        res = {}
        for ln in lines[end:end + 60]:
            m = re.match(r";\s*(\w+):\s*(\d+)", ln)
            if m and m.group(1) in RESOURCE_KEYS and m.group(1) not in res:
                res[m.group(1)] = int(m.group(2))
        out[name] = (lines[start + 1:end], res)
    return out


def classify(ln: str):
    ln = ln.split(";")[0].strip()
    if not ln:
        return None
    if re.match(r"\.LBB\d+_\d+:", ln):
        return ("label", ln[:-1])
    op = ln.split()[0]
    if re.match(r"(global|buffer|flat|scratch)_load_", op):
        return ("run", op)
    if op == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", ln)
        return ("one", f"s_waitcnt vmcnt({m.group(1)})") if m else None
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return ("run", "ds_write")
    if op.startswith("v_mfma"):
        return ("run", op)
    if op == "s_barrier":
        return ("one", "s_barrier")
    if op.startswith("s_cbranch") or op == "s_branch":
        return ("one", ln)
    if op == "s_endpgm":
        return ("one", "s_endpgm")
    return None


def chains(body):
    out, last, count = [], None, 0

    def flush():
        nonlocal last, count
        if last is not None:
            out.append(f"  {last} x{count}" if count > 1 else f"  {last}")
        last, count = None, 0

    for ln in body:
        ev = classify(ln)
        if ev is None:
            continue
        kind, what = ev
        if kind == "run" and what == last:
            count += 1
            continue
        flush()
        if kind == "label":
            out.append(f"{what}:")
        elif kind == "run":
            last, count = what, 1
        else:
            out.append(f"  {what}")
    flush()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="file name under nnue-vision_amd/csrc, e.g. ftm_kernels.hip")
    ap.add_argument("substring", help="substring of the demangled kernel name; every match is printed")
    ap.add_argument("--asm", help="an existing listing of that source (skips the compile)")
    args = ap.parse_args()
    if args.asm:
        text = Path(args.asm).read_text()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            asm = Path(tmp) / "out.s"
            compile_asm(args.source, asm)
            text = asm.read_text()
    ks = kernels(text)
    mangled = sorted(ks)
    hits = [(m, d) for m, d in zip(mangled, demangle(mangled)) if args.substring in d]
    if not hits:
        print(f"no kernel of {args.source} matches {args.substring!r}", file=sys.stderr)
        return 1
    for m, d in hits:
        body, res = ks[m]
        print(f"== {args.source}: {d}")
        print("   " + "  ".join(f"{k}={res[k]}" for k in RESOURCE_KEYS if k in res))
        print("\n".join(chains(body)))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
