#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc --cuda-device-only -S) kernel by kernel: whether the instruction streams
are identical, the register and scratch numbers of both, and any difference in the multiset of mnemonics. Kernels are
paired by name and template arguments (the parameter list is ignored, so a renamed argument struct still pairs);
--map OLD=NEW pairs a kernel of file A with a differently named one of file B (several OLD may map to one NEW);
OLD=NEW+ARGS also appends ARGS to the template arguments (k<4> -> n<4, true> is --map k=n+true).
Mnemonics are classed by prefix only: float = v_* on a float type, mem = global_/ds_/flat_/buffer_/scratch_*, the rest
is v_* (integer / move / cross-lane) and s_* (scalar).
Usage: python tools/isa_diff.py A.s B.s [--map OLD=NEW ...] [--only REGEX]"""
import argparse
import collections
import re
import shutil
import subprocess

MEM = ("global_", "ds_", "flat_", "buffer_", "scratch_")
FLOAT_TYPES = ("_f16", "_f32", "_f64", "_bf16")
STATS = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def key_of(demangled):
    """`void ns::(anonymous namespace)::k<4, false>(int const*, ...)` -> `k<4, false>`."""
    m = re.search(r"(\w+(?:<[^()]*>)?)\(", demangled.replace("(anonymous namespace)::", ""))
    return m.group(1) if m else demangled


def klass(mn):
    if mn.startswith(MEM):
        return "mem"
    if mn.startswith("v_"):
        return "float" if any(t in mn for t in FLOAT_TYPES) else "v"
    return "s" if mn.startswith("s_") else "other"


def parse(path):
    kernels, cur, last = {}, None, None
    for line in open(path):
        m = re.match(r"^(\w+):\s*; @\1", line)
        if m:
            cur = last = m.group(1)
            kernels[cur] = {"text": [], "mn": collections.Counter(), "fseq": [], "stats": {}}
            continue
        if cur and line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and last and m.group(1) in STATS:
            kernels[last]["stats"].setdefault(m.group(1), int(m.group(2)))
            continue
        if cur and line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            ins = line.split(";")[0].strip()
            if ins:
                kernels[cur]["text"].append(re.sub(r"\.LBB\d+_", ".LBB_", ins))
                kernels[cur]["mn"][ins.split()[0]] += 1
                if klass(ins.split()[0]) == "float":  # order and modifiers of the float instructions, registers blanked
                    kernels[cur]["fseq"].append(re.sub(r"\b[vs]\d+\b|\b[vs]\[\d+:\d+\]", "r", ins))
    names = demangle(list(kernels))
    return {key_of(names[k]): v for k, v in kernels.items() if "ScratchSize" in v["stats"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    ka, kb = parse(args.a), parse(args.b)
    rename = dict(m.split("=") for m in args.map)
    n_same = n_diff_sched = n_diff_fm = 0
    seen = set()
    for name in sorted(ka):
        base, targs = (name.split("<", 1) + [""])[:2]
        new, _, extra = rename.get(base, base).partition("+")
        other = new + ("<" + (targs[:-1] + ", " + extra + ">" if extra else targs) if targs else "")
        seen.add(other)
        if args.only and not re.search(args.only, name):
            continue
        if other not in kb:
            print(f"{name}: only in A")
            continue
        a, b = ka[name], kb[other]
        same = a["text"] == b["text"]
        delta = {mn: b["mn"][mn] - a["mn"][mn] for mn in set(a["mn"]) | set(b["mn"]) if a["mn"][mn] != b["mn"][mn]}
        fm = {mn: d for mn, d in delta.items() if klass(mn) in ("float", "mem")}
        verdict = "identical" if same else (
            "float+mem multiset DIFFERS" if fm else "float+mem multiset same, stream differs")
        if not same and not fm:
            verdict += " (float instructions in the same order)" if a["fseq"] == b["fseq"] else " (float order differs)"
        n_same += same
        n_diff_sched += (not same and not fm)
        n_diff_fm += bool(fm)
        st = "  ".join(f"{k} {a['stats'].get(k, '-')}/{b['stats'].get(k, '-')}" for k in STATS)
        label = name if other == name else f"{name} -> {other}"
        print(f"{label}: {verdict}   [A/B] {st}   instructions {len(a['text'])}/{len(b['text'])}")
        for cls in ("float", "mem", "v", "s", "other"):
            d = sorted((mn, v) for mn, v in delta.items() if klass(mn) == cls)
            if d:
                print(f"    {cls:5s} " + "  ".join(f"{mn} {v:+d}" for mn, v in d))
    for name in sorted(set(kb) - seen):
        if not args.only or re.search(args.only, name):
            print(f"{name}: only in B")
    print(f"summary: {n_same} identical, {n_diff_sched} same float+mem multiset with another stream, "
          f"{n_diff_fm} with another float+mem multiset")


if __name__ == "__main__":
    main()
