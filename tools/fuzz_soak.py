#!/usr/bin/env python3
"""One-off soak of tests/test_gpu_fuzz.py's differential fuzz beyond the seeds the suite pins (0..319): every seed in
[first, last) through run_case, failures collected (seed, kind, message) instead of stopping at the first.
Usage: python tools/fuzz_soak.py first last            (conv layers: run_case)
       python tools/fuzz_soak.py --models first last   (whole models: run_model_case)
       python tools/fuzz_soak.py --fused first last    (rgbx_fused_layer_f32 by option: run_fused_layer_case)
       python tools/fuzz_soak.py --ref64 seed [seed ...]   (the listed seeds against the oracle computing in float64)
       python tools/fuzz_soak.py --families first last [--kind NAME]   (tests/test_gpu_fuzz_families.py: run_family_case;
                                  with --kind every seed runs that kind, else a seed's kind is seed % 8; a HIP error ends the run)
       python tools/fuzz_soak.py --edge-families first last [--kind NAME]   (tests/test_gpu_fuzz_edge_families.py:
                                  run_edge_family_case; --kind and a HIP error as for --families, a seed's kind is seed % 9)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import test_gpu_fuzz as F
import test_gpu_fuzz_edge_families as EF
import test_gpu_fuzz_families as FF
from conftest import usable_cpus

torch.set_num_threads(min(torch.get_num_threads(), usable_cpus()))  # the oracle half: the cgroup's CPUs, not the host's


def is_hip_error(exc):
    """A failure of the runtime or of a launch (ops check(): 'hipError'; torch: 'HIP error'), not an argument the library
    refused on the host."""
    text = str(exc)
    return isinstance(exc, RuntimeError) and ("hipError" in text or "HIP error" in text or "CUDA error" in text)


def main():
    dev = torch.device("cuda")
    if sys.argv[1] == "--ref64":
        rc = 0
        for seed in map(int, sys.argv[2:]):
            for dtype in (torch.float32, torch.float64):
                try:
                    F.run_case(dev, seed, dtype)
                    print(f"seed {seed} vs the {dtype} oracle: within tolerance", flush=True)
                except AssertionError as exc:
                    print(f"seed {seed} vs the {dtype} oracle: {repr(exc)[:260]}", flush=True)
                    rc |= dtype == torch.float64
        return int(rc)
    which = sys.argv[1] if sys.argv[1].startswith("--") else ""
    if which:
        sys.argv.pop(1)
    family = None
    if "--kind" in sys.argv:
        at = sys.argv.index("--kind")
        family = sys.argv[at + 1]
        names = {"--families": FF.KINDS, "--edge-families": EF.KINDS}.get(which)
        if names is None or family not in names:
            sys.exit(f"--kind goes with --families ({FF.KINDS}) or --edge-families ({EF.KINDS}) and names one of its kinds")
        del sys.argv[at:at + 2]
    run, kinds = {"--models": (F.run_model_case, F.MODEL_KINDS), "--fused": (F.run_fused_layer_case, ["fused_layer"]),
                  "--families": (lambda d, seed: FF.run_family_case(d, seed, family), [family] if family else FF.KINDS),
                  "--edge-families": (lambda d, seed: EF.run_edge_family_case(d, seed, family),
                                      [family] if family else EF.KINDS),
                  "": (F.run_case, F.KINDS)}[which]
    by_family = which in ("--families", "--edge-families")
    first, last = int(sys.argv[1]), int(sys.argv[2])
    bad, t0, mark = [], time.time(), time.time()
    for seed in range(first, last):
        try:
            run(dev, seed)
        except Exception as exc:  # noqa: BLE001 - collected, reported below
            bad.append((seed, kinds[seed % len(kinds)], repr(exc)[:1200 if by_family else 300]))
            print("FAIL", bad[-1], flush=True)
            if by_family and is_hip_error(exc):  # the device is in an unknown state: nothing more runs on it
                print(f"soak [{first}, {seed}]: ended by a HIP error after {seed - first + 1} cases, {len(bad)} failures", flush=True)
                return 2
        if time.time() - mark > 30:
            mark = time.time()
            print(f"seed {seed} ({seed - first + 1} cases, {len(bad)} failures, {time.time() - t0:.0f} s)", flush=True)
    torch.cuda.synchronize()
    print(f"soak [{first}, {last}): {last - first} cases, {len(bad)} failures in {time.time() - t0:.0f} s", flush=True)
    for b in bad:
        print(b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
