#!/usr/bin/env python
"""tools/spatial_order_timing.py -- time of fdgs.densify.spatial_order (curve keys + stable argsort of the positions, with the aabb given) at
300 k and 2 M Gaussians, both curves: median of HIP-event times over --reps calls after --warmup calls, plus the launches of one call as the
library's own timing report counts them.

Run it twice, once as it is (the library's kernels) and once with FDGS_NATIVE_ORDER=0 (the torch expressions + torch.argsort, the path the
project used before): each run stores its leg ("native" / "torch") in the same JSON file (default profiles/spatial_order_timing.json), and
once both legs are there the file also says, per size and curve, whether the native median is at or below the torch one.  (GPU)"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fdgs = importlib.import_module("4dgaussians_amd")
D = fdgs.densify


def launches_of_one_call(fn):
    L = fdgs._lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    L.fdgs_timing_enable(1)
    try:
        fn()
        fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    finally:
        L.fdgs_timing_enable(0)
    return {l.split()[0]: {"launches": int(l.split()[1]), "ms": round(float(l.split()[2]), 4)} for l in buf.value.decode().strip().splitlines()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_order_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[300_000, 2_000_000])
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20")
    dev = torch.device("cuda:0")
    leg = "native" if D.NATIVE_ORDER else "torch"
    rows = {}
    for n in args.sizes:
        xyz = (torch.randn(n, 3, generator=torch.Generator().manual_seed(6666)) * 1.3).to(dev)
        hi, lo = torch.tensor([1.5, 1.4, 1.6], device=dev), torch.tensor([-1.5, -1.6, -1.4], device=dev)
        for curve in ("hilbert", "morton"):
            def call():
                return D.spatial_order(xyz, lo, hi, curve=curve)
            for _ in range(args.warmup):
                call()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            rows[f"{curve}_{n}"] = {"N": n, "curve": curve, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                                    "max_ms": round(max(ms), 4), "reps": args.reps, "warmup": args.warmup,
                                    "library_launches_per_call": launches_of_one_call(call)}
            print(f"[spatial_order_timing] {leg} {curve} N={n}: median {rows[f'{curve}_{n}']['median_ms']:.4f} ms "
                  f"(min {min(ms):.4f}, max {max(ms):.4f}, {args.reps} reps)", flush=True)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["what"] = "fdgs.densify.spatial_order(xyz, aabb), HIP-event time per call; legs: native = csrc/spatial.hip, torch = FDGS_NATIVE_ORDER=0"
    doc["device"] = torch.cuda.get_device_name(0)
    doc[leg] = rows
    if "native" in doc and "torch" in doc:
        doc["native_not_above_torch"] = {k: doc["native"][k]["median_ms"] <= doc["torch"][k]["median_ms"]
                                         for k in doc["native"] if k in doc["torch"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
