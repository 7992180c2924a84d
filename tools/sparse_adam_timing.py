#!/usr/bin/env python
"""tools/sparse_adam_timing.py -- what an optimizer step costs when only the visible rows are stepped (fdgs.SparseGaussianAdam).

Section "timing" -> profiles/sparse_adam_timing.json.  The parameter set of BASELINE config 4 (SynthModel: 300 k rows of the six per-Gaussian
tensors, 59 floats per row, plus the dynerf_default deformation MLP and HexPlane grid tensors), random gradients, medians over --steps steps
(>= 30) after --warmup steps, per leg:

    a  FusedAdam.step()                                  (fdgs_adam_step; with --parent-tree DIR also the parent commit's, in a process of its own)
    b  SparseGaussianAdam.step(mask, N), all rows visible
    c  ... 12 % visible in contiguous runs of 32 rows    (what a frame marks in the spatial order the library keeps)
    d  ... 12 % visible at random rows
    e  ... no row visible

For each leg: the HIP-event time of a whole step() (host work included: the device idles while Python builds the descriptors), the
library's own time of the launch (fdgs_timing_report: "adam_step" / "adam_step_rows"), and the bytes the launch should move -- 28 B per
element of every float4 that has a visible row, 1 B per mask byte, and the same counted in whole 128-byte lines -- with the time those
bytes take at the 6.3 TB/s HBM roof.  b against a is what reading the mask costs, c against d what the row order is worth.  Nothing here
is a pass or fail condition.

Section "ab" (with --parent-tree DIR, a built checkout of the parent commit) -> profiles/sparse_adam_ab.json: `python bench.py --gpus 1` in
DIR and in this tree, alternating, --runs times each (>= 3); both ranges are recorded, and whether this tree's median lies below the
parent's lowest run (DESIGN 7.13's rule).  bench.py calls none of the new code.

Every measurement is a child process of its own under `timeout` (a step that hangs ends there and nothing is started after a step that
failed); this process never opens the device.  (GPU)"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 300
HBM_ROOF_TBPS = 6.3
N_ROWS, DEFORM = 300_000, "dynerf_default"
ROW_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LEGS = ("a", "b", "c", "d", "e")


def _masks(torch, N, dev):
    gen = torch.Generator().manual_seed(5)
    runs = torch.zeros((N + 31) // 32, dtype=torch.bool)
    runs[torch.randperm(runs.numel(), generator=gen)[:round(0.12 * runs.numel())]] = True
    rand = torch.zeros(N, dtype=torch.bool)
    rand[torch.randperm(N, generator=gen)[:int(runs.repeat_interleave(32)[:N].sum())]] = True
    return {"b": torch.ones(N, dtype=torch.bool, device=dev), "c": runs.repeat_interleave(32)[:N].contiguous().to(dev), "d": rand.to(dev),
            "e": torch.zeros(N, dtype=torch.bool, device=dev)}


def _bytes(torch, opt, mask):
    """Bytes the launch should move: per float4 with a visible row 4 x 28 B, per mask byte 1 B; and the same in whole 128-byte lines."""
    quad_bytes = line_bytes = elements = 0
    for group in opt.param_groups:
        for p in group["params"]:
            if p.grad is None:
                continue
            n = p.numel()
            elements += n
            if mask is None or group.get("name") not in ROW_GROUPS:
                quad_bytes += 28 * n
                line_bytes += 28 * n
                continue
            live = mask.repeat_interleave(n // mask.numel())
            pad = torch.zeros((-n) % 32, dtype=torch.bool, device=live.device)
            live = torch.cat([live, pad])
            quad_bytes += 28 * 4 * int(live.view(-1, 4).any(1).sum()) + mask.numel()
            line_bytes += 7 * 128 * int(live.view(-1, 32).any(1).sum()) + mask.numel()
    return elements, quad_bytes, line_bytes


def measure(tree, steps, warmup, legs):
    sys.path.insert(0, tree)
    import torch
    fdgs = importlib.import_module("4dgaussians_amd")
    L = fdgs._lib.lib()
    dev = torch.device("cuda:0")
    pc = fdgs.synthetic.SynthModel(N_ROWS, DEFORM, seed=6666, device=dev)
    gen = torch.Generator().manual_seed(1)
    for p in pc.parameters():
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
    masks = _masks(torch, N_ROWS, dev) if hasattr(fdgs, "SparseGaussianAdam") else {}
    doc = {"N": N_ROWS, "deformation": DEFORM, "steps": steps, "warmup": warmup, "device": torch.cuda.get_device_name(0), "legs": {}}
    buf = ctypes.create_string_buffer(1 << 16)
    for leg in legs:
        if leg != "a" and not masks:
            continue
        opt = (fdgs.FusedAdam if leg == "a" else fdgs.SparseGaussianAdam)(pc.optimizer_groups(lr=1e-6), lr=0.0, eps=1e-15)
        mask = masks.get(leg)
        step = (lambda: opt.step()) if leg == "a" else (lambda: opt.step(mask, N_ROWS))
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
        L.fdgs_timing_enable(1)
        try:
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
        finally:
            L.fdgs_timing_enable(0)
        table = {l.split()[0]: (int(l.split()[1]), float(l.split()[2])) for l in buf.value.decode().strip().splitlines()}
        launches, kernel_ms = table.get("adam_step" if leg == "a" else "adam_step_rows", (0, 0.0))
        elements, quad_bytes, line_bytes = _bytes(torch, opt, mask)
        rec = {"step_event_median_ms": round(statistics.median(ms), 4), "step_event_min_ms": round(min(ms), 4),
               "launches_per_step": round(launches / steps, 3), "kernel_ms_mean": round(kernel_ms / max(launches, 1), 5),
               "elements": elements, "visible_rows": None if mask is None else int(mask.sum()),
               "bytes_float4": quad_bytes, "bytes_128B_lines": line_bytes,
               "roof_ms_float4": round(quad_bytes / (HBM_ROOF_TBPS * 1e12) * 1e3, 5), "roof_ms_128B_lines": round(line_bytes / (HBM_ROOF_TBPS * 1e12) * 1e3, 5)}
        rec["kernel_over_roof_128B_lines"] = round(rec["kernel_ms_mean"] / rec["roof_ms_128B_lines"], 2) if rec["roof_ms_128B_lines"] > 0 else None
        doc["legs"][leg] = rec
        print(f"[sparse_adam_timing] leg {leg}: {json.dumps(rec)}", flush=True)
    return doc


def _child(cmd, cwd=None):
    """One measurement in a process of its own under a time limit -> (exit status, its standard output)."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S)] + cmd, cwd=cwd, stdout=subprocess.PIPE, text=True)
    return p.returncode, p.stdout


def _bench(tree):
    rc, out = _child([sys.executable, "bench.py", "--gpus", "1"], cwd=tree)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    return rc, (json.loads(lines[-1]) if rc == 0 and lines else None)


def ab(parent_tree, runs):
    trees = (("parent", os.path.abspath(parent_tree)), ("change", ROOT))
    doc = {"what": "`python bench.py --gpus 1` (frames/s, higher is better) in a checkout of the parent commit and in this tree (bench.py steps "
                   "FusedAdam: the dense instantiation of adam_kernel), same machine, one session, alternating; tools/sparse_adam_timing.py",
           "headline_frames_per_s": {"parent": [], "change": []}, "ms_per_step": {"parent": [], "change": []}}
    for i in range(runs):
        for who, tree in (trees if i % 2 == 0 else trees[::-1]):      # neither tree always runs behind the other
            rc, res = _bench(tree)
            if res is None:
                print(f"[sparse_adam_timing] bench.py in the {who} tree: exit status {rc}; stopping", flush=True)
                return None, rc or 1
            doc["headline_frames_per_s"][who].append(round(res["value"], 2))
            doc["ms_per_step"][who].append(round(res["ms_per_step"], 4))
            print(f"[sparse_adam_timing] run {i} {who}: {res['value']:.1f} frames/s ({res['ms_per_step']:.4f} ms per step)", flush=True)
    h = doc["headline_frames_per_s"]
    doc["parent_range"], doc["change_range"] = [min(h["parent"]), max(h["parent"])], [min(h["change"]), max(h["change"])]
    doc["change_median"], doc["parent_median"] = round(statistics.median(h["change"]), 2), round(statistics.median(h["parent"]), 2)
    doc["change_median_not_below_parent_lowest_run"] = doc["change_median"] >= doc["parent_range"][0]
    return doc, 0


def _write(path, doc):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_adam_timing.json"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "sparse_adam_ab.json"))
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sections", default="timing", help="comma-separated: timing, ab (the latter needs --parent-tree)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (leg a of the parent; section ab)")
    ap.add_argument("--runs", type=int, default=3, help="bench.py runs per tree of section ab (>= 3)")
    ap.add_argument("--tree", default=None, help="(internal) measure in this process, importing the package from this tree, and write to --out")
    ap.add_argument("--legs", default=",".join(LEGS), help="(internal) the legs of --tree")
    args = ap.parse_args()
    if args.steps < 30:
        ap.error("--steps: at least 30")
    if args.tree is not None:
        with open(args.out, "w") as f:
            json.dump(measure(args.tree, args.steps, args.warmup, [l for l in args.legs.split(",") if l]), f)
        return 0
    sections = [s for s in args.sections.split(",") if s]
    if "ab" in sections and (args.parent_tree is None or args.runs < 3):
        ap.error("section ab: --parent-tree DIR and --runs >= 3")
    if "timing" in sections:
        doc = {"what": "one optimizer step over the config 4 parameter set (300 k rows x 59 floats + the dynerf_default deformation and grid "
                       "tensors): FusedAdam (a) and SparseGaussianAdam with every row visible (b), 12 % visible in runs of 32 rows (c), 12 % "
                       "visible at random rows (d), no row visible (e); medians of HIP-event times per step(), the library's own time of "
                       "the launch, the bytes it should move and their time at 6.3 TB/s; tools/sparse_adam_timing.py"}
        with tempfile.TemporaryDirectory() as tmp:
            jobs = [("this_tree", ROOT, ",".join(LEGS))] + ([("parent_tree", os.path.abspath(args.parent_tree), "a")] if args.parent_tree else [])
            for name, tree, legs in jobs:
                part = os.path.join(tmp, name + ".json")
                rc, out = _child([sys.executable, os.path.abspath(__file__), "--tree", tree, "--legs", legs, "--out", part, "--steps", str(args.steps),
                                  "--warmup", str(args.warmup)])
                sys.stdout.write(out)
                if rc != 0:          # a failed or hung step: nothing more is started on the device
                    print(f"[sparse_adam_timing] {name}: exit status {rc}; stopping", flush=True)
                    return rc
                with open(part) as f:
                    doc[name] = json.load(f)
        res = os.path.join(ROOT, "4dgaussians_amd", "build", "adam.resources.txt")
        if os.path.exists(res):      # (written by the build that compiled adam.hip)
            doc["resources"] = {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in open(res) if l.strip()}
        _write(args.out, doc)
    if "ab" in sections:
        rec, rc = ab(args.parent_tree, args.runs)
        if rec is None:
            return rc
        _write(args.ab_out, rec)
    return 0


if __name__ == "__main__":
    sys.exit(main())
