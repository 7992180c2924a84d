#!/usr/bin/env python
"""tools/absgrad_ab.py -- what the absolute screen-space gradients (pipe.absgrad) cost a training frame, and that a frame which does not ask
pays nothing.  Three sections of profiles/absgrad_ab.json:

no_regression (with --parent-tree DIR: a built checkout of the parent commit): `python bench.py --gpus 1 --no-cpu-baseline` (BASELINE config 4;
bench.py does not ask) in DIR and in this tree, alternating in one job, --runs times each (>= 3).  Both ranges are recorded, and whether this
tree's median lies inside the spread of the parent's own runs (or above it).

cost: within this build, on config 4 (dynerf_default, 300 k Gaussians, 1352 x 1014) with the bench's cube scene and with the shell scene
(synthetic.make_gaussians(scene="shell"): most rows live), a training frame -- fdgs.render of the live model and the backward of its image
under a fixed random gradient image -- with the option off and on: the HIP-event median per frame over --frames frames after --warmup, in
--rounds rounds that alternate the legs, and the library's own times (fdgs_timing_report) of the blending backward and of the chain-rule
kernel.  The cost is what it is; nothing here is a pass or fail condition.

resources: registers, LDS and scratch of every instantiation of the two blending-backward kernels and of the chain-rule kernel, from the
build's resource remarks, with the waves per SIMD the register count allows (512 registers per lane and SIMD, allocated in eights, at most 8).

Every measurement is a child process of its own under `timeout` (a step that hangs ends there and nothing is started after a step that
failed); this process never opens the device.  Sections measured by one call replace those sections of the file, the others stay.  (GPU)"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 300
ROWS = ("render_bwd", "preprocess_bwd")
N, W, H, DCFG = 300_000, 1352, 1014, "dynerf_default"


def measure(scene, frames, warmup, rounds):
    import numpy as np
    import torch
    from playback_timing import kernel_table, row, timed

    fdgs = importlib.import_module("4dgaussians_amd")
    syn = fdgs.synthetic
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(N, DCFG, seed=6666, device=dev, scene=scene)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    off, on, bg = syn.PipelineParams(), syn.PipelineParams(), torch.zeros(3, device=dev)
    on.absgrad = True
    total = warmup + frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    cams = [syn.make_camera(W, H, float(th), float(k % 8) / 7.0).to(dev) for k, th in enumerate(thetas)]
    grad = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    last = {}

    def train(cam, pipe):
        for q in pc.parameters():
            q.grad = None
        res = fdgs.render(cam, pc, pipe, bg, stage="fine")
        res["render"].backward(grad)
        last["vsp"] = res["viewspace_points"]

    legs = {"train": [lambda c=c: train(c, off) for c in cams], "train_absgrad": [lambda c=c: train(c, on) for c in cams]}
    doc = {"N": N, "W": W, "H": H, "deformation": DCFG, "scene": scene, "frames": frames, "warmup": warmup,
           "device": torch.cuda.get_device_name(0), "rounds": []}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        leg["train_absgrad_over_train"] = round(leg["train_absgrad"]["median_ms"] / leg["train"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[absgrad_ab] {scene} round {r}: training frame {leg['train']['median_ms']:.4f} -> {leg['train_absgrad']['median_ms']:.4f} ms "
              f"(x{leg['train_absgrad_over_train']})", flush=True)
    # the statistic of the last frame: how much larger than the signed one it is on the rows that have one
    vsp = last["vsp"]
    a, s = vsp.absgrad[:, :2].norm(dim=1), vsp.grad[:, :2].norm(dim=1)
    live = a > 0
    doc["last_frame"] = {"rows_with_a_nonzero_absolute_sum": int(live.sum()), "median_abs_over_signed": float((a[live] / s[live].clamp_min(1e-30)).median()),
                         "share_with_abs_at_least_10x_signed": float((a[live] >= 10 * s[live]).float().mean())}
    doc["kernels"] = {}
    for k, calls in legs.items():
        timed_calls = calls[warmup:]
        table = kernel_table(lambda: [f() for f in timed_calls])
        doc["kernels"][k] = {n: {"launches_per_frame": round(v["launches"] / len(timed_calls), 3),
                                 "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5)} for n, v in table.items() if n in ROWS}
    print(f"[absgrad_ab] {scene} kernels: {json.dumps(doc['kernels'])}; last frame: {json.dumps(doc['last_frame'])}", flush=True)
    return doc


def _child(cmd, cwd=None):
    """One measurement in a process of its own under a time limit -> (exit status, its standard output)."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S)] + cmd, cwd=cwd, stdout=subprocess.PIPE, text=True)
    return p.returncode, p.stdout


def _bench(tree):
    rc, out = _child([sys.executable, "bench.py", "--gpus", "1", "--no-cpu-baseline"], cwd=tree)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    return rc, (json.loads(lines[-1]) if rc == 0 and lines else None)


def no_regression(parent_tree, runs):
    trees = (("parent", os.path.abspath(parent_tree)), ("change", ROOT))
    doc = {"what": "`python bench.py --gpus 1 --no-cpu-baseline` (frames/s, higher is better) in a checkout of the parent commit and in this "
                   "tree (bench.py does not ask for absgrad), same machine, one job, alternating",
           "headline_frames_per_s": {"parent": [], "change": []}, "ms_per_step": {"parent": [], "change": []}}
    for i in range(runs):
        for who, tree in trees:
            rc, res = _bench(tree)
            if res is None:
                print(f"[absgrad_ab] bench.py in the {who} tree: exit status {rc}; stopping", flush=True)
                return None, rc or 1
            doc["headline_frames_per_s"][who].append(round(res["value"], 2))
            doc["ms_per_step"][who].append(round(res["ms_per_step"], 4))
            print(f"[absgrad_ab] run {i} {who}: {res['value']:.1f} frames/s ({res['ms_per_step']:.4f} ms per step)", flush=True)
    h = doc["headline_frames_per_s"]
    doc["parent_range"], doc["change_range"] = [min(h["parent"]), max(h["parent"])], [min(h["change"]), max(h["change"])]
    doc["change_median"], doc["parent_median"] = round(statistics.median(h["change"]), 2), round(statistics.median(h["parent"]), 2)
    doc["change_median_not_below_parent_range"] = doc["change_median"] >= doc["parent_range"][0]
    print(f"[absgrad_ab] no regression: parent {doc['parent_range']} frames/s, change {doc['change_range']} (median {doc['change_median']}): "
          f"{'inside or above' if doc['change_median_not_below_parent_range'] else 'BELOW'} the parent's range", flush=True)
    return doc, 0


def resources():
    out = {}
    for unit, keys in (("render", ("render_bwd_kernel", "render_bwd_strip_kernel")), ("preprocess", ("preprocess_bwd_kernel",))):
        path = os.path.join(ROOT, "4dgaussians_amd", "build", unit + ".resources.txt")
        if not os.path.exists(path):      # (written by the build that compiled the unit)
            continue
        for line in open(path):
            if any(k in line for k in keys):
                rec = dict(kv.split("=") for kv in line.split()[1:])
                if rec.get("vgprs", "?").isdigit():
                    rec["waves_per_simd_by_registers"] = min(8, 512 // ((int(rec["vgprs"]) + 7) // 8 * 8))
                out[line.split()[0]] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absgrad_ab.json"))
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sections", default="cost", help="comma-separated: cost, no_regression (the latter needs --parent-tree)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (section no_regression)")
    ap.add_argument("--runs", type=int, default=3, help="bench.py runs per tree of section no_regression (>= 3)")
    ap.add_argument("--scene", default=None, help="(internal) measure this one scene in this process and write its record to --out")
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames: at least 30")
    if args.scene is not None:
        with open(args.out, "w") as f:
            json.dump(measure(args.scene, args.frames, args.warmup, args.rounds), f)
        return 0
    sections = [s for s in args.sections.split(",") if s]
    if "no_regression" in sections and (args.parent_tree is None or args.runs < 3):
        ap.error("section no_regression: --parent-tree DIR and --runs >= 3")
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["what"] = ("no_regression: bench.py of the parent commit against this tree, alternating.  cost: a training frame (fdgs.render + backward) "
                   "of config 4 on the cube and the shell scene with pipe.absgrad off and on, same process per scene, HIP-event median per "
                   "frame, and the library's kernel times.  resources: registers, LDS and scratch of the blending-backward and chain-rule "
                   "kernels from the build's resource remarks; tools/absgrad_ab.py")
    if "no_regression" in sections:
        rec, rc = no_regression(args.parent_tree, args.runs)
        if rec is None:
            return rc
        doc["no_regression"] = rec
    if "cost" in sections:
        cost = {}
        with tempfile.TemporaryDirectory() as tmp:
            for scene in ("cube", "shell"):
                part = os.path.join(tmp, scene + ".json")
                rc, out = _child([sys.executable, os.path.abspath(__file__), "--scene", scene, "--out", part, "--frames", str(args.frames),
                                  "--warmup", str(args.warmup), "--rounds", str(args.rounds)])
                sys.stdout.write(out)
                if rc != 0:          # a failed or hung step: nothing more is started on the device
                    print(f"[absgrad_ab] {scene}: exit status {rc}; stopping", flush=True)
                    return rc
                with open(part) as f:
                    cost["cfg4_" + scene] = json.load(f)
        doc["cost"] = cost
    res = resources()
    if res:
        doc["resources"] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
