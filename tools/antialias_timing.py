#!/usr/bin/env python
"""tools/antialias_timing.py -- what the opacity compensation (pipe.antialiasing) costs a frame, and that a frame which does not ask pays nothing.

Cost of asking (section "cost"), on BASELINE configs 4 and 2:

    cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014          cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800

The model is the bench's (SynthModel, seed 6666, Hilbert order), the cameras are the video orbit.  Per configuration, as medians of HIP-event
times over --frames frames (>= 30) after --warmup frames, one event pair per frame, in --rounds rounds that alternate the legs:

    train / train_aa         fdgs.render of the live model and the backward of its image under a fixed random gradient image, switch off / on
    playback / playback_aa   Baked.render of the model baked at eight timestamps, switch off / on

with the pair count of the last frame of each leg (it can only fall with the switch on: h <= 1 tightens the cull ellipse) and the library's
own per-kernel times (fdgs_timing_report) of the projection, the chain rule and the two blending kernels.  Nothing here is a pass or fail
condition.

No regression for frames that do not ask (section "no_regression", with --parent-tree DIR: a built checkout of the parent commit):
`python bench.py --gpus 1` in DIR and in this tree, alternating, --runs times each (>= 3); both ranges are recorded, and whether this tree's
median lies inside the parent's own run-to-run range (or above it).

Every measurement is a child process of its own under `timeout` (a step that hangs ends there and nothing is started after a step that
failed); this process never opens the device.  Sections measured by one call replace those sections of profiles/antialias_timing.json, the
others stay.  (GPU)"""
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
ROWS = ("preprocess_fwd", "preprocess_bwd", "render_fwd", "render_bwd")
T_BAKED = 8


def measure(name, frames, warmup, rounds):
    import numpy as np
    import torch
    from playback_timing import CONFIGS, kernel_table, row, timed

    fdgs = importlib.import_module("4dgaussians_amd")
    syn, P, R = fdgs.synthetic, fdgs.playback, fdgs.rasterizer
    N, W, H, dcfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(N, dcfg, seed=6666, device=dev)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    off, on, bg = syn.PipelineParams(), syn.PipelineParams(), torch.zeros(3, device=dev)
    on.antialiasing = True
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    total = warmup + frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    cams = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    grad = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    baked = P.bake(pc, times)

    def train(cam, pipe):
        for q in pc.parameters():
            q.grad = None
        fdgs.render(cam, pc, pipe, bg, stage="fine")["render"].backward(grad)

    legs = {"train": [lambda c=c: train(c, off) for c in cams], "train_aa": [lambda c=c: train(c, on) for c in cams],
            "playback": [lambda c=c: baked.render(c, off, bg) for c in cams], "playback_aa": [lambda c=c: baked.render(c, on, bg) for c in cams]}
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "frames": frames, "warmup": warmup, "device": torch.cuda.get_device_name(0), "rounds": []}
    for r in range(rounds):
        leg = {}
        for k, calls in legs.items():
            leg[k] = row(*timed(calls, warmup))
            torch.cuda.synchronize()
            leg[k]["pairs_last_frame"] = R.last_num_rendered()
        leg["train_aa_over_train"] = round(leg["train_aa"]["median_ms"] / leg["train"]["median_ms"], 4)
        leg["playback_aa_over_playback"] = round(leg["playback_aa"]["median_ms"] / leg["playback"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[antialias_timing] {name} round {r}: training frame {leg['train']['median_ms']:.4f} -> {leg['train_aa']['median_ms']:.4f} ms "
              f"(x{leg['train_aa_over_train']}), playback frame {leg['playback']['median_ms']:.4f} -> {leg['playback_aa']['median_ms']:.4f} ms "
              f"(x{leg['playback_aa_over_playback']}); pairs {leg['train']['pairs_last_frame']} -> {leg['train_aa']['pairs_last_frame']}", flush=True)
    with torch.no_grad():
        a, b = baked.render(cams[-1], on, bg)["render"], baked.render(cams[-1], off, bg)["render"]
        doc["image_mean_abs_difference_on_vs_off"] = float((a - b).abs().mean())
    doc["kernels"] = {}
    for k in ("train", "train_aa"):
        timed_calls = legs[k][warmup:]
        table = kernel_table(lambda: [f() for f in timed_calls])
        doc["kernels"][k] = {n: {"launches_per_frame": round(v["launches"] / len(timed_calls), 3),
                                 "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5)} for n, v in table.items() if n in ROWS}
    print(f"[antialias_timing] {name} kernels: {json.dumps(doc['kernels'])}", flush=True)
    return doc


def _child(cmd, cwd=None):
    """One measurement in a process of its own under a time limit -> (exit status, its standard output)."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S)] + cmd, cwd=cwd, stdout=subprocess.PIPE, text=True)
    return p.returncode, p.stdout


def _bench(tree):
    rc, out = _child([sys.executable, "bench.py", "--gpus", "1"], cwd=tree)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    return rc, (json.loads(lines[-1]) if rc == 0 and lines else None)


def no_regression(parent_tree, runs):
    trees = (("parent", os.path.abspath(parent_tree)), ("change", ROOT))
    doc = {"what": "`python bench.py --gpus 1` (frames/s, higher is better) in a checkout of the parent commit and in this tree (switch off: "
                   "bench.py does not ask), same machine, one session, alternating",
           "headline_frames_per_s": {"parent": [], "change": []}, "ms_per_step": {"parent": [], "change": []}}
    for i in range(runs):
        for who, tree in trees:
            rc, res = _bench(tree)
            if res is None:
                print(f"[antialias_timing] bench.py in the {who} tree: exit status {rc}; stopping", flush=True)
                return None, rc or 1
            doc["headline_frames_per_s"][who].append(round(res["value"], 2))
            doc["ms_per_step"][who].append(round(res["ms_per_step"], 4))
            print(f"[antialias_timing] run {i} {who}: {res['value']:.1f} frames/s ({res['ms_per_step']:.4f} ms per step)", flush=True)
    h = doc["headline_frames_per_s"]
    doc["parent_range"], doc["change_range"] = [min(h["parent"]), max(h["parent"])], [min(h["change"]), max(h["change"])]
    doc["change_median"], doc["parent_median"] = round(statistics.median(h["change"]), 2), round(statistics.median(h["parent"]), 2)
    doc["change_median_not_below_parent_range"] = doc["change_median"] >= doc["parent_range"][0]
    print(f"[antialias_timing] no regression: parent {doc['parent_range']} frames/s, change {doc['change_range']} (median {doc['change_median']}): "
          f"{'inside or above' if doc['change_median_not_below_parent_range'] else 'BELOW'} the parent's range", flush=True)
    return doc, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "antialias_timing.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sections", default="cost", help="comma-separated: cost, no_regression (the latter needs --parent-tree)")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (section no_regression)")
    ap.add_argument("--runs", type=int, default=3, help="bench.py runs per tree of section no_regression (>= 3)")
    ap.add_argument("--config", default=None, help="(internal) measure this one configuration in this process and write its record to --out")
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames: at least 30")
    if args.config is not None:
        with open(args.out, "w") as f:
            json.dump(measure(args.config, args.frames, args.warmup, args.rounds), f)
        return 0
    sections = [s for s in args.sections.split(",") if s]
    if "no_regression" in sections and (args.parent_tree is None or args.runs < 3):
        ap.error("section no_regression: --parent-tree DIR and --runs >= 3")
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["what"] = ("cost: a training frame (fdgs.render + backward) and a playback frame (Baked.render) with pipe.antialiasing off and on, same "
                   "process per configuration, HIP-event median per frame, pair counts.  no_regression: bench.py of the parent commit against "
                   "this tree.  resources: registers and scratch of the kernels that gained an antialiased instantiation, from the build's "
                   "resource remarks; tools/antialias_timing.py")
    if "cost" in sections:
        cost = {}
        with tempfile.TemporaryDirectory() as tmp:
            for name in ("cfg4_dynerf_300k_1352x1014", "cfg2_dnerf_100k_800x800"):
                part = os.path.join(tmp, name + ".json")
                rc, out = _child([sys.executable, os.path.abspath(__file__), "--config", name, "--out", part, "--frames", str(args.frames),
                                  "--warmup", str(args.warmup), "--rounds", str(args.rounds)])
                sys.stdout.write(out)
                if rc != 0:          # a failed or hung step: nothing more is started on the device
                    print(f"[antialias_timing] {name}: exit status {rc}; stopping", flush=True)
                    return rc
                with open(part) as f:
                    cost[name] = json.load(f)
        doc["cost"] = cost
    if "no_regression" in sections:
        rec, rc = no_regression(args.parent_tree, args.runs)
        if rec is None:
            return rc
        doc["no_regression"] = rec
    res = os.path.join(ROOT, "4dgaussians_amd", "build", "preprocess.resources.txt")
    if os.path.exists(res):      # (written by the build that compiled preprocess.hip)
        doc["resources"] = {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in open(res)
                            if any(k in l for k in ("preprocess_fwd_kernel", "preprocess_bwd_kernel", "camera_grad_partial_kernel"))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
