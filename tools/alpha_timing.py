#!/usr/bin/env python
"""tools/alpha_timing.py -- what the accumulated-alpha image costs a training frame, and that a frame which does not ask pays nothing.

Cost of asking (section "cost"), on BASELINE configs 4 and 2:

    cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014          cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800

The model is the bench's (SynthModel, seed 6666, Hilbert order), the cameras are the video orbit.  Per configuration, as medians of HIP-event
times over --frames frames (>= 30) after --warmup frames, one event pair per frame, in --rounds rounds that alternate the three legs (reported
one by one: their difference is the run-to-run spread):

    train             fdgs.render of the live model and the backward of its image under a fixed random gradient image
    train_alpha       the same frame with pipe.render_alpha, the backward of image AND alpha under fixed random gradient images
    train_two_frames  the only route to a differentiable alpha without this feature: the frame, and a SECOND whole differentiable frame with
                      override_color = 1 over a black background whose first channel is alpha; one backward through both

with the two ratios train_alpha / train and train_two_frames / train, and the library's own per-kernel times (fdgs_timing_report) of
render_fwd and render_bwd over the frames of the first two legs.  Nothing here is a pass or fail condition.

No regression for frames that do not ask (section "no_regression", with --parent-tree DIR: a built checkout of the commit before the alpha
image): `python bench.py` in DIR and in this tree, alternating, --runs times each (>= 3), every headline figure recorded; then
`bench.py --full --no-cpu-baseline --no-extras` once in each for the per-kernel render_fwd / render_bwd times.  The rule the record states:
the change is accepted when the MEDIAN of its headline figures is not below the parent's LOWEST run.

Every measurement is a child process of its own under `timeout` (a step that hangs ends there and nothing is started after a step that
failed); this process never opens the device.  Sections measured by one call replace those sections of profiles/alpha_timing.json, the
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
ROWS = ("render_fwd", "render_bwd", "preprocess_bwd", "preprocess_fwd")


class _AlphaPipe:
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False
    render_alpha = True


def measure(name, frames, warmup, rounds):
    import numpy as np
    import torch
    from playback_timing import CONFIGS, kernel_table, row, timed

    fdgs = importlib.import_module("4dgaussians_amd")
    syn = fdgs.synthetic
    N, W, H, dcfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(N, dcfg, seed=6666, device=dev)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    total = warmup + frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    cams = [syn.make_camera(W, H, float(th), float(k % 32) / 31.0).to(dev) for k, th in enumerate(thetas)]
    gen = torch.Generator().manual_seed(3)
    grad = torch.randn(3, H, W, generator=gen).to(dev)
    grad_alpha = torch.randn(1, H, W, generator=gen).to(dev)
    ones = torch.ones(N, 3, device=dev)

    def clear():
        for q in pc.parameters():
            q.grad = None

    def train(cam):
        clear()
        fdgs.render(cam, pc, pipe, bg, stage="fine")["render"].backward(grad)

    def train_alpha(cam):
        clear()
        res = fdgs.render(cam, pc, _AlphaPipe(), bg, stage="fine")
        torch.autograd.backward([res["render"], res["alpha"]], [grad, grad_alpha])

    def train_two_frames(cam):
        clear()
        res = fdgs.render(cam, pc, pipe, bg, stage="fine")
        cover = fdgs.render(cam, pc, pipe, bg, override_color=ones, stage="fine")["render"][0:1]
        torch.autograd.backward([res["render"], cover], [grad, grad_alpha])

    legs = {k: [lambda cam=cam, f=f: f(cam) for cam in cams] for k, f in (("train", train), ("train_alpha", train_alpha),
                                                                          ("train_two_frames", train_two_frames))}
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "frames": frames, "warmup": warmup, "device": torch.cuda.get_device_name(0), "rounds": []}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        base = leg["train"]["median_ms"]
        leg["alpha_over_train"] = round(leg["train_alpha"]["median_ms"] / base, 4)
        leg["two_frames_over_train"] = round(leg["train_two_frames"]["median_ms"] / base, 4)
        doc["rounds"].append(leg)
        print(f"[alpha_timing] {name} round {r}: training frame {base:.4f} ms, with alpha in the loss {leg['train_alpha']['median_ms']:.4f} ms "
              f"(x{leg['alpha_over_train']}), as a second frame {leg['train_two_frames']['median_ms']:.4f} ms (x{leg['two_frames_over_train']})",
              flush=True)
    with torch.no_grad():       # what was timed is the alpha the second frame gives, to float32 rounding
        cam = cams[-1]
        a = fdgs.render(cam, pc, _AlphaPipe(), bg, stage="fine")["alpha"]
        b = fdgs.render(cam, pc, pipe, bg, override_color=ones, stage="fine")["render"][0:1]
        doc["alpha_vs_second_frame_max_abs"] = float((a - b).abs().max())
        doc["alpha_mean"] = float(a.mean())
    doc["kernels"] = {}
    for k in ("train", "train_alpha"):
        timed_calls = legs[k][warmup:]
        table = kernel_table(lambda: [f() for f in timed_calls])
        doc["kernels"][k] = {n: {"launches_per_frame": round(v["launches"] / len(timed_calls), 3),
                                 "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5),
                                 "kernel_ms_per_frame": round(v["ms"] / len(timed_calls), 5)} for n, v in table.items() if n in ROWS}
    print(f"[alpha_timing] {name} kernels: {json.dumps(doc['kernels'])}", flush=True)
    return doc


def _child(cmd, cwd=None):
    """One measurement in a process of its own under a time limit -> (exit status, its standard output)."""
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S)] + cmd, cwd=cwd, stdout=subprocess.PIPE, text=True)
    return p.returncode, p.stdout


def _bench(tree, extra=()):
    """`python bench.py` in `tree` -> (exit status, the JSON result line)."""
    rc, out = _child([sys.executable, "bench.py", "--gpus", "1", *extra], cwd=tree)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    return rc, (json.loads(lines[-1]) if rc == 0 and lines else None)


def no_regression(parent_tree, runs):
    trees = (("parent", os.path.abspath(parent_tree)), ("change", ROOT))
    doc = {"what": "`python bench.py` (frames/s, higher is better) in a checkout of the parent commit and in this tree, same machine, one session, "
                   "alternating; then bench.py --full --no-cpu-baseline --no-extras once in each for kernels_ms_per_step",
           "rule": "accepted when the median of the change's headline figures is not below the parent's lowest run",
           "headline_frames_per_s": {"parent": [], "change": []}, "ms_per_step": {"parent": [], "change": []}, "src_sha16": {}}
    for i in range(runs):
        for who, tree in trees:
            rc, res = _bench(tree)
            if res is None:
                print(f"[alpha_timing] bench.py in the {who} tree: exit status {rc}; stopping", flush=True)
                return None, rc or 1
            doc["headline_frames_per_s"][who].append(round(res["value"], 2))
            doc["ms_per_step"][who].append(round(res["ms_per_step"], 4))
            doc["src_sha16"][who] = res.get("src_sha16")
            print(f"[alpha_timing] run {i} {who}: {res['value']:.1f} frames/s ({res['ms_per_step']:.4f} ms per step)", flush=True)
    doc["kernels_ms_per_step"] = {}
    for who, tree in trees:
        rc, res = _bench(tree, ("--full", "--no-cpu-baseline", "--no-extras"))
        if res is None:
            print(f"[alpha_timing] bench.py --full in the {who} tree: exit status {rc}; stopping", flush=True)
            return None, rc or 1
        doc["kernels_ms_per_step"][who] = {k: res["kernels_ms_per_step"].get(k) for k in ("render_fwd", "render_bwd")}
    h = doc["headline_frames_per_s"]
    doc["change_median"], doc["parent_lowest"] = round(statistics.median(h["change"]), 2), min(h["parent"])
    doc["parent_median"] = round(statistics.median(h["parent"]), 2)
    doc["accepted"] = doc["change_median"] >= doc["parent_lowest"]
    print(f"[alpha_timing] no regression: change median {doc['change_median']} against parent lowest {doc['parent_lowest']} frames/s "
          f"(parent median {doc['parent_median']}): {'accepted' if doc['accepted'] else 'NOT accepted'}; kernels {json.dumps(doc['kernels_ms_per_step'])}",
          flush=True)
    return doc, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_timing.json"))
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
    doc["what"] = ("cost: a training frame (fdgs.render + backward) without alpha, with alpha in the loss, and with a second differentiable frame of "
                   "unit colours over black as the alpha; same process per configuration, HIP-event median per frame.  no_regression: bench.py of "
                   "the parent commit against this tree; tools/alpha_timing.py")
    if "cost" in sections:
        cost = {}
        with tempfile.TemporaryDirectory() as tmp:
            for name in ("cfg4_dynerf_300k_1352x1014", "cfg2_dnerf_100k_800x800"):
                part = os.path.join(tmp, name + ".json")
                rc, out = _child([sys.executable, os.path.abspath(__file__), "--config", name, "--out", part, "--frames", str(args.frames),
                                  "--warmup", str(args.warmup), "--rounds", str(args.rounds)])
                sys.stdout.write(out)
                if rc != 0:          # a failed or hung step: nothing more is started on the device
                    print(f"[alpha_timing] {name}: exit status {rc}; stopping", flush=True)
                    return rc
                with open(part) as f:
                    cost[name] = json.load(f)
        doc["cost"] = cost
    if "no_regression" in sections:
        rec, rc = no_regression(args.parent_tree, args.runs)
        if rec is None:
            return rc
        doc["no_regression"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
