#!/usr/bin/env python
"""tools/features_bwd_timing.py -- what a training step on per-row values costs on a baked playback frame, on BASELINE configs 2 and 4:

    cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800          cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014

The model is the bench's (SynthModel, seed 6666, Hilbert order, 32 baked timestamps), the cameras are the video orbit, every frame at a
baked timestamp.  Per configuration, as medians of HIP-event times over --frames frames (>= 30) after --warmup frames, one event pair per
frame, in --rounds rounds that alternate the routes (reported one by one: their difference is the run-to-run spread):

    render          Baked.render, the frame alone
    features_C      Baked.render_features with C = 3, 8, 16, 32 channels, forward only
    step_C          Baked.render_features(differentiable=True) and `.backward(G)` of its features with a fixed random gradient image: the
                    frame, ONE fdgs_render_features, ONE fdgs_render_features_bwd into a zeroed [N,C]
    live_train      fdgs.render of the live model at the same views and times and the backward of its image under a fixed random gradient
                    image: the training frame whose blending backward (`render_bwd`) the feature backward is set against

plus the library's own per-kernel times (fdgs_timing_report, per launch) over the frames of each step_C leg and of live_train: the
`render_features`, `render_features_bwd`, `render_fwd` and `render_bwd` rows, and the ratios of the feature backward to the feature forward
at the same C and to the blending backward.  Nothing here is a pass or fail condition.

Every configuration is measured by a child process of its own under `timeout` (a step that hangs ends there and nothing is started after
a step that failed); this process never opens the device.  Writes profiles/features_bwd_timing.json.  (GPU)"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 420
CHANNELS = (3, 8, 16, 32)
ROWS = ("render_fwd", "render_features", "render_features_bwd", "render_bwd", "tile_order", "preprocess_fwd")


def measure(name, frames, warmup, rounds):
    import numpy as np
    import torch
    from playback_timing import CONFIGS, T_BAKED, kernel_table, row, timed

    fdgs = importlib.import_module("4dgaussians_amd")
    P, syn = fdgs.playback, fdgs.synthetic
    N, W, H, dcfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(N, dcfg, seed=6666, device=dev)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    total = warmup + frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    cams = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    baked = P.bake(pc, times)
    gen = torch.Generator().manual_seed(3)
    values = torch.randn(N, max(CHANNELS), generator=gen).to(dev)
    grad = torch.randn(max(CHANNELS), H, W, generator=gen).to(dev)
    per_c = {c: (values[:, :c].contiguous(), values[:, :c].clone().requires_grad_(), grad[:c].contiguous()) for c in CHANNELS}

    def step(cam, c):
        _, v, g = per_c[c]
        v.grad = None
        baked.render_features(cam, pipe, bg, v, differentiable=True)["features"].backward(g)
        return v.grad

    def live_train(cam):
        for q in pc.parameters():
            q.grad = None
        fdgs.render(cam, pc, pipe, bg, stage="fine")["render"].backward(grad[:3])

    legs = {"render": [lambda cam=cam: baked.render(cam, pipe, bg) for cam in cams],
            "live_train": [lambda cam=cam: live_train(cam) for cam in cams]}
    for c in CHANNELS:
        legs[f"features_{c}"] = [lambda cam=cam, c=c: baked.render_features(cam, pipe, bg, per_c[c][0]) for cam in cams]
        legs[f"step_{c}"] = [lambda cam=cam, c=c: step(cam, c) for cam in cams]
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "timestamps": T_BAKED, "frames": frames, "warmup": warmup, "channels": list(CHANNELS),
           "device": torch.cuda.get_device_name(0), "rounds": []}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        for c in CHANNELS:
            leg[f"step_{c}_minus_features_ms"] = round(leg[f"step_{c}"]["median_ms"] - leg[f"features_{c}"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[features_bwd_timing] {name} round {r}: render {leg['render']['median_ms']:.4f} ms, live training frame "
              f"{leg['live_train']['median_ms']:.4f} ms; forward / forward + backward per frame: "
              + ", ".join(f"C={c}: {leg[f'features_{c}']['median_ms']:.4f} / {leg[f'step_{c}']['median_ms']:.4f} ms" for c in CHANNELS), flush=True)
    doc["kernels"] = {}
    for k, calls in legs.items():
        if not (k.startswith("step_") or k == "live_train"):
            continue
        timed_calls = calls[warmup:]
        table = kernel_table(lambda: [f() for f in timed_calls])
        doc["kernels"][k] = {n: {"launches_per_frame": round(v["launches"] / len(timed_calls), 3),
                                 "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5),
                                 "kernel_ms_per_frame": round(v["ms"] / len(timed_calls), 5)} for n, v in table.items() if n in ROWS}
    live = doc["kernels"]["live_train"]
    for c in CHANNELS:
        s = doc["kernels"][f"step_{c}"]
        if "render_features" in s and "render_features_bwd" in s and "render_bwd" in live:
            b = s["render_features_bwd"]["kernel_ms_mean"]
            doc[f"C{c}"] = {"render_features_bwd_kernel_ms": b, "render_features_kernel_ms": s["render_features"]["kernel_ms_mean"],
                            "render_fwd_kernel_ms": s["render_fwd"]["kernel_ms_mean"], "render_bwd_kernel_ms": live["render_bwd"]["kernel_ms_mean"],
                            "bwd_over_features_forward": round(b / s["render_features"]["kernel_ms_mean"], 4),
                            "bwd_over_render_bwd": round(b / live["render_bwd"]["kernel_ms_mean"], 4)}
    print(f"[features_bwd_timing] {name} kernels: {json.dumps({f'C{c}': doc.get(f'C{c}') for c in CHANNELS})}", flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bwd_timing.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--config", default=None, help="(internal) measure this one configuration in this process and write its record to --out")
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames: at least 30")
    if args.config is not None:
        with open(args.out, "w") as f:
            json.dump(measure(args.config, args.frames, args.warmup, args.rounds), f)
        return 0
    doc = {"what": "Baked.render_features forward against forward + backward (render_features(differentiable=True), .backward(G)) at C = 3, 8, "
                   "16, 32 and against a live training frame of the same model and views, same process per configuration, HIP-event median "
                   "per frame, and the render_features / render_features_bwd / render_bwd rows of fdgs_timing_report over the same frames; "
                   "tools/features_bwd_timing.py", "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("cfg4_dynerf_300k_1352x1014", "cfg2_dnerf_100k_800x800"):
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--config", name, "--out", part,
                   "--frames", str(args.frames), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
            rc = subprocess.call(cmd)
            if rc != 0:          # a failed or hung step: nothing more is started on the device
                print(f"[features_bwd_timing] {name}: exit status {rc}; stopping", flush=True)
                return rc
            with open(part) as f:
                doc["configs"][name] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
