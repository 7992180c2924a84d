#!/usr/bin/env python
"""tools/pick_timing.py -- what the pick pass costs on top of a baked playback frame, on BASELINE configs 2 and 4:

    cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800          cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014

The model is the bench's (SynthModel, seed 6666, Hilbert order, 32 baked timestamps), the cameras are the video orbit, every frame at a
baked timestamp.  Per configuration, as medians of HIP-event times over --frames frames (>= 30) after --warmup frames, one event pair per
frame, in --rounds rounds that alternate the two routes (reported one by one: their difference is the run-to-run spread):

    render        Baked.render
    render_pick   Baked.render_pick: the frame, then ONE fdgs_render_pick over the frame's own lists

plus the library's own per-kernel times of the render_pick frames of one round (fdgs_timing_report): the `render_fwd` and `render_pick`
rows, per launch.  The yardstick is the frame's own render_fwd row: the pick walks the same entries with one load fewer per staged entry
and no colour arithmetic, so pick_over_fwd should not exceed 1.1.

Every configuration is measured by a child process of its own under `timeout` (a step that hangs ends there and nothing is started after
a step that failed); this process never opens the device.  Writes profiles/pick_timing.json.  (GPU)"""
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
STEP_TIMEOUT_S = 240
ALPHA_CUT = 0.5


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
    legs = {"render": [lambda c=c: baked.render(c, pipe, bg) for c in cams],
            "render_pick": [lambda c=c: baked.render_pick(c, pipe, bg, alpha_cut=ALPHA_CUT) for c in cams]}
    one = legs["render_pick"][3]()
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "timestamps": T_BAKED, "frames": frames, "warmup": warmup, "alpha_cut": ALPHA_CUT,
           "device": torch.cuda.get_device_name(0), "rounds": [],
           "one_frame": {"pixels_with_a_pick": int((one["pick_id"] >= 0).sum()), "pixels_with_a_surface": int((one["surface_id"] >= 0).sum()),
                         "pixels": W * H}}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        leg["pick_minus_render_ms"] = round(leg["render_pick"]["median_ms"] - leg["render"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[pick_timing] {name} round {r}: render {leg['render']['median_ms']:.4f} ms, render_pick {leg['render_pick']['median_ms']:.4f} ms, "
              f"difference {leg['pick_minus_render_ms']:.4f} ms", flush=True)
    calls = legs["render_pick"][warmup:]
    table = kernel_table(lambda: [f() for f in calls])
    kernels = {k: {"launches": v["launches"], "launches_per_frame": round(v["launches"] / len(calls), 3),
                   "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5)}
               for k, v in table.items() if k in ("render_fwd", "render_pick", "tile_order", "preprocess_fwd")}
    doc["kernels_of_render_pick"] = kernels
    if "render_fwd" in kernels and "render_pick" in kernels:
        doc["pick_over_fwd"] = round(kernels["render_pick"]["kernel_ms_mean"] / kernels["render_fwd"]["kernel_ms_mean"], 4)
        doc["yardstick"] = "render_pick kernel time <= 1.1 x the same frames' render_fwd kernel time"
    doc["all_kernels_of_render_pick_ms_per_frame"] = {k: round(v["ms"] / len(calls), 5) for k, v in sorted(table.items())}
    print(f"[pick_timing] {name} kernels: {json.dumps(kernels)} pick_over_fwd = {doc.get('pick_over_fwd')}", flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick_timing.json"))
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
    doc = {"what": "Baked.render against Baked.render_pick, same process per configuration, HIP-event median per frame, and the render_fwd / "
                   "render_pick rows of fdgs_timing_report over the same frames; tools/pick_timing.py", "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("cfg2_dnerf_100k_800x800", "cfg4_dynerf_300k_1352x1014"):
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--config", name, "--out", part,
                   "--frames", str(args.frames), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
            rc = subprocess.call(cmd)
            if rc != 0:          # a failed or hung step: nothing more is started on the device
                print(f"[pick_timing] {name}: exit status {rc}; stopping", flush=True)
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
