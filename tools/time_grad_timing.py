#!/usr/bin/env python
"""tools/time_grad_timing.py -- what the time's gradient costs a training frame, on BASELINE configs 4 and 2:

    cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014          cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800

The model is the bench's (SynthModel, seed 6666, Hilbert order), the cameras are the video orbit.  Per configuration, as medians of HIP-event
times over --frames frames (>= 30) after --warmup frames, one event pair per frame, in --rounds rounds that alternate the legs (reported
one by one: their difference is the run-to-run spread):

    train           fdgs.render of the live model and the backward of its image under a fixed random gradient image
    train_time      the same frame with camera.time a scalar tensor that requires grad: the sibling autograd node, the host read of the
                    time's value in the forward, fdgs_deform_time_grad behind fdgs_deform_bwd
    train_fd        the only route there was before: a central finite difference -- the training frame plus two more forward frames (no
                    graph) at t -/+ h and the difference of their images against the same gradient image

plus the library's own per-kernel times (fdgs_timing_report, per launch) over the frames of the first two legs: the two launches of
fdgs_deform_time_grad (`deform_time_grad_partial`, `deform_time_grad_final`) with the deformation backward's kernels beside them.  Nothing
here is a pass or fail condition.

Every configuration is measured by a child process of its own under `timeout` (a step that hangs ends there and nothing is started after
a step that failed); this process never opens the device.  Writes profiles/time_grad_timing.json.  (GPU)"""
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
STEP_TIMEOUT_S = 300
ROWS = ("deform_time_grad_partial", "deform_time_grad_final", "deform_plane_grad", "deform_bwd_data", "deform_wgrad", "row_list", "deform_fwd")
FD_STEP = 1e-3


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
    times = [0.02 + 0.96 * float(k % 32) / 31.0 for k in range(total)]      # (inside the time rows: a clamped time has no gradient to form)
    cams = [syn.make_camera(W, H, float(th), t).to(dev) for th, t in zip(thetas, times)]
    timed_cams = [syn.make_camera(W, H, float(th), t).to(dev) for th, t in zip(thetas, times)]
    for cam in timed_cams:
        cam.time = torch.tensor(cam.time, device=dev, requires_grad=True)
    grad = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    fd_out = []

    def train(cam):
        for q in pc.parameters():
            q.grad = None
        if isinstance(cam.time, torch.Tensor):
            cam.time.grad = None
        fdgs.render(cam, pc, pipe, bg, stage="fine")["render"].backward(grad)

    def train_fd(cam):
        train(cam)
        t = cam.time
        with torch.no_grad():
            cam.time = t + FD_STEP
            hi = fdgs.render(cam, pc, pipe, bg, stage="fine")["render"]
            cam.time = t - FD_STEP
            lo = fdgs.render(cam, pc, pipe, bg, stage="fine")["render"]
            cam.time = t
            fd_out[:] = [((hi - lo) * grad).sum() / (2 * FD_STEP)]

    legs = {"train": [lambda cam=cam: train(cam) for cam in cams], "train_time": [lambda cam=cam: train(cam) for cam in timed_cams],
            "train_fd": [lambda cam=cam: train_fd(cam) for cam in cams]}
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "frames": frames, "warmup": warmup, "device": torch.cuda.get_device_name(0),
           "fd_step": FD_STEP, "rounds": []}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        leg["time_minus_train_ms"] = round(leg["train_time"]["median_ms"] - leg["train"]["median_ms"], 4)
        leg["fd_minus_train_ms"] = round(leg["train_fd"]["median_ms"] - leg["train"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[time_grad_timing] {name} round {r}: training frame {leg['train']['median_ms']:.4f} ms, with a time leaf "
              f"{leg['train_time']['median_ms']:.4f} ms, with a central finite difference {leg['train_fd']['median_ms']:.4f} ms", flush=True)
    assert timed_cams[-1].time.grad is not None and timed_cams[-1].time.grad.shape == ()
    doc["last_frame"] = {"dL_dt": float(timed_cams[-1].time.grad), "finite_difference": float(fd_out[0])}
    doc["kernels"] = {}
    for k in ("train", "train_time"):
        timed_calls = legs[k][warmup:]
        table = kernel_table(lambda: [f() for f in timed_calls])
        doc["kernels"][k] = {n: {"launches_per_frame": round(v["launches"] / len(timed_calls), 3),
                                 "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5),
                                 "kernel_ms_per_frame": round(v["ms"] / len(timed_calls), 5)} for n, v in table.items() if n in ROWS}
    print(f"[time_grad_timing] {name} kernels: {json.dumps(doc['kernels'])}; last frame {json.dumps(doc['last_frame'])}", flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_grad_timing.json"))
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
    doc = {"what": "a training frame (fdgs.render + backward) without a time leaf, with one, and with the central finite difference that was "
                   "the only route before (two more forward frames); same process per configuration, HIP-event median per frame, legs "
                   "alternating per round; and the deform_time_grad_partial / deform_time_grad_final rows of fdgs_timing_report with the "
                   "deformation backward's kernels beside them, over the same frames; tools/time_grad_timing.py", "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("cfg4_dynerf_300k_1352x1014", "cfg2_dnerf_100k_800x800"):
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--config", name, "--out", part,
                   "--frames", str(args.frames), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
            rc = subprocess.call(cmd)
            if rc != 0:          # a failed or hung step: nothing more is started on the device
                print(f"[time_grad_timing] {name}: exit status {rc}; stopping", flush=True)
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
