#!/usr/bin/env python
"""tools/playback_timing.py -- a forward-only (evaluation) frame with and without the deformation: fdgs.render() under torch.no_grad()
against fdgs.playback.Baked.render, on the two BASELINE configurations with a deformation to skip:

    config 4   dynerf_default, 300 k Gaussians, 1352 x 1014      (all five heads on: 236 bytes per Gaussian and timestamp)
    config 2   dnerf_bouncingballs, 100 k Gaussians, 800 x 800   (no_do, no_dshs: 40 bytes per Gaussian and timestamp + 196 once)

The model is the bench's (SynthModel, seed 6666, Hilbert order), 32 timestamps are baked, the cameras are the video orbit.  Per
configuration, as the median of HIP-event times over --frames frames (>= 30) after --warmup frames, one event pair per frame:

    live                 render() under no_grad at baked timestamps            (the path a render.py loop takes without this module)
    baked                Baked.render at the same cameras and timestamps       (bit-identical images: tests/test_gpu_playback.py)
    baked_linear         Baked.render at the midpoints between timestamps      (one fdgs_state_blend launch more)
    blend                the fdgs_state_blend launch alone, with the bytes it moves per second next to the 6.3 TB/s HBM roof
    to_rgb8              fdgs_image_rgb8 of one frame
    bake                 the whole bake (32 deformation forwards + copies), once

plus the wall-clock frame rate of each leg, the stored bytes and the library's own per-kernel timing report of one frame of each leg.
Writes profiles/playback_timing.json.  (GPU)"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fdgs = importlib.import_module("4dgaussians_amd")
P, syn = fdgs.playback, fdgs.synthetic
CONFIGS = {"cfg4_dynerf_300k_1352x1014": (300_000, 1352, 1014, "dynerf_default"),
           "cfg2_dnerf_100k_800x800": (100_000, 800, 800, "dnerf_bouncingballs")}
HBM_ROOF_TBPS = 6.3
T_BAKED = 32


def kernel_table(fn):
    """The library's timing report of one call: {kernel: {launches, ms}}."""
    L = fdgs._lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    L.fdgs_timing_enable(1)
    try:
        fn()
        fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    finally:
        L.fdgs_timing_enable(0)
    return {l.split()[0]: {"launches": int(l.split()[1]), "ms": round(float(l.split()[2]), 4)} for l in buf.value.decode().strip().splitlines()}


def timed(calls, warmup):
    """calls: one callable per frame.  -> (HIP-event ms per frame after the warm-up frames, wall-clock ms per frame over the same frames)."""
    for c in calls[:warmup]:
        c()
    torch.cuda.synchronize()
    ms = []
    t0 = time.perf_counter()
    for c in calls[warmup:]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / max(len(ms), 1) * 1e3
    return ms, wall


def row(ms, wall):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "frames": len(ms),
            "wall_ms_per_frame": round(wall, 4), "wall_frames_per_s": round(1e3 / wall, 1)}


def measure(name, frames, warmup):
    N, W, H, dcfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(N, dcfg, seed=6666, device=dev)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    total = warmup + frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    at_stamps = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    mids = [0.5 * (times[k % (T_BAKED - 1)] + times[k % (T_BAKED - 1) + 1]) for k in range(total)]
    at_mids = [syn.make_camera(W, H, float(th), t).to(dev) for th, t in zip(thetas, mids)]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    baked = P.bake(pc, times)
    e1.record()
    torch.cuda.synchronize()
    bake_wall, bake_ms = (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
    assert all(P.locate(times, c.time)[0] == P.locate(times, c.time)[1] for c in at_stamps)
    assert all(P.locate(times, c.time)[0] != P.locate(times, c.time)[1] for c in at_mids)

    def live(cam):
        with torch.no_grad():
            return fdgs.render(cam, pc, pipe, bg, stage="fine")

    same = torch.equal(live(at_stamps[3])["render"], baked.render(at_stamps[3], pipe, bg)["render"])
    out = {"N": N, "W": W, "H": H, "deformation": dcfg, "head_on": list(baked.head_on), "timestamps": T_BAKED, "warmup": warmup,
           "nbytes": baked.nbytes, "bytes_per_gaussian_and_timestamp": 4 * sum(w for w, on in zip(P.FIELD_WIDTH, baked.head_on) if on),
           "baked_image_bit_identical_to_live": bool(same),
           "bake": {"event_ms": round(bake_ms, 3), "wall_ms": round(bake_wall, 3), "event_ms_per_timestamp": round(bake_ms / T_BAKED, 4)}}
    legs = {"live": [lambda c=c: live(c) for c in at_stamps],
            "baked": [lambda c=c: baked.render(c, pipe, bg) for c in at_stamps],
            "baked_linear": [lambda c=c: baked.render(c, pipe, bg, interp="linear") for c in at_mids]}
    for leg, calls in legs.items():
        out[leg] = row(*timed(calls, warmup))
        out[leg]["kernels_of_one_frame"] = kernel_table(calls[warmup])
        print(f"[playback_timing] {name} {leg}: median {out[leg]['median_ms']:.4f} ms per frame ({out[leg]['wall_frames_per_s']} frames/s wall)", flush=True)
    ms, wall = timed([lambda k=k: baked.blend(k % (T_BAKED - 1), k % (T_BAKED - 1) + 1, 0.5) for k in range(total)], warmup)
    moved = 3 * out["bytes_per_gaussian_and_timestamp"] * N          # two states read, one written
    out["blend"] = row(ms, wall)
    out["blend"].update({"bytes_moved": moved, "TB_per_s": round(moved / (statistics.median(ms) * 1e-3) / 1e12, 3), "hbm_roof_TB_per_s": HBM_ROOF_TBPS})
    image = baked.render(at_stamps[0], pipe, bg)["render"]
    for mode in ("trunc", "round"):
        out["to_rgb8_" + mode] = row(*timed([lambda: P.to_rgb8(image, mode)] * total, warmup))
    out["baked_not_above_live"] = out["baked"]["median_ms"] <= out["live"]["median_ms"]
    out["baked_over_live"] = round(out["baked"]["median_ms"] / out["live"]["median_ms"], 4)
    out["baked_linear_over_live"] = round(out["baked_linear"]["median_ms"] / out["live"]["median_ms"], 4)
    print(f"[playback_timing] {name}: blend {out['blend']['median_ms']:.4f} ms ({out['blend']['TB_per_s']} TB/s), bake {bake_ms:.1f} ms, "
          f"{baked.nbytes / 2 ** 20:.1f} MiB, baked / live = {out['baked_over_live']}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playback_timing.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames: at least 30")
    doc = {"what": "forward-only frame time, HIP-event median per frame: live = fdgs.render() under no_grad, baked = fdgs.playback.Baked.render at "
                   "baked timestamps, baked_linear = at midpoints (one fdgs_state_blend launch more); tools/playback_timing.py",
           "device": torch.cuda.get_device_name(0)}
    for name in args.configs:
        doc[name] = measure(name, args.frames, args.warmup)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
