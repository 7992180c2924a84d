#!/usr/bin/env python
"""tools/motion_timing.py -- what motion vectors and coverage cost on top of a baked playback frame, in one process, on BASELINE config 4:

    dynerf_default, 300 k Gaussians, 1352 x 1014, 32 timestamps

The model is the bench's (SynthModel, seed 6666, Hilbert order), the cameras are the video orbit, every frame at a baked timestamp and
`toward` the frame before it (its pose and its time).  Three routes, as the median of HIP-event times over --frames frames (>= 30) after
--warmup frames, one event pair per frame, in --rounds rounds that alternate the routes (the rounds are reported one by one: their
difference is the run-to-run spread):

    render          (a) Baked.render
    render_motion   (b) Baked.render_motion(cam, toward=previous camera): the frame, fdgs_motion_rows into recC, ONE more fdgs_render_fwd over the
                        frame's own lists, fdgs_motion_resolve
    two_frames      (c) what a user of the library can do without render_motion: Baked.render, both position sets projected with torch, a
                        WHOLE second frame (rasterize_forward with colors_precomp: projection, two sorts, blend), the divide in torch

plus the library's own per-kernel times of one round of (b) (fdgs_timing_report): motion_rows, motion_resolve, render_fwd, with the bytes
the two small kernels move per second next to the 6.3 TB/s HBM roof.  Writes profiles/motion_timing.json.  (GPU)"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from playback_timing import HBM_ROOF_TBPS, T_BAKED, kernel_table, row, timed  # noqa: E402

fdgs = importlib.import_module("4dgaussians_amd")
P, R, syn = fdgs.playback, fdgs.rasterizer, fdgs.synthetic
N, W, H, DCFG = 300_000, 1352, 1014, "dynerf_default"
MIN_ALPHA = 0.0


def _pixels(cam, xyz):
    """(pixel x, pixel y, view depth) of [N,3] points, in torch: the rasterizer's convention."""
    hom = xyz @ cam.full_proj_transform[:3] + cam.full_proj_transform[3]
    r = 1.0 / (hom[:, 3] + 1e-7)
    z = xyz @ cam.world_view_transform[:3, 2] + cam.world_view_transform[3, 2]
    return ((hom[:, 0] * r + 1.0) * W - 1.0) * 0.5, ((hom[:, 1] * r + 1.0) * H - 1.0) * 0.5, z


def two_frames(baked, cam, prev, pipe, bg, zero):
    """Route (c): no call into anything this tool's commit added."""
    out = baked.render(cam, pipe, bg)
    with torch.no_grad():
        xyz_to = baked.state_at(prev.time)[0].xyz
        st = baked.state_at(cam.time)[0]
        ax, ay, az = _pixels(cam, st.xyz)
        tx, ty, tz = _pixels(prev, xyz_to)
        ok = (az > 0.2) & (tz > 0.2)
        colors = torch.stack([torch.where(ok, tx - ax, 0.0), torch.where(ok, ty - ay, 0.0), torch.ones_like(ax)], dim=1)
        settings = R.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=float(np.tan(cam.FoVx * 0.5)), tanfovy=float(np.tan(cam.FoVy * 0.5)), bg=zero,
            scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=baked.active_sh_degree,
            campos=cam.camera_center, prefiltered=False, debug=False)
        raw, *_ = R.rasterize_forward(settings, st.xyz, None, colors, st.opacity, st.scales, st.rotations, None)
        a = raw[2:3]
        out["motion_raw"], out["alpha"] = raw, a
        out["motion"] = torch.where(a > MIN_ALPHA, raw[:2] / a, 0.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_timing.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rows", type=int, default=N, help="Gaussians (the default is config 4's; smaller only to rehearse)")
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames: at least 30")
    n = args.rows
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(n, DCFG, seed=6666, device=dev)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    pipe, bg, zero = syn.PipelineParams(), torch.zeros(3, device=dev), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    total = args.warmup + args.frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    cams = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    prevs = [cams[k - 1] for k in range(total)]
    baked = P.bake(pc, times)

    legs = {"render": [lambda c=c: baked.render(c, pipe, bg) for c in cams],
            "render_motion": [lambda c=c, q=q: baked.render_motion(c, pipe, bg, toward=q, min_alpha=MIN_ALPHA) for c, q in zip(cams, prevs)],
            "two_frames": [lambda c=c, q=q: two_frames(baked, c, q, pipe, bg, zero) for c, q in zip(cams, prevs)]}
    b, c = legs["render_motion"][3](), legs["two_frames"][3]()
    agree = {k: float((b[k] - c[k]).abs().max()) for k in ("motion_raw", "motion", "alpha")}
    doc = {"what": "Baked.render (a) against Baked.render_motion (b) against the route without it (c: a whole second frame with colors_precomp and "
                   "torch elementwise work), same process, HIP-event median per frame; tools/motion_timing.py",
           "device": torch.cuda.get_device_name(0), "N": n, "W": W, "H": H, "deformation": DCFG, "timestamps": T_BAKED, "frames": args.frames,
           "warmup": args.warmup, "rounds": [], "min_alpha": MIN_ALPHA,
           "expectation": {"blend_forward_ms_DESIGN": 0.17, "b_minus_a": "about one blend forward plus two small launches",
                           "c_minus_a": "about a whole frame (0.41 ms)"},
           "max_abs_difference_b_vs_c_one_frame": agree,
           "max_abs_motion_px_that_frame": float(b["motion"].abs().max())}
    for r in range(args.rounds):
        leg = {name: row(*timed(calls, args.warmup)) for name, calls in legs.items()}
        leg["b_minus_a_ms"] = round(leg["render_motion"]["median_ms"] - leg["render"]["median_ms"], 4)
        leg["c_minus_a_ms"] = round(leg["two_frames"]["median_ms"] - leg["render"]["median_ms"], 4)
        leg["b_over_c"] = round(leg["render_motion"]["median_ms"] / leg["two_frames"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[motion_timing] round {r}: (a) {leg['render']['median_ms']:.4f} ms, (b) {leg['render_motion']['median_ms']:.4f} ms, "
              f"(c) {leg['two_frames']['median_ms']:.4f} ms; b - a = {leg['b_minus_a_ms']:.4f}, c - a = {leg['c_minus_a_ms']:.4f}", flush=True)
    calls = legs["render_motion"][args.warmup:]
    table = kernel_table(lambda: [f() for f in calls])
    kernels = {}
    moved = {"motion_rows": n * (24 + 16), "motion_resolve": W * H * (12 + 12)}
    for name in ("motion_rows", "motion_resolve", "render_fwd", "tile_order", "preprocess_fwd"):
        k = table.get(name)
        if not k:
            continue
        kernels[name] = {"launches": k["launches"], "launches_per_frame": round(k["launches"] / len(calls), 3),
                         "kernel_ms_mean": round(k["ms"] / max(k["launches"], 1), 5)}
        if name in moved:
            kernels[name]["bytes_moved"] = moved[name]
            kernels[name]["TB_per_s_of_kernel_time"] = round(moved[name] / (k["ms"] / k["launches"] * 1e-3) / 1e12, 3)
            kernels[name]["hbm_roof_TB_per_s"] = HBM_ROOF_TBPS
    doc["kernels_of_render_motion"] = kernels
    doc["all_kernels_of_render_motion_ms_per_frame"] = {k: round(v["ms"] / len(calls), 5) for k, v in sorted(table.items())}
    print(f"[motion_timing] kernels: {json.dumps(kernels)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
