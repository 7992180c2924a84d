#!/usr/bin/env python
"""tools/compose_timing.py -- a frame of two placed models: fdgs.compose.Composite.render against what a user has without it, torch ops on
top of Baked frames (the loop of the reference's merge_many_4dgs.py: place with elementwise ops, `cat` every field, rasterize).

Workload: two BASELINE-config-4-sized synthetic models (dynerf_default, 300 k Gaussians each, all five heads on: 236 bytes per Gaussian and
timestamp), 1352 x 1014, 32 baked timestamps each, the video orbit; the second model is turned, shifted and scaled.  As the median of
HIP-event times over --frames frames (>= 30) after --warmup frames, one event pair per frame:

    compose              Composite.render at baked timestamps          (two fdgs_state_place launches, no blend, + the rasterizer)
    compose_linear       Composite.render at midpoints                 (the temporal blend fused into the same two launches)
    torch_route          Baked.state_at per model, (xyz * s) @ R^T + d, scales * s, torch.cat of the five fields, GaussianRasterizer
    torch_route_linear   the same at midpoints                         (one fdgs_state_blend launch per model more)
    place / place_blend  ONE fdgs_state_place launch of one model alone, without and with the fused blend, with the bytes it moves per second
    blend                ONE fdgs_state_blend launch of one model (the streaming kernel the playback unit already had), from the same run

plus the library's per-kernel timing report of one frame of each leg.  Writes profiles/compose_timing.json.  (GPU)"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from playback_timing import HBM_ROOF_TBPS, kernel_table, row, timed  # noqa: E402

fdgs = importlib.import_module("4dgaussians_amd")
C, P, syn = fdgs.compose, fdgs.playback, fdgs.synthetic
N, W, H, DCFG = 300_000, 1352, 1014, "dynerf_default"
T_BAKED = 32
ROW_BYTES = 4 * sum(P.FIELD_WIDTH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_timing.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    if args.frames < 30:
        ap.error("--frames: at least 30")
    dev = torch.device("cuda:0")
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    models = []
    for seed in (6666, 7777):
        pc = syn.SynthModel(N, DCFG, seed=seed, device=dev)
        fdgs.densify.spatial_reorder(pc, curve="hilbert")
        models.append(P.bake(pc, times))
        del pc
    c, s = np.cos(0.8), np.sin(0.8)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    placements = [C.Placement(), C.Placement(rotation=R, translation=(1.2, 0.0, -0.4), scale=0.8)]
    scene = C.compose(models, placements)
    total = args.warmup + args.frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    at_stamps = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    mids = [0.5 * (times[k % (T_BAKED - 1)] + times[k % (T_BAKED - 1) + 1]) for k in range(total)]
    at_mids = [syn.make_camera(W, H, float(th), t).to(dev) for th, t in zip(thetas, mids)]
    Rt = [torch.tensor(p.rotation, device=dev).t().contiguous() for p in placements]
    dt = [torch.tensor(p.translation, device=dev) for p in placements]

    def torch_route(cam):
        """merge_many_4dgs.py's render(): the script's semantics (positions and scales only), one cat per field and frame."""
        with torch.no_grad():
            parts = []
            for m, (model, p) in enumerate(zip(models, placements)):
                st, _ = model.state_at(cam.time)
                if m == 0:
                    parts.append((st.xyz, st.scales, st.rotations, st.opacity, st.shs))
                else:
                    parts.append((torch.matmul(st.xyz * float(p.scale), Rt[m]) + dt[m], st.scales * float(p.scale), st.rotations, st.opacity, st.shs))
            xyz, scales, rots, op, shs = (torch.cat(f, dim=0) for f in zip(*parts))
            settings = fdgs.GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=float(np.tan(cam.FoVx * 0.5)), tanfovy=float(np.tan(cam.FoVy * 0.5)), bg=bg,
                scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=scene.active_sh_degree,
                campos=cam.camera_center, prefiltered=False, debug=False)
            return fdgs.GaussianRasterizer(settings)(means3D=xyz, means2D=torch.zeros_like(xyz), shs=shs, opacities=op, scales=scales, rotations=rots)

    doc = {"what": "frame time of two placed 300 k-Gaussian models, HIP-event median per frame: compose = fdgs.compose.Composite.render, torch_route = "
                   "torch ops + cat on Baked frames + GaussianRasterizer (the reference script's loop); tools/compose_timing.py",
           "device": torch.cuda.get_device_name(0), "N_per_model": N, "models": 2, "W": W, "H": H, "deformation": DCFG, "timestamps": T_BAKED,
           "warmup": args.warmup, "row_bytes": ROW_BYTES, "composite_nbytes": scene.nbytes, "hbm_roof_TB_per_s": HBM_ROOF_TBPS}
    legs = {"compose": [lambda c=c: scene.render(c, pipe, bg) for c in at_stamps],
            "compose_linear": [lambda c=c: scene.render(c, pipe, bg) for c in at_mids],
            "torch_route": [lambda c=c: torch_route(c) for c in at_stamps],
            "torch_route_linear": [lambda c=c: torch_route(c) for c in at_mids]}
    for leg, calls in legs.items():
        doc[leg] = row(*timed(calls, args.warmup))
        doc[leg]["kernels_of_one_frame"] = kernel_table(calls[args.warmup])
        print(f"[compose_timing] {leg}: median {doc[leg]['median_ms']:.4f} ms per frame ({doc[leg]['wall_frames_per_s']} frames/s wall)", flush=True)
    # one launch alone: model 1 (the general placement), all five fields
    kernels = {"place": ([lambda k=k: scene._place(1, 31, k % T_BAKED, k % T_BAKED, 0.0) for k in range(total)], 2 * ROW_BYTES * N),
               "place_blend": ([lambda k=k: scene._place(1, 31, k % (T_BAKED - 1), k % (T_BAKED - 1) + 1, 0.5) for k in range(total)], 3 * ROW_BYTES * N),
               "blend": ([lambda k=k: models[1].blend(k % (T_BAKED - 1), k % (T_BAKED - 1) + 1, 0.5) for k in range(total)], 3 * ROW_BYTES * N)}
    for name, (calls, moved) in kernels.items():
        ms, wall = timed(calls, args.warmup)
        doc[name] = row(ms, wall)
        doc[name].update({"bytes_moved": moved, "TB_per_s": round(moved / (statistics.median(ms) * 1e-3) / 1e12, 3)})
        print(f"[compose_timing] {name}: median {doc[name]['median_ms']:.4f} ms, {doc[name]['TB_per_s']} TB/s", flush=True)
    scene._shown = [None] * len(models)
    doc["place_over_blend_bytes_per_s"] = round(doc["place_blend"]["TB_per_s"] / doc["blend"]["TB_per_s"], 4)
    doc["place_below_half_of_blend"] = doc["place_over_blend_bytes_per_s"] < 0.5
    doc["compose_over_torch_route"] = round(doc["compose"]["median_ms"] / doc["torch_route"]["median_ms"], 4)
    doc["compose_linear_over_torch_route_linear"] = round(doc["compose_linear"]["median_ms"] / doc["torch_route_linear"]["median_ms"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
