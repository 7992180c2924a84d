#!/usr/bin/env python
"""tools/sparse_compose_timing.py -- a composite of two placed models over dense bakes against the same composite over sparse bakes
(fdgs.compose.compose(..., allow_sparse=True)), in one process:

    two dynerf_default models, 300 k Gaussians each, 1352 x 1014, 32 timestamps    (all five heads on: 236 bytes per Gaussian and timestamp)

The models, the placements and the cameras are those of tools/compose_timing.py; a share s of dynamic rows is forced per model as in
tools/sparse_playback_timing.py (tol = (q, inf, inf, inf, inf), q the (1 - s) quantile of the model's position extents; s = 1 is tol = -1).
As the median of HIP-event times over --frames frames (>= 64) after --warmup frames, one event pair per frame, in --rounds rounds that
alternate the dense and the sparse legs (reported one by one: their difference is the run-to-run spread):

    dense / dense_linear        Composite.render over the dense bakes at baked timestamps / at the midpoints: two fdgs_state_place launches
                                over all N rows of each model (the baseline: this code is the parent commit's)
    sparse / sparse_linear      Composite.render over the sparse bakes at the same cameras: every frame is at another time than the one
                                before, so every frame pays ONE fdgs_state_place_rows launch per model over its D rows
    place_copy / _blend         the fdgs_state_place launch of model 1 alone (all five fields, N rows), N * (2 or 3) * bytes_on moved
    place_rows_copy / _blend    the fdgs_state_place_rows launch of model 1 alone, D * (2 or 3) * bytes_on + 4 * D moved, per second next to
                                the 6.3 TB/s HBM roof; next to the event median the library's own per-kernel time (fdgs_timing_report)

plus the stored bytes of both scenes.  Nothing is asserted.  Writes profiles/sparse_compose_timing.json.  (GPU)"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from playback_timing import HBM_ROOF_TBPS, T_BAKED, row, timed  # noqa: E402
from sparse_playback_timing import launch_row  # noqa: E402

fdgs = importlib.import_module("4dgaussians_amd")
C, P, syn = fdgs.compose, fdgs.playback, fdgs.synthetic
N, W, H, DCFG = 300_000, 1352, 1014, "dynerf_default"
SHARES = (1.0, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_compose_timing.json"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rows", type=int, default=N, help="Gaussians per model (the default is config 4's; smaller only to rehearse)")
    args = ap.parse_args()
    if args.frames < 64:
        ap.error("--frames: at least 64")
    n = args.rows
    dev = torch.device("cuda:0")
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    c, s = np.cos(0.8), np.sin(0.8)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    placements = [C.Placement(), C.Placement(rotation=R, translation=(1.2, 0.0, -0.4), scale=0.8)]
    dense, sparse = [], {s: [] for s in SHARES}
    for seed in (6666, 7777):
        pc = syn.SynthModel(n, DCFG, seed=seed, device=dev)
        fdgs.densify.spatial_reorder(pc, curve="hilbert")
        dense.append(P.bake(pc, times))
        ext = P.motion_extent(pc, times)
        for s in SHARES:
            tol = -1.0 if s >= 1.0 else (float(torch.kthvalue(ext[:, 0], max(1, math.ceil((1.0 - s) * n))).values), *([math.inf] * 4))
            sparse[s].append(P.bake_sparse(pc, times, tol))
        del pc, ext
    bytes_on = 4 * sum(w for w, on in zip(P.FIELD_WIDTH, dense[1].head_on) if on)
    mask = P._field_mask(dense[1].head_on)
    scene_dense = C.compose(dense, placements)
    scenes = {s: C.compose(sparse[s], placements, allow_sparse=True) for s in SHARES}
    total = args.warmup + args.frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    mids = [0.5 * (times[k % (T_BAKED - 1)] + times[k % (T_BAKED - 1) + 1]) for k in range(total)]
    at_stamps = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    at_mids = [syn.make_camera(W, H, float(th), t).to(dev) for th, t in zip(thetas, mids)]
    copies = [(k % T_BAKED, k % T_BAKED, 0.0) for k in range(total)]
    blends = [(k % (T_BAKED - 1), k % (T_BAKED - 1) + 1, 0.5) for k in range(total)]

    doc = {"what": "frame time of two placed 300 k-Gaussian models, HIP-event median per frame: fdgs.compose.Composite.render over dense bakes "
                   "against the same composite over sparse bakes (allow_sparse=True) at forced shares of dynamic rows, same process; "
                   "tools/sparse_compose_timing.py",
           "device": torch.cuda.get_device_name(0), "N_per_model": n, "models": 2, "W": W, "H": H, "deformation": DCFG, "timestamps": T_BAKED,
           "frames": args.frames, "warmup": args.warmup, "rounds": args.rounds, "bytes_on_per_row": bytes_on, "hbm_roof_TB_per_s": HBM_ROOF_TBPS,
           "composite_nbytes": scene_dense.nbytes, "dense_stored_nbytes": sum(m.nbytes for m in dense), "dense_rounds": []}
    for s in SHARES:
        same = all(torch.equal(scenes[s].render(cam, pipe, bg)["render"], scene_dense.render(cam, pipe, bg)["render"]) for cam in (at_stamps[3], at_mids[5]))
        doc[f"share_{s}"] = {"D": [m.D for m in sparse[s]], "dynamic_share": [round(m.D / n, 4) for m in sparse[s]],
                             "stored_nbytes": sum(m.nbytes for m in sparse[s]), "composite_nbytes": scenes[s].nbytes,
                             "stored_over_dense": round(sum(m.nbytes for m in sparse[s]) / sum(m.nbytes for m in dense), 4),
                             "images_bit_identical_to_dense": bool(same), "rounds": []}
    for r in range(args.rounds):
        leg = {"dense": row(*timed([lambda cam=cam: scene_dense.render(cam, pipe, bg) for cam in at_stamps], args.warmup)),
               "dense_linear": row(*timed([lambda cam=cam: scene_dense.render(cam, pipe, bg) for cam in at_mids], args.warmup)),
               "place_copy": launch_row([lambda k=k: scene_dense._place(1, mask, *k) for k in copies], args.warmup, "state_place", 2 * bytes_on * n),
               "place_blend": launch_row([lambda k=k: scene_dense._place(1, mask, *k) for k in blends], args.warmup, "state_place", 3 * bytes_on * n)}
        scene_dense._shown = [None] * 2
        doc["dense_rounds"].append(leg)
        print(f"[sparse_compose_timing] round {r} dense: frame {leg['dense']['median_ms']:.4f} ms, in between {leg['dense_linear']['median_ms']:.4f} ms, "
              f"place copy {leg['place_copy']['kernel_ms_mean']:.4f} / blend {leg['place_blend']['kernel_ms_mean']:.4f} ms", flush=True)
        base = leg
        for s, scene in scenes.items():
            D = sparse[s][1].D
            leg = {"sparse": row(*timed([lambda cam=cam: scene.render(cam, pipe, bg) for cam in at_stamps], args.warmup)),
                   "sparse_linear": row(*timed([lambda cam=cam: scene.render(cam, pipe, bg) for cam in at_mids], args.warmup)),
                   "place_rows_copy": launch_row([lambda k=k: scene._place(1, mask, *k) for k in copies], args.warmup, "state_place_rows",
                                                 D * 2 * bytes_on + 4 * D),
                   "place_rows_blend": launch_row([lambda k=k: scene._place(1, mask, *k) for k in blends], args.warmup, "state_place_rows",
                                                  D * 3 * bytes_on + 4 * D)}
            scene._shown = [None] * 2
            leg["sparse_over_dense"] = round(leg["sparse"]["median_ms"] / base["dense"]["median_ms"], 4)
            leg["sparse_linear_over_dense_linear"] = round(leg["sparse_linear"]["median_ms"] / base["dense_linear"]["median_ms"], 4)
            for kind in ("copy", "blend"):
                if base[f"place_{kind}"]["kernel_ms_mean"] > 0:
                    leg[f"place_rows_{kind}_over_place_{kind}_kernel_time"] = round(
                        leg[f"place_rows_{kind}"]["kernel_ms_mean"] / base[f"place_{kind}"]["kernel_ms_mean"], 4)
            doc[f"share_{s}"]["rounds"].append(leg)
            print(f"[sparse_compose_timing] round {r} share {s}: frame {leg['sparse']['median_ms']:.4f} ms, in between "
                  f"{leg['sparse_linear']['median_ms']:.4f} ms, place_rows copy {leg['place_rows_copy']['kernel_ms_mean']:.4f} / blend "
                  f"{leg['place_rows_blend']['kernel_ms_mean']:.4f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
