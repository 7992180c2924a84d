#!/usr/bin/env python
"""tools/sparse_playback_timing.py -- the dense bake against the sparse bake, in one process, on BASELINE config 4:

    dynerf_default, 300 k Gaussians, 1352 x 1014, 32 timestamps    (all five heads on: 236 bytes per Gaussian and timestamp)

The model is the bench's (SynthModel, seed 6666, Hilbert order), the cameras are the video orbit.  A share s of dynamic rows is forced
through the tolerance: tol = (q, inf, inf, inf, inf) with q the (1 - s) quantile of the position column of fdgs.playback.motion_extent, so
that the positions alone decide and s * N rows (up to ties) are dynamic; s = 1 is tol = -1.  Per share, as the median of HIP-event times
over --frames frames (>= 30) after --warmup frames, one event pair per frame, in --rounds rounds that alternate the dense and the sparse
legs (the rounds are reported one by one: their difference is the run-to-run spread):

    dense / dense_linear       Baked.render at baked timestamps / at the midpoints          (the midpoints: one fdgs_state_blend launch more)
    sparse / sparse_linear     SparseBaked.render at the same cameras; every frame is at another time than the one before, so every
                               frame pays ONE fdgs_state_scatter launch: a copy at a baked timestamp, the fused blend at a midpoint
    blend                      the fdgs_state_blend launch of the dense bake alone
    scatter_copy / _blend      the fdgs_state_scatter launch alone (SparseBaked.state_at), with the bytes it moves,
                               D * (2 or 3) * bytes_on + 4 * D, per second next to the 6.3 TB/s HBM roof; next to the event median the
                               library's own per-kernel time (fdgs_timing_report) averaged over the same calls
    bake / bake_sparse         the whole bake, once, wall clock around a synchronise

plus the stored bytes.  Writes profiles/sparse_playback_timing.json.  (GPU)"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from playback_timing import HBM_ROOF_TBPS, T_BAKED, kernel_table, row, timed  # noqa: E402

fdgs = importlib.import_module("4dgaussians_amd")
P, syn = fdgs.playback, fdgs.synthetic
N, W, H, DCFG = 300_000, 1352, 1014, "dynerf_default"
SHARES = (1.0, 0.5, 0.1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def launch_row(calls, warmup, kernel, moved):
    """One state update per call: the event median, the library's own kernel time averaged over the timed calls, bytes per second."""
    ms, wall = timed(calls, warmup)
    table = kernel_table(lambda: [c() for c in calls[warmup:]])
    r = row(ms, wall)
    k = table.get(kernel, {"launches": 0, "ms": 0.0})
    r.update({"kernel": kernel, "kernel_launches": k["launches"], "kernel_ms_mean": round(k["ms"] / max(k["launches"], 1), 5), "bytes_moved": moved})
    if k["launches"]:
        r["TB_per_s_of_kernel_time"] = round(moved / (k["ms"] / k["launches"] * 1e-3) / 1e12, 3)
        r["hbm_roof_TB_per_s"] = HBM_ROOF_TBPS
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_playback_timing.json"))
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
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    total = args.warmup + args.frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    mids = [0.5 * (times[k % (T_BAKED - 1)] + times[k % (T_BAKED - 1) + 1]) for k in range(total)]
    at_stamps = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    at_mids = [syn.make_camera(W, H, float(th), t).to(dev) for th, t in zip(thetas, mids)]

    P.bake(pc, times[:2])                                           # (code objects loaded before anything is timed)
    baked, bake_ms = wall_ms(lambda: P.bake(pc, times))
    ext, extent_ms = wall_ms(lambda: P.motion_extent(pc, times))
    bytes_on = 4 * sum(w for w, on in zip(P.FIELD_WIDTH, baked.head_on) if on)
    doc = {"what": "dense fdgs.playback.Baked against fdgs.playback.SparseBaked at forced shares of dynamic rows, same process, HIP-event "
                   "median per frame; tools/sparse_playback_timing.py",
           "device": torch.cuda.get_device_name(0), "N": n, "W": W, "H": H, "deformation": DCFG, "head_on": list(baked.head_on),
           "timestamps": T_BAKED, "frames": args.frames, "warmup": args.warmup, "rounds": args.rounds, "bytes_on_per_row": bytes_on,
           "dense_nbytes": baked.nbytes, "bake_wall_ms": round(bake_ms, 3), "motion_extent_wall_ms": round(extent_ms, 3),
           "parent_commit_figures": {"state_blend_ms": 0.041, "baked_frame_ms": 0.412, "source": "profiles/playback_timing.json"},
           "extent_quantiles_of_positions": {str(q): float(torch.quantile(ext[:, 0], q)) for q in (0.1, 0.5, 0.9)}}
    sparse = {}
    for s in SHARES:
        tol = -1.0 if s >= 1.0 else (float(torch.kthvalue(ext[:, 0], max(1, math.ceil((1.0 - s) * n))).values), *([math.inf] * 4))
        sb, ms = wall_ms(lambda: P.bake_sparse(pc, times, tol))
        sparse[s] = sb
        doc[f"share_{s}"] = {"tol": tol if isinstance(tol, float) else [t if math.isfinite(t) else "inf" for t in tol], "D": sb.D,
                             "dynamic_share": round(sb.D / n, 4), "nbytes": sb.nbytes, "nbytes_over_dense": round(sb.nbytes / baked.nbytes, 4),
                             "bake_sparse_wall_ms": round(ms, 3), "bake_sparse_over_bake": round(ms / bake_ms, 3), "rounds": []}
        print(f"[sparse_playback_timing] share {s}: D = {sb.D}, {sb.nbytes / 2 ** 20:.1f} MiB (dense {baked.nbytes / 2 ** 20:.1f}), "
              f"bake_sparse {ms:.1f} ms (bake {bake_ms:.1f})", flush=True)
    same = all(torch.equal(sparse[1.0].render(c, pipe, bg)["render"], baked.render(c, pipe, bg)["render"]) for c in (at_stamps[3], at_mids[5]))
    doc["share_1.0_images_bit_identical_to_dense"] = bool(same)
    doc["dense_rounds"] = []
    for r in range(args.rounds):
        dense = {"dense": row(*timed([lambda c=c: baked.render(c, pipe, bg) for c in at_stamps], args.warmup)),
                 "dense_linear": row(*timed([lambda c=c: baked.render(c, pipe, bg) for c in at_mids], args.warmup)),
                 "blend": launch_row([lambda k=k: baked.blend(k % (T_BAKED - 1), k % (T_BAKED - 1) + 1, 0.5) for k in range(total)], args.warmup,
                                     "state_blend", 3 * bytes_on * n)}
        doc["dense_rounds"].append(dense)
        print(f"[sparse_playback_timing] round {r} dense: frame {dense['dense']['median_ms']:.4f} ms, in between {dense['dense_linear']['median_ms']:.4f} ms, "
              f"blend {dense['blend']['kernel_ms_mean']:.4f} ms", flush=True)
        for s, sb in sparse.items():
            leg = {"sparse": row(*timed([lambda c=c: sb.render(c, pipe, bg) for c in at_stamps], args.warmup)),
                   "sparse_linear": row(*timed([lambda c=c: sb.render(c, pipe, bg) for c in at_mids], args.warmup)),
                   "scatter_copy": launch_row([lambda c=c: sb.state_at(c.time) for c in at_stamps], args.warmup, "state_scatter",
                                              sb.D * (2 * bytes_on + 4)),
                   "scatter_blend": launch_row([lambda c=c: sb.state_at(c.time) for c in at_mids], args.warmup, "state_scatter",
                                               sb.D * (3 * bytes_on + 4))}
            leg["sparse_over_dense"] = round(leg["sparse"]["median_ms"] / dense["dense"]["median_ms"], 4)
            leg["sparse_linear_over_dense_linear"] = round(leg["sparse_linear"]["median_ms"] / dense["dense_linear"]["median_ms"], 4)
            if s >= 1.0 and dense["blend"]["kernel_ms_mean"] > 0:
                leg["blend_scatter_over_state_blend_kernel_time"] = round(leg["scatter_blend"]["kernel_ms_mean"] / dense["blend"]["kernel_ms_mean"], 4)
            doc[f"share_{s}"]["rounds"].append(leg)
            print(f"[sparse_playback_timing] round {r} share {s}: frame {leg['sparse']['median_ms']:.4f} ms, in between "
                  f"{leg['sparse_linear']['median_ms']:.4f} ms, scatter copy {leg['scatter_copy']['kernel_ms_mean']:.4f} / blend "
                  f"{leg['scatter_blend']['kernel_ms_mean']:.4f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
