#!/usr/bin/env python
"""tools/contrib_timing.py -- what the contribution pass costs on top of a baked playback frame, and what it saves, on BASELINE configs 2
and 4:

    cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800          cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014

The model is the bench's (SynthModel, seed 6666, Hilbert order, 32 baked timestamps), the cameras are the video orbit, every frame at a
baked timestamp.  Per configuration, as medians of HIP-event times over --frames frames (>= 30) after --warmup frames, one event pair per
frame, in --rounds rounds that alternate the two routes (reported one by one: their difference is the run-to-run spread):

    render           Baked.render
    render_contrib   Baked.render_contrib: the frame, then ONE fdgs_render_contrib over the frame's own lists, into one Contribution

plus the library's own per-kernel times (fdgs_timing_report, per launch): the `render_fwd` and `render_contrib` rows of the render_contrib
frames of one round, and the `render_bwd` row of TRAINING frames (fdgs.render + backward) of the same model at the same views.  The
yardstick is that render_bwd: the contribution pass is the blending backward's walk over the same lists with three values reduced per hit
in place of nine and at most 16 bytes of atomics per (tile, entry) in place of a 64-byte line, so it should take no longer.

What it saves: the share of the rows no pixel of any of the tool's views shows (pixels == 0 after all frames), and the stored bytes of the
bake before and after `select_rows` of the others.

Every configuration is measured by a child process of its own under `timeout` (a step that hangs ends there and nothing is started after
a step that failed); this process never opens the device.  Writes profiles/contrib_timing.json.  (GPU)"""
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
TRAIN_VIEWS = 16
ROWS = ("render_fwd", "render_contrib", "tile_order", "preprocess_fwd")


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
    acc = P.Contribution(baked.N, dev)
    legs = {"render": [lambda c=c: baked.render(c, pipe, bg) for c in cams],
            "render_contrib": [lambda c=c: baked.render_contrib(c, pipe, bg, into=acc) for c in cams]}
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "timestamps": T_BAKED, "frames": frames, "warmup": warmup,
           "device": torch.cuda.get_device_name(0), "lib": os.path.basename(fdgs._lib.LIB_PATH), "rounds": []}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        leg["contrib_minus_render_ms"] = round(leg["render_contrib"]["median_ms"] - leg["render"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[contrib_timing] {name} round {r}: render {leg['render']['median_ms']:.4f} ms, render_contrib "
              f"{leg['render_contrib']['median_ms']:.4f} ms, difference {leg['contrib_minus_render_ms']:.4f} ms", flush=True)
    calls = legs["render_contrib"][warmup:]
    table = kernel_table(lambda: [f() for f in calls])
    kernels = {k: {"launches": v["launches"], "launches_per_frame": round(v["launches"] / len(calls), 3),
                   "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5)} for k, v in table.items() if k in ROWS}
    doc["kernels_of_render_contrib"] = kernels
    doc["all_kernels_of_render_contrib_ms_per_frame"] = {k: round(v["ms"] / len(calls), 5) for k, v in sorted(table.items())}

    # the saving: one clean pass over every view of the tool, then the rows none of them shows
    acc.reset()
    P.contribution(baked, cams, pipe, bg, into=acc)
    keep = acc.keep_mask(min_pixels=1)
    unseen = 1.0 - float(keep.sum()) / N
    small = baked.select_rows(keep)
    doc["saving"] = {"views": len(cams), "rows": N, "rows_with_pixels": int(keep.sum()), "fraction_rows_with_pixels_eq_0": round(unseen, 4),
                     "fraction_rows_with_radius_eq_0_in_view_0": round(float((baked.render(cams[0], pipe, bg)["radii"] == 0).sum()) / N, 4),
                     "bake_bytes_before": baked.nbytes, "bake_bytes_after_select_rows": small.nbytes,
                     "bake_bytes_formula_after": P.bake_bytes(small.N, T_BAKED, baked.head_on)}
    one = P.contribution(baked, cams[warmup:warmup + 1], pipe, bg)
    doc["saving"]["fraction_rows_with_pixels_eq_0_in_one_view"] = round(1.0 - float(one.keep_mask().sum()) / N, 4)
    # (a row that only ever ENDS saturated pixels is not blended and is dropped: those pixels go on to the next entry, see select_rows)
    a, b = small.render(cams[warmup], pipe, bg)["render"], baked.render(cams[warmup], pipe, bg)["render"]
    doc["saving"]["tool_view_after_select_rows"] = {"pixels_that_differ": int((a != b).any(0).sum()), "pixels": W * H,
                                                    "max_abs_difference": float((a - b).abs().max())}
    print(f"[contrib_timing] {name} saving: {json.dumps(doc['saving'])}", flush=True)
    del small

    # the yardstick: the blending backward of training frames of the same model at the same views
    target = torch.rand(3, H, W, device=dev)

    def train():
        for c in cams[warmup:warmup + TRAIN_VIEWS]:
            res = fdgs.render(c, pc, pipe, bg, stage="fine")
            (res["render"] * target).sum().backward()
        torch.cuda.synchronize()
    train()                                                            # (the first frames size the buffers)
    ttable = kernel_table(train)
    bwd = ttable.get("render_bwd")
    if bwd and "render_contrib" in kernels and "render_fwd" in kernels:
        doc["render_bwd_of_training_frames"] = {"launches": bwd["launches"], "kernel_ms_mean": round(bwd["ms"] / max(bwd["launches"], 1), 5),
                                                "views": TRAIN_VIEWS}
        doc["contrib_over_bwd"] = round(kernels["render_contrib"]["kernel_ms_mean"] / doc["render_bwd_of_training_frames"]["kernel_ms_mean"], 4)
        doc["contrib_over_fwd"] = round(kernels["render_contrib"]["kernel_ms_mean"] / kernels["render_fwd"]["kernel_ms_mean"], 4)
        doc["yardstick"] = "render_contrib kernel time <= the render_bwd kernel time of training frames of the same scene and views"
    print(f"[contrib_timing] {name} kernels: {json.dumps(kernels)} render_bwd: {json.dumps(doc.get('render_bwd_of_training_frames'))} "
          f"contrib_over_bwd = {doc.get('contrib_over_bwd')}", flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib_timing.json"))
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
    doc = {"what": "Baked.render against Baked.render_contrib, same process per configuration, HIP-event median per frame; the render_fwd / "
                   "render_contrib rows of fdgs_timing_report over the same frames and the render_bwd row of training frames at the same "
                   "views; the rows no view shows and the bake's bytes before and after select_rows; tools/contrib_timing.py", "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("cfg2_dnerf_100k_800x800", "cfg4_dynerf_300k_1352x1014"):
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--config", name, "--out", part,
                   "--frames", str(args.frames), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
            rc = subprocess.call(cmd)
            if rc != 0:          # a failed or hung step: nothing more is started on the device
                print(f"[contrib_timing] {name}: exit status {rc}; stopping", flush=True)
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
