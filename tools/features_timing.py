#!/usr/bin/env python
"""tools/features_timing.py -- what the feature pass costs on top of a baked playback frame, on BASELINE configs 2 and 4:

    cfg2  dnerf_bouncingballs, 100 k Gaussians, 800 x 800          cfg4  dynerf_default, 300 k Gaussians, 1352 x 1014

The model is the bench's (SynthModel, seed 6666, Hilbert order, 32 baked timestamps), the cameras are the video orbit, every frame at a
baked timestamp.  Per configuration, as medians of HIP-event times over --frames frames (>= 30) after --warmup frames, one event pair per
frame, in --rounds rounds that alternate the routes (reported one by one: their difference is the run-to-run spread):

    render          Baked.render, the frame alone
    features_C      Baked.render_features with C = 3, 8, 16, 32 channels: the frame, then ONE fdgs_render_features over the frame's own lists
    recC_C          the route there was before: the same forward-only frame, then ceil(C / 3) x (three channels copied into recC, one
                    fdgs_render_fwd over the frame's own lists with a zero background).  The values are handed over in the stored row
                    order already, and the frame's colours are gone afterwards

plus the library's own per-kernel times (fdgs_timing_report, per launch) over the frames of each features_C and recC_C leg: the
`render_fwd` and `render_features` rows.  Nothing here is a pass or fail condition.

Every configuration is measured by a child process of its own under `timeout` (a step that hangs ends there and nothing is started after
a step that failed); this process never opens the device.  Writes profiles/features_timing.json.  (GPU)"""
import argparse
import ctypes
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
CHANNELS = (3, 8, 16, 32)
ROWS = ("render_fwd", "render_features", "tile_order", "preprocess_fwd")


def measure(name, frames, warmup, rounds):
    import numpy as np
    import torch
    from playback_timing import CONFIGS, T_BAKED, kernel_table, row, timed

    fdgs = importlib.import_module("4dgaussians_amd")
    P, syn, L = fdgs.playback, fdgs.synthetic, fdgs._lib
    N, W, H, dcfg = CONFIGS[name]
    dev = torch.device("cuda:0")
    pc = syn.SynthModel(N, dcfg, seed=6666, device=dev)
    fdgs.densify.spatial_reorder(pc, curve="hilbert")
    pipe, bg, zero = syn.PipelineParams(), torch.zeros(3, device=dev), torch.zeros(3, device=dev)
    times = [float(t) for t in np.linspace(0.0, 1.0, T_BAKED)]
    total = warmup + frames
    thetas = np.linspace(-180, 180, total + 1)[:-1]
    cams = [syn.make_camera(W, H, float(th), times[k % T_BAKED]).to(dev) for k, th in enumerate(thetas)]
    baked = P.bake(pc, times)
    values = torch.randn(N, max(CHANNELS), generator=torch.Generator().manual_seed(3)).to(dev)
    stored = values if baked._maps[0] is None else baked._maps[0](values)
    per_c = {c: (values[:, :c].contiguous(), stored[:, :c].contiguous()) for c in CHANNELS}

    def recC_route(cam, c):
        """The forward-only frame, then its blend again per three channels with those channels as the colour record."""
        with torch.no_grad():
            settings, t = P._renderer._frame_settings(cam, None, bg, 1.0, baked.active_sh_degree, dev, pipe)
            out, st = P._state_frame(baked.state_at(t)[0], settings, *baked._maps, None, None)
            q = ctypes.c_void_p()
            L.check(L.lib().fdgs_geom_field(L.ptr(st.geom), N, 3, q))
            off = q.value - st.geom.data_ptr()
            recC = st.geom[off:off + 16 * N].view(torch.float32).view(N, 4)
            p2 = L.RasterParams.from_buffer_copy(st.params)
            p2.bg, p2.acc_zero = L.ptr(zero), None
            planes = torch.empty((c + 2) // 3 * 3, H, W, device=dev)
            vals = per_c[c][1]
            for c0 in range(0, c, 3):
                k = min(3, c - c0)
                if k < 3:
                    recC[:, :3] = 0.0
                recC[:, :k] = vals[:, c0:c0 + k]
                L.check(L.lib().fdgs_render_fwd(L.stream_ptr(), p2, L.ptr(st.geom), L.ptr(st.binning), L.ptr(st.img), st.capacity,
                                                L.ptr(planes[c0:c0 + 3]), L.ptr(out["depth"])))
            return planes[:c]

    legs = {"render": [lambda cam=cam: baked.render(cam, pipe, bg) for cam in cams]}
    for c in CHANNELS:
        legs[f"features_{c}"] = [lambda cam=cam, c=c: baked.render_features(cam, pipe, bg, per_c[c][0]) for cam in cams]
        legs[f"recC_{c}"] = [lambda cam=cam, c=c: recC_route(cam, c) for cam in cams]
    same = {c: bool(torch.equal(legs[f"features_{c}"][3]()["features"], legs[f"recC_{c}"][3]())) for c in CHANNELS}
    doc = {"N": N, "W": W, "H": H, "deformation": dcfg, "timestamps": T_BAKED, "frames": frames, "warmup": warmup, "channels": list(CHANNELS),
           "device": torch.cuda.get_device_name(0), "rounds": [], "features_equal_the_recC_route_bit_for_bit": same}
    for r in range(rounds):
        leg = {k: row(*timed(calls, warmup)) for k, calls in legs.items()}
        for c in CHANNELS:
            leg[f"features_{c}_minus_render_ms"] = round(leg[f"features_{c}"]["median_ms"] - leg["render"]["median_ms"], 4)
            leg[f"recC_{c}_minus_render_ms"] = round(leg[f"recC_{c}"]["median_ms"] - leg["render"]["median_ms"], 4)
        doc["rounds"].append(leg)
        print(f"[features_timing] {name} round {r}: render {leg['render']['median_ms']:.4f} ms; extra per frame, features / recC route: "
              + ", ".join(f"C={c}: {leg[f'features_{c}_minus_render_ms']:.4f} / {leg[f'recC_{c}_minus_render_ms']:.4f} ms" for c in CHANNELS),
              flush=True)
    doc["kernels"] = {}
    for k, calls in legs.items():
        if k == "render":
            continue
        timed_calls = calls[warmup:]
        table = kernel_table(lambda: [f() for f in timed_calls])
        doc["kernels"][k] = {n: {"launches_per_frame": round(v["launches"] / len(timed_calls), 3),
                                 "kernel_ms_mean": round(v["ms"] / max(v["launches"], 1), 5),
                                 "kernel_ms_per_frame": round(v["ms"] / len(timed_calls), 5)} for n, v in table.items() if n in ROWS}
    for c in CHANNELS:
        f, o = doc["kernels"][f"features_{c}"], doc["kernels"][f"recC_{c}"]
        if "render_features" in f and "render_fwd" in f and "render_fwd" in o:
            extra_blends = o["render_fwd"]["kernel_ms_per_frame"] - f["render_fwd"]["kernel_ms_per_frame"]
            doc[f"C{c}"] = {"render_features_kernel_ms": f["render_features"]["kernel_ms_mean"],
                            "render_fwd_kernel_ms": f["render_fwd"]["kernel_ms_mean"],
                            "extra_render_fwd_kernel_ms_of_the_recC_route": round(extra_blends, 5),
                            "features_over_one_blend": round(f["render_features"]["kernel_ms_mean"] / f["render_fwd"]["kernel_ms_mean"], 4)}
    print(f"[features_timing] {name} kernels: {json.dumps({f'C{c}': doc.get(f'C{c}') for c in CHANNELS})}", flush=True)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_timing.json"))
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
    doc = {"what": "Baked.render against Baked.render_features at C = 3, 8, 16, 32 and against the recC route (ceil(C/3) x (rewrite recC + "
                   "fdgs_render_fwd)), same process per configuration, HIP-event median per frame, and the render_fwd / render_features rows "
                   "of fdgs_timing_report over the same frames; tools/features_timing.py", "configs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("cfg4_dynerf_300k_1352x1014", "cfg2_dnerf_100k_800x800"):
            part = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--config", name, "--out", part,
                   "--frames", str(args.frames), "--warmup", str(args.warmup), "--rounds", str(args.rounds)]
            rc = subprocess.call(cmd)
            if rc != 0:          # a failed or hung step: nothing more is started on the device
                print(f"[features_timing] {name}: exit status {rc}; stopping", flush=True)
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
