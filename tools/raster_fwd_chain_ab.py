"""Alternated A/B of the rasterizer forward chain (knobs bin_count, blend_fwd_form) against a build of the parent commit, one bench.py
process per line: the method of profiles/raster_fwd_chain_ab.txt.  Legs: p = tools/_variants/libfdgs_parent.so (libfdgs.so built from a
checkout of the parent commit, loaded through FDGS_LIB), a = bin_count 1 only, b = blend_fwd_form 1 only, ab = both, o = both off (config 4), a2 = bin_count 2 (config 5);
AB_LEGS=p,ab,... picks other legs.  Output: tools_out/raster_fwd_chain_ab_TAG.txt.  (development, GPU)
usage: python tools/raster_fwd_chain_ab.py TAG ROUNDS SHAPE [SHAPE ...]      SHAPE = cfg4 | shell | cfg2 | cfg3 | cfg5"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "tools", "_variants", "libfdgs_parent.so")
SHAPES = {
    "cfg4": [], "shell": ["--scene", "shell"], "cfg2": ["--workload", "cfg2_dnerf_100k_800x800"],
    "cfg3": ["--workload", "cfg3_hypernerf_300k_536x960"], "cfg5": ["--workload", "cfg5_stress_2M_2048x2048"],
}
LEGS = {
    "p": ("parent commit", {"FDGS_LIB": PARENT}),
    "a": ("this change, bin_count 1 blend_fwd_form 0", {"FDGS_BIN_COUNT": "1", "FDGS_BLEND_FWD_FORM": "0"}),
    "b": ("this change, bin_count 0 blend_fwd_form 1", {"FDGS_BIN_COUNT": "0", "FDGS_BLEND_FWD_FORM": "1"}),
    "ab": ("this change, bin_count 1 blend_fwd_form 1", {"FDGS_BIN_COUNT": "1", "FDGS_BLEND_FWD_FORM": "1"}),
    "a2": ("this change, bin_count 2 blend_fwd_form 0", {"FDGS_BIN_COUNT": "2", "FDGS_BLEND_FWD_FORM": "0"}),
    "o": ("this change, bin_count 0 blend_fwd_form 0", {"FDGS_BIN_COUNT": "0", "FDGS_BLEND_FWD_FORM": "0"}),
}


def main():
    tag, rounds, shapes = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    os.makedirs(os.path.join(ROOT, "tools_out"), exist_ok=True)
    out = open(os.path.join(ROOT, "tools_out", f"raster_fwd_chain_ab_{tag}.txt"), "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    for shape in shapes:
        legs = ["p", "a", "b", "ab"] + (["a2"] if shape == "cfg5" else []) + (["o"] if shape == "cfg4" else [])
        if os.environ.get("AB_LEGS"):
            legs = os.environ["AB_LEGS"].split(",")
        args = ["--gpus", "1", "--repeats", "0", "--steps", "40", "--warmup", "8"] + SHAPES[shape]
        say(f"# bench.py {' '.join(args)}   (" + ", ".join(f"{k} = {LEGS[k][0]}" for k in legs) + ")")
        fps = {k: [] for k in legs}
        for r in range(1, rounds + 1):
            for k in legs:
                env = dict(os.environ)
                env.update(LEGS[k][1])
                p = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
                if p.returncode != 0:
                    say(f"{k} {r} FAILED rc={p.returncode}: {p.stderr[-400:]}")
                    return 1          # nothing more on this GPU after a failure
                d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
                fps[k].append(d["value"])
                say(f"{k} {r} {d['value']:.2f} frames/s  {d['ms_per_step']:.4f} ms  p10 {d['p10_ms_per_step']:.4f} p90 {d['p90_ms_per_step']:.4f}  regions {d['timed_regions']}")
        for k in legs:
            v = fps[k]
            say(f"= {k} median {statistics.median(v):.2f}  min {min(v):.2f}  max {max(v):.2f}  max-min {max(v) - min(v):.2f} frames/s over {len(v)} runs")
        base, bar = statistics.median(fps["p"]), max(fps["p"]) - min(fps["p"])
        for k in legs[1:]:
            d = statistics.median(fps[k]) - base
            say(f"= {k} - p = {d:.2f} frames/s ({100 * d / base:.2f} %); bar = p's max - min = {bar:.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
