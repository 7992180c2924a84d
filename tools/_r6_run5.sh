O=${OUT_DIR:-tools_out}
mkdir -p $O
timeout 1500 python -m pytest tests/test_gpu_fullsize.py tests/test_gpu_render_branches.py -x -q -m gpu > $O/t5.log 2>&1; echo "rc=$?" >> $O/t5.log
tail -12 $O/t5.log
python bench.py --full --steps 20 --warmup 5 > $O/bench_io.json 2> $O/bench_io.err
python - <<PY
import json
d=json.loads(open("$O/bench_io.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["avg_launch_ms"], d["roofline"]["frac"])
for k in ("random_order","random_order_implicit_permutation_off","shell_scene","all_tiles_backward"):
    print(k, {kk:vv for kk,vv in d[k].items() if kk in ("frames_per_s","ms_per_step","kernels_ms_per_step")})
PY
