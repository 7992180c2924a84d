O=${OUT_DIR:-tools_out}
mkdir -p $O
timeout 900 python -m pytest tests/test_gpu_raster.py tests/test_zz_gpu_reference_train_step.py -x -q -m gpu -s > $O/t3.log 2>&1; echo "rc=$?" >> $O/t3.log
tail -15 $O/t3.log
for m in auto capacity exact; do FDGS_BINNING=$m timeout 600 python bench.py --full --steps 20 --warmup 5 > $O/bench_$m.json 2> $O/bench_$m.err; echo "$m rc=$?"; done
O=$O python - <<'PY'
import json, os
for m in ("auto","capacity","exact"):
    try:
        d=json.loads(open(os.environ["O"] + f"/bench_{m}.json").read().strip().splitlines()[-1])
        print(m, d["value"], d["ms_per_step"], d["binning"]["mode"], d["binning"]["capacity_reruns"], d.get("roofline"))
    except Exception as e: print(m, "ERR", e)
PY
