# tools/frame_timeline.sh -- rocprofv3 --kernel-trace of a short bench run -> $OUT_DIR/r05x_frame_timeline_cfg4.txt (tools/frame_timeline.py)
R=${REPO_ROOT:-$(pwd)}; O=${OUT_DIR:-$R/tools_out}; mkdir -p $O; cd $R
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace -d $O/tl_prof -o trace --output-format csv -- python $R/bench.py --full --steps 20 --warmup 6 --repeats 2 --no-cpu-baseline --no-extras > $O/tl_bench.json 2> $O/tl.err
cd $R
python tools/frame_timeline.py $O/tl_prof $O/r05x_frame_timeline_cfg4.txt
rm -rf $O/tl_prof
python -c "
import json; d=json.load(open('$O/tl_bench.json')); print(d['value'], d['ms_per_step'], d['kernels_ms_per_step'])"
