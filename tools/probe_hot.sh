cp h264-fer_amd/libferhip.so /tmp/keep.so
cp h264-fer_amd/var/libferhip_probe.so h264-fer_amd/libferhip.so
export OUT=${OUT:-bench_out}; mkdir -p $OUT   # where the bench lines go
for dbg in 0 512; do
FER_DBG=$dbg python bench.py --full --streams 128 --contexts 1 --steps 1 --warmup 1 --cpu-frames 0 --secondary 0 --e2e 0 --resolve-group 16 --probe-build 1 > $OUT/pr_$dbg.json 2> $OUT/pr_$dbg.err
done
cp /tmp/keep.so h264-fer_amd/libferhip.so
python - <<'PY'
import json, os
for f in ("pr_0","pr_512"):
    d=json.load(open(os.path.join(os.environ["OUT"], f + ".json"))); k=d["roofline"]["kernels"]
    print(f, d["value"], "resolve", k["me_resolve"]["avg_launch_us"], d["speculation"])
PY
