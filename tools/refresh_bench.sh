# The default bench line (with the CPU baseline), the two T-path workloads and the one-sample-per-call shapes.
# usage (on the GPU box): bash tools/refresh_bench.sh <outdir>
O=${1:?usage: bash tools/refresh_bench.sh <outdir>}
mkdir -p $O
timeout 280 python bench.py --full --steps 100 > $O/bench_default.json 2> $O/bench_default.err
timeout 200 python bench.py --full --steps 100 --workload cfg3_t --no-cpu-baseline > $O/bench_cfg3_t.json 2>> $O/bench_default.err
timeout 200 python bench.py --full --steps 100 --workload cfg5_t --batch 2 --no-cpu-baseline > $O/bench_cfg5_t.json 2>> $O/bench_default.err
timeout 200 python bench.py --full --steps 100 --batch 1 --no-cpu-baseline > $O/bench_batch1.json 2>> $O/bench_default.err
timeout 200 python bench.py --full --steps 100 --batch 1 --inflight 1 --no-cpu-baseline > $O/bench_single.json 2>> $O/bench_default.err
tail -c 600 $O/bench_default.err
