# Round-3 evidence, run on the GPU box: bash tools/profile_round3.sh   (-> gpurun_out/r03_*, copy into profiles/)
#   1. rocprofv3 --kernel-trace --stats of the default bench command -> r03_kernel_stats.csv, r03_step_dump.txt
#   2. HBM traffic per kernel (separate --pmc FETCH_SIZE / WRITE_SIZE passes) -> r03_pmc_traffic.{json,_summary.txt}
#   3. matrix-pipe / LDS counters of the shipped kernels -> r03_pmc_mfma_lds.txt
#   4. the bench lines (c2 with roofline + cpu_baseline, c3, c4, c5 bf16 / fp8)
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=gpurun_out
OUT=$O/prof_r03; rm -rf $OUT; mkdir -p $OUT
STEPS=50; WARM=5
rocprofv3 --kernel-trace --stats -d $OUT -o t -- python bench.py --steps $STEPS --warmup $WARM --no-cpu-baseline --no-roofline > $OUT/bench.log 2>&1 || true
DB=$(ls $OUT/*.db $OUT/*/*.db 2>/dev/null | head -1)
python tools/rocprof_summary.py $DB $O/r03_kernel_stats.csv $((STEPS + WARM + 2))
python tools/step_dump.py $DB > $O/r03_step_dump.txt
rm -rf $OUT
STEPS=6 bash tools/pmc_step.sh > $O/r03_pmc_step.log 2>&1 || true
cp $O/pmc_step/pmc_traffic.json $O/r03_pmc_traffic.json
cp $O/pmc_step/summary.txt $O/r03_pmc_traffic_summary.txt
rm -rf $O/pmc_step/FETCH_SIZE $O/pmc_step/WRITE_SIZE
mkdir -p profiles && cp $O/r03_pmc_traffic.json profiles/r03_pmc_traffic.json     # bench.py reads it from profiles/
TAG=r03 STEPS=6 bash tools/pmc_mfma.sh > $O/r03_pmc_mfma.log 2>&1 || true
rm -rf $O/pmc_mfma
python bench.py --full --steps 100 --warmup 10 2>/dev/null | tail -1 > $O/r03_bench_c2.json
python bench.py --full --steps 100 --warmup 10 --config c3 --no-cpu-baseline 2>/dev/null | tail -1 > $O/r03_bench_c3.json
python bench.py --full --steps 100 --warmup 10 --config c4 --no-cpu-baseline 2>/dev/null | tail -1 > $O/r03_bench_c4_1gpu.json
python bench.py --full --steps 30 --warmup 5 --config c5 --no-cpu-baseline 2>/dev/null | tail -1 > $O/r03_bench_c5_fp8.json
python bench.py --full --steps 30 --warmup 5 --config c5 --dtype bf16 --no-cpu-baseline 2>/dev/null | tail -1 > $O/r03_bench_c5_bf16.json
head -30 $O/r03_kernel_stats.csv; tail -3 $O/r03_pmc_traffic_summary.txt; tail -25 $O/r03_pmc_mfma_lds.txt; python -c "
import json
for n in ('c2','c3','c4_1gpu','c5_fp8','c5_bf16'):
    d=json.load(open('$O/r03_bench_%s.json'%n)); print(n, round(d['ms_per_step'],3), round(d['value']), (d.get('roofline') or {}).get('encoder_block',{}).get('mfma_frac'))
"
