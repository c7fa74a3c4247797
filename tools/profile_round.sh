set -e
O=${O:-out}      # output folder
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $O/prof_k
rocprofv3 --kernel-trace --stats -d $O/prof_k -o r01k -- python bench.py --steps 50 --warmup 5 --no-cpu-baseline --no-roofline > $O/prof_k/bench.log 2>&1 || true
DB=$(ls $O/prof_k/*.db $O/prof_k/*/*.db 2>/dev/null | head -1)
echo DB=$DB
python tools/rocprof_summary.py $DB $O/r01_k_kernel_stats.csv 57
python tools/step_timeline.py $DB > $O/r01_k_step_timeline.txt
STEPS=6 bash tools/pmc_step.sh > $O/pmc_step_k.log 2>&1 || true
python bench.py --full --steps 100 --warmup 10 2>/dev/null | tail -1 > $O/r01_k_bench.json
head -12 $O/r01_k_kernel_stats.csv; cat $O/r01_k_step_timeline.txt | head -20; tail -5 $O/pmc_step_k.log
