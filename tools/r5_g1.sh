set -x
O=${O:-out}      # output folder
mkdir -p $O/r5
python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > $O/r5/g1_pytest.log
python tools/torch_ops_in_step.py > $O/r5/g1_torch_ops.log 2>&1
CAPTURE=1 python tools/torch_ops_in_step.py > $O/r5/g1_torch_ops_capture.log 2>&1
tools/ubench/prod > $O/r5/g1_prod.log 2>&1
WHICH=block python tools/bench_fused.py > $O/r5/g1_block.log 2>&1
python bench.py --full --steps 40 --warmup 5 > $O/r5/g1_c2.json 2> $O/r5/g1_c2.err
python bench.py --full --config c5 --dtype bf16 --steps 30 --warmup 5 > $O/r5/g1_c5.json 2> $O/r5/g1_c5.err
