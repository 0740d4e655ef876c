set -x
OUT=${OUT:-$(pwd)/out/final}
mkdir -p $OUT
R=$GRAFT_REPO_ROOT
timeout 1500 python -m pytest tests -m gpu -q 2>&1 | tail -8 > $OUT/pytest_gpu.txt
timeout 600 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_fp32 -o run -- python $R/bench.py --steps 3 --warmup 1 --skip-cpu --skip-roofline --skip-secondary --no-settle > $OUT/prof_fp32.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_bf16 -o run -- python $R/bench.py --dtype bf16 --imsize 224 --steps 3 --warmup 1 --skip-cpu --skip-roofline --skip-secondary --no-settle > $OUT/prof_bf16.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_roof -o run -- python $R/bench.py --roofline-only > $OUT/prof_roof.log 2>&1
cd $R
cat $OUT/pytest_gpu.txt
cut -c1-300 $OUT/bench_default.json
