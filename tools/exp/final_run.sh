set -x
OUT=${OUT:-$(pwd)/out}
mkdir -p $OUT
bash tools/make_profiles.sh r04 > $OUT/make_profiles.log 2>&1
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
tail -c 600 $OUT/bench_default.err
