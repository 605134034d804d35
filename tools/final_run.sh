#!/bin/bash
# ON THE GPU BOX: what is run on the final sources of a round -- the whole GPU test suite, the round's profile set
# (tools/profiles.sh), clean bench lines of every configuration, the randomized parity sweep.  Results land in $OUT/;
# summarise locally with tools/summarize_prof.py and copy what is to be judged into profiles/.
cd ${GRAFT_REPO_ROOT:-/root/repo}
OUT=${OUT:-tool_out}; mkdir -p "$OUT"        # output folder (git-ignored default)
(timeout 3000 python -m pytest tests -m gpu -q -rA 2>&1 | grep -E "passed|failed|error|config5 chain" | tail -6) > $OUT/r06_pytest_gpu.txt
tools/profiles.sh r06 > $OUT/r06_profiles.log 2>&1
( time python bench.py --full ) > $OUT/r06f_bench.json 2> $OUT/r06f_bench.err
python bench.py --full --steps 10 --warmup 3 --scene bistro --voxel-dim 1024 --width 3840 --height 2160 --cpu-seconds 0 > $OUT/r06f_c5_bench.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --voxel-dim 512 --width 3840 --height 2160 --bounces 2 --cpu-seconds 0 --no-sweep > $OUT/r06f_c3_bench.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --scene bistro --cpu-seconds 0 --no-sweep > $OUT/r06f_bistro1080_bench.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --scene atrium-textured --cpu-seconds 0 --no-sweep > $OUT/r06f_tex_bench.json 2>/dev/null
if [ -z "$SKIP_FUZZ" ]; then
  ( FUZZ_SEED0=400000 python tools/fuzz_gpu.py 600 ; FUZZ_SEED0=400000 python tools/fuzz_gpu.py 900 big ) > $OUT/r06_fuzz.txt 2>&1
  tail -3 $OUT/r06_fuzz.txt
fi
tail -4 $OUT/r06f_bench.err
