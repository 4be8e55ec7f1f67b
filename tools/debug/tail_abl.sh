#!/bin/bash
# What the four small products (h2, logits, d_z2, d_z1) cost inside tail_dx_train_kernel at c2: kernel stats of the plain bench
# command with the timing-only knob NNUE_CLS_ABL_SKIP_TAIL_PRODUCTS off and on (two profiles per setting: the spread between
# profiles of identical code), then the kernel's phase clocks with it off and on.  Needs a library built with
# NNUE_BUILD_ABLATIONS=1 (python nnue-vision_amd/csrc/build.py --force).  Usage: bash tools/debug/tail_abl.sh OUTDIR
set -o pipefail
R=$PWD; O=$R/$1; mkdir -p $O; export TMPDIR=/tmp
for n in off_a on_a off_b on_b; do
  case $n in on_*) k=1;; *) k=0;; esac
  NNUE_CLS_ABL_SKIP_TAIL_PRODUCTS=$k timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt_$n -- \
    python3 $R/bench.py --gpus 1 > $O/$n.json 2> $O/$n.err || { echo "$n failed: $(tail -3 $O/$n.err)"; exit 1; }
  f=$(find $O/kt_$n -name '*kernel_stats.csv' | head -1)
  cp $f $O/kernel_stats_$n.csv
  echo "$n $(grep -o '"ms_per_step": [0-9.]*' $O/$n.json) tail_dx_train_kernel average ns: $(grep tail_dx_train_kernel $f | awk -F, '{print $(NF-4)}')"
done
for k in 0 1; do
  NNUE_CLS_ABL_TAIL_CLOCKS=1 NNUE_CLS_ABL_SKIP_TAIL_PRODUCTS=$k timeout -k 10 150 python3 $R/tools/debug/tail_clocks.py c2 12 | tee $O/clocks_skip$k.txt || exit 1
done
