#!/bin/bash
# Closing measurements of a round: the whole bench line (bench.py --full), kernel stats of
# the bench step, the 4-bit beam, and one rank's time slice alone at G = 2 / 8 (ranks 0 and 7).
# Logs under $OUT (default: out, relative to the repository root).
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p "$OUT"
timeout -k 10 600 python3 bench.py --full > $OUT/fin_bench.log 2>&1 || { echo "bench failed"; tail -20 $OUT/fin_bench.log; exit 1; }
tail -1 $OUT/fin_bench.log | cut -c1-300
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/fin_prof -o run -- python3 bench.py --steps 3 --warmup 1 \
    > $OUT/fin_prof.log 2>&1 || { echo "prof failed"; tail -20 $OUT/fin_prof.log; exit 1; }
python3 scripts/kstats.py "$(find $OUT/fin_prof -name '*.db' | head -1)" $OUT/fin_kstats.csv
head -20 $OUT/fin_kstats.csv | cut -c1-150
timeout -k 10 300 python3 bench.py --nbits 4 --steps 5 --warmup 2 > $OUT/fin_4bit.log 2>&1 \
    || { echo "4-bit failed"; tail -5 $OUT/fin_4bit.log; exit 1; }
echo "4-bit: $(python3 scripts/benchline.py $OUT/fin_4bit.log)"
rm -f $OUT/fin_simslice.jsonl
for s in 0/2 0/8 7/8; do
  timeout -k 10 300 python3 bench.py --mode slices --sim-slice $s --steps 5 --warmup 2 > $OUT/fin_sim.log 2>&1 \
      || { echo "sim-slice $s failed"; tail -5 $OUT/fin_sim.log; exit 1; }
  echo "sim-slice $s: $(python3 scripts/benchline.py $OUT/fin_sim.log)"
  tail -1 $OUT/fin_sim.log >> $OUT/fin_simslice.jsonl
done
echo "final done"
