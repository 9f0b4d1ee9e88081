# same-box A/B of bench.py configurations: tools/ab_bench.sh "ENV1=1" "ENV2=1" ...  (the empty configuration is always included;
# a configuration that restates a default, e.g. "LA_CP_EPI16=0", is the control: the same library state against itself)
# AB_ROUNDS = interleaved rounds (default 3); AB_ARGS = bench.py arguments (default: the --full run this tool always made).
# Every run is a fresh process under a time limit of its own; the first one that fails ends the series.
set -o pipefail
rounds=${AB_ROUNDS:-3}
args=${AB_ARGS:---full --no-cpu-baseline --steps 20 --warmup 3}
for i in $(seq 1 $rounds); do
  for cfg in "" "$@"; do
    echo "== cfg [$cfg] round $i"
    env $cfg timeout -k 10 300 python bench.py $args 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(round(d['ms_per_step'],3), round(d.get('roofline',{}).get('frac',0),4))" || { echo "run failed: series ended"; exit 1; }
  done
done
