set -o pipefail
o=${1:-${TMPDIR:-/tmp}/inflight_sweep}
mkdir -p $o
for n in 12 16 24 28; do
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-lossless --steps 96 --inflight $n > $o/if$n.json 2> $o/if$n.err || exit 1
done
