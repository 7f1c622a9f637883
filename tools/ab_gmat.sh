# C3 + C5 A/B of the current build against ab/old/libpgamd.so, then a WRITE_SIZE pass of C5: tools/ab_gmat.sh OUT
set -eo pipefail
OUT=$1
mkdir -p "$OUT"
tools/ab_bench.sh "$OUT/c3" mitsuba-path-guiding_amd/build/libpgamd.so ab/old/libpgamd.so --steps 3 --warmup 1
for L in mitsuba-path-guiding_amd/build/libpgamd.so ab/old/libpgamd.so; do
  PG_LIB=$L timeout -k 10 200 python bench.py --scene smoke --steps 2 --warmup 1 --full --no-cpu > "$OUT/c5_$(basename $(dirname $(dirname $L))).log" 2>&1
done
grep -h '"value"' "$OUT"/c5_*.log | python -c "
import sys,json
for l in sys.stdin:
    d=json.loads(l); print('C5', d['value'], d['roofline']['avg_launch_ms'])"
export TMPDIR=/tmp
timeout -s KILL 200 rocprofv3 --pmc WRITE_SIZE -d "$OUT/c5w" -o run --output-format csv -- python3 bench.py --scene smoke --steps 1 --warmup 0 --full --no-cpu > "$OUT/c5w.log" 2>&1
echo done
