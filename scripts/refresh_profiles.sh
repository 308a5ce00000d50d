# end-of-round evidence: rocprofv3 stats + traffic for cfg3, bench lines for cfg3 (--full: with cpu_baseline), cfg2, cfg5
#   bash scripts/refresh_profiles.sh <tag> <output directory>
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r1_v2d}
OUT=${2:?usage: refresh_profiles.sh <tag> <output directory>}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
# kernel stats, then HBM traffic of the same command: FETCH_SIZE in its own pass (3 of the 4 TCC slots), counters only with --kernel-trace
(cd /tmp && export TMPDIR=/tmp
 rm -rf $OUT/prof_$TAG $OUT/pmc_$TAG
 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $R/bench.py --steps 2 --warmup 1 > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_$TAG.err
 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_$TAG -- python3 $R/bench.py --steps 1 --warmup 0 > $OUT/pmc_${TAG}_bench.json 2> $OUT/pmc_$TAG.err
) > $OUT/profile_$TAG.log 2>&1
cd $R
python3 bench.py --full > $OUT/${TAG}_cfg3_bench_with_cpu_baseline.json 2> $OUT/${TAG}_cfg3.err
python3 bench.py --workload cfg2 > $OUT/${TAG}_cfg2_bench.json 2> $OUT/${TAG}_cfg2.err
python3 bench.py --workload cfg5 > $OUT/${TAG}_cfg5_bench.json 2> $OUT/${TAG}_cfg5.err
for n in 2 4 8; do ZR_BENCH_SHARD_OF=$n python3 bench.py 2>/dev/null | python3 -c "import json,sys; d=json.loads(sys.stdin.readline()); print('shard 1/$n ms_per_step', d['ms_per_step'])"; done > $OUT/${TAG}_shards.txt
# compact summaries for profiles/
python3 - "$OUT" "$TAG" <<'PY'
import csv, glob, json, os, sys, collections
OUT, TAG = sys.argv[1:3]
f = sorted(glob.glob(f'{OUT}/prof_{TAG}/*/*kernel_stats.csv'), key=os.path.getmtime)[-1]
open(f'{OUT}/{TAG}_cfg3_kernel_stats.csv', 'w').write(open(f).read())
f = sorted(glob.glob(f'{OUT}/pmc_{TAG}/*/*counter_collection.csv'), key=os.path.getmtime)[-1]
agg = collections.defaultdict(float); n = collections.Counter(); seen = set()
for r in csv.DictReader(open(f)):
    if r['Counter_Name'] != 'FETCH_SIZE': continue
    k = r['Kernel_Name']
    name = 'stream_extend' if 'stream_extend<false' in k else 'stream_shade' if 'stream_shade<false' in k else None
    if not name: continue
    agg[name] += float(r['Counter_Value'])
    key = (name, r['Dispatch_Id'])
    if key not in seen: seen.add(key); n[name] += 1
out = {'workload': 'cfg3', 'command': 'rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -- python3 bench.py --steps 1 --warmup 0',
       'note': 'FETCH_SIZE is reported in KB; on gfx950 it tallies 128-B requests at 64 B, so bytes = 2 x FETCH_SIZE x 1024 (MI355X_MICROARCH.md, HBM section); Infinity-Cache hits are counted, not excluded',
       'kernels': {k: {'launches': n[k], 'FETCH_SIZE_KB_sum': agg[k], 'hbm_read_bytes_per_launch': 2 * 1024 * agg[k] / max(1, n[k])} for k in agg}}
json.dump(out, open(f'{OUT}/{TAG}_cfg3_traffic.json', 'w'), indent=1)
print(json.dumps(out['kernels']))
PY
cat $OUT/${TAG}_shards.txt
tail -1 $OUT/${TAG}_cfg3_bench_with_cpu_baseline.json | cut -c1-200
