#!/bin/bash
# Run on an MI355X box: rocprofv3 kernel stats + HBM traffic counters for the bench workload (bench.py --full: every leg of the line).
# Usage: bash scripts/collect_profiles.sh <tag> [<output dir>]     (outputs under <output dir>/<tag>_*, default profile_out/)
TAG=${1:-r01}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${2:-$R/profile_out}")
cd /tmp && export TMPDIR=/tmp
mkdir -p $O
python3 $R/bench.py --full --steps 5 --warmup 2 > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err
rocprofv3 --kernel-trace --stats --output-format csv -d $O/${TAG}_stats -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-other-configs > $O/${TAG}_bench_under_rocprof.json 2>/dev/null
# counters in their own passes (kernel-trace only), as the microarch guide prescribes
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/${TAG}_pmc_fetch -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-other-configs > /dev/null 2>&1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/${TAG}_pmc_write -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-other-configs > /dev/null 2>&1
python3 $R/scripts/parse_traffic.py $O ${TAG}
