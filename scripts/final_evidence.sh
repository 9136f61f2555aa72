#!/bin/bash
# evidence on the final tree of a round (run on an MI355X box):  bash scripts/final_evidence.sh <tag> [<output dir>]   (default profile_out/)
TAG=${1:-r05z}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${2:-$R/profile_out}")
cd $R
mkdir -p $O
python -m pytest tests -q -m gpu -x 2>&1 | tail -5 > $O/${TAG}_gputests.txt
bash scripts/collect_profiles.sh $TAG $O > $O/${TAG}_collect.log 2>&1
python tests/tools/parity_families.py > $O/${TAG}_parity.log 2>&1
python scripts/parity_report.py > $O/${TAG}_parity_report.log 2>&1
{ python scripts/other_configs.py; python scripts/eat_bench.py; python scripts/effnet_bench.py 256; python scripts/effnet_bench.py 1024; python scripts/aves_bench.py 128; } 2>&1 | grep -v amdgpu.ids > $O/${TAG}_other_configs.txt
python tests/tools/fuzz_kernels.py 300 41 > $O/${TAG}_fuzz_kernels.txt 2>&1
python tests/tools/fuzz_e2e.py 150 23 > $O/${TAG}_fuzz_e2e.txt 2>&1
python scripts/soak.py 90 > $O/${TAG}_soak.txt 2>&1
cat $O/${TAG}_gputests.txt
tail -qn 2 $O/${TAG}_fuzz_kernels.txt $O/${TAG}_fuzz_e2e.txt $O/${TAG}_soak.txt
cat $O/${TAG}_other_configs.txt
cat $O/${TAG}_bench.json
