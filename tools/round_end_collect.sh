#!/bin/bash
# Round-end collection (run ON the GPU box, repo root): full GPU suite, smoke, default bench, the secondary NB bench lines, workspace-kernel
# timing and the shim sweeps; summaries land in $O/profiles_out/ (O defaults to build/round_end; copy them into profiles/).
set -o pipefail
O=${1:-build/round_end}
mkdir -p $O/profiles_out
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $O/t_full.log 2>&1; tail -3 $O/t_full.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -2
python bench.py --full > $O/profiles_out/default_bench.json 2> $O/default_bench.err; python -c "import json;j=json.load(open('$O/profiles_out/default_bench.json'));print('default', j['value'], j['roofline']['frac'], j['cpu_baseline']['value'])"
for w in NB_N96_GF256 NB_BDS_GF64_TMM NB_BDS_GF64_LTMM; do python bench.py --full --workload $w > $O/profiles_out/r03_${w}_bench.json 2>/dev/null; python -c "import json;j=json.load(open('$O/profiles_out/r03_${w}_bench.json'));print('$w', j['value'])"; done
python tools/nb_hbm_time.py > $O/profiles_out/r03_nb_hbm_time.txt 2>&1; tail -2 $O/profiles_out/r03_nb_hbm_time.txt
bash tools/shim_sweep_time.sh > $O/profiles_out/r03_shim_sweep.txt 2>&1; grep "^real" $O/profiles_out/r03_shim_sweep.txt
rm -rf gpurun_out/shim_bin
