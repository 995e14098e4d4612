cd $GRAFT_REPO_ROOT
show() { python -c "
import json,sys
j=json.load(open('$1'))
p=j['pcie_inclusive']
print('$2', 'both', round(p['value']/1e6,1), 'single', round(p['single_call']['value']/1e6,1), 'dist', round(p['distances_only']['value']/1e6,1))
"; }
T=$(mktemp -d)
python bench.py --full --no-cpu-baseline > $T/b1.json 2>/dev/null; show $T/b1.json no-cpu-baseline
python bench.py --full > $T/b2.json 2>/dev/null; show $T/b2.json with-cpu-baseline
OMP_WAIT_POLICY=passive python bench.py --full > $T/b3.json 2>/dev/null; show $T/b3.json with-cpu-baseline-passive
