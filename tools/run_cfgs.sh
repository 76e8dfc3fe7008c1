cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/run_cfgs.sh OUTDIR}; mkdir -p $O
for c in cfg2 cfg3 cfg4 cfg5; do
timeout 300 python bench.py --full --config $c --no-cpu-baseline --no-shard-probe 2>$O/$c.err | tail -1 > $O/$c.json
python -c "
import json; d=json.loads(open('$O/$c.json').read()); print('$c', round(d['ms_per_step'],2),'ms  frac',round(d['roofline']['frac'],3), {k:round(v,2) for k,v in d.get('stages_ms_per_eval',{}).items()})"
done
