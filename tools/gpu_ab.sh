# A/B of env-selected schedules on one box: bench (no CPU baseline) once per setting.
#   gpurun -- bash tools/gpu_ab.sh "VAR=a" "VAR=b" ...
set -e
R=$GRAFT_REPO_ROOT
cd $R
O=${TFUSION_OUT:-out}/ab      # TFUSION_OUT: the folder that collects the logs
mkdir -p $O
i=0
for setting in "$@"; do
  i=$((i+1))
  env $setting timeout -k 10 300 python bench.py --full --steps 300 --warmup 20 --no-cpu-baseline > $O/$i.log 2>&1 || { tail -20 $O/$i.log; exit 1; }
  python -c "import json,sys; d=json.loads(open('$O/$i.log').read().strip().splitlines()[-1]); print('$setting', d['value'], d['stage_ms_per_frame'])"
done
