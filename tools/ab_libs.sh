#!/bin/bash
# A/B of library variants on the train step and DDIM-100 sampling: tools/ab_libs.sh default h1 h4 ...   (two rounds each)
for round in 1 2; do
for v in "$@"; do
  if [ "$v" = default ]; then unset IDF_LIB; else export IDF_LIB=$PWD/infodiffusion_amd/variants/libinfodiff_hip_$v.so; fi
  python bench.py --steps 30 --warmup 5 --full --no-cpu-baseline --no-roofline --no-large-batch 2>/dev/null | tail -1 > /tmp/_ab.json
  python - "$v" <<'PY'
import json, sys
d = json.load(open('/tmp/_ab.json'))
print('%-8s ms/step %.3f median %.3f  sampling %.1f img/s' % (sys.argv[1], d['ms_per_step'], d['ms_per_step_median'], d['sampling']['value']))
PY
done
done
