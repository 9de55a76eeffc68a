#!/bin/bash
# usage: tools/ab_bench.sh OUT_DIR "ENV1" "ENV2" ... ; each run: bench --full --no-cpu-baseline, its line in OUT_DIR/r<i>.json
out=$1; shift
mkdir -p "$out"
i=0
for e in "$@"; do
  i=$((i+1))
  env $e timeout 200 python bench.py --full --no-cpu-baseline 2>/dev/null | tail -1 > "$out/r$i.json"
  python - "$e" "$out/r$i.json" <<'PY'
import json,sys
d=json.loads(open(sys.argv[2]).read()); g=d["gpu_ms"]
print(sys.argv[1], "step", d["ms_per_step"], "ray", g["raymarch"], "chg", g["change_dir_light"], "unc", g["change_dir_light_uncached"], "cold", g["reset_all_lights_cold"], "warm", g["reset_all_lights_warm"], "win", g["window_sweep_step"])
PY
done
