#!/bin/bash
# usage (GPU box): tools/ab_env.sh name:VAR=val,VAR2=val ... -> one short bench per environment
# ("name:" alone = defaults). Prints value + per-kernel us. Extra bench args via $AB_ARGS.
# Logs go to $AB_OUT (default bench_out/).
export AB_OUT=${AB_OUT:-bench_out}
mkdir -p "$AB_OUT"
for spec in "$@"; do
  name=${spec%%:*}; envs=${spec#*:}
  ( IFS=','; for kv in $envs; do [ -n "$kv" ] && export "$kv"; done; unset IFS
    timeout -k 10 150 python bench.py --full --no-cpu-baseline --steps 10 $AB_ARGS > "$AB_OUT/ab_$name.log" 2>&1 ) \
    || { echo "$name failed"; tail -5 "$AB_OUT/ab_$name.log"; exit 1; }
  python - "$name" <<'PY'
import json, os, sys
v = sys.argv[1]
d = json.loads(open(os.path.join(os.environ["AB_OUT"], f"ab_{v}.log")).read().strip().splitlines()[-1])
k = d["kernel_avg_us"] or {}
print(v, d["value"], d.get("dtype"), " ".join(f"{a}={b}" for a, b in sorted(k.items())), flush=True)
PY
done
