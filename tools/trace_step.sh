#!/bin/bash
# usage (GPU box): tools/trace_step.sh <tag>  -> $PROFILE_OUT/<tag>_trace/ (default bench_out/) + report on stdout
set -e
export TMPDIR=/tmp
out=${PROFILE_OUT:-bench_out}
mkdir -p "$out"
timeout -k 10 180 rocprofv3 --kernel-trace --output-format csv -d $out/$1_trace -o run -- \
  python bench.py --full --no-cpu-baseline --no-roofline --steps 20 > $out/$1_trace.log 2>&1
python tools/trace_report.py $out/$1_trace/run_kernel_trace.csv 12 > $out/$1_trace_report.md
cat $out/$1_trace_report.md
