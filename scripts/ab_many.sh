#!/bin/bash
# dev tool: compare several builds of libpt_amd.so on the same box, interleaved. usage: ab_many.sh "bench args" a.bin b.bin ...
# Every bench run has a time limit of its own (AB_TIMEOUT seconds, default 300); the first run that fails or is killed ends the comparison:
# nothing is started on a GPU behind a fault.
ARGS=$1; shift
L=single-file-vulkan-pathtracing_amd/libpt_amd.so
cp $L /tmp/keep.so
T=$(mktemp -d)   # this comparison's own bench output
rc=0
for r in $(seq 1 ${AB_ROUNDS:-3}); do
  for B in "$@"; do
    cp $B $L; echo -n "$(basename $B): "
    timeout -k 10 ${AB_TIMEOUT:-300} python bench.py --no-cpu-baseline --no-extra-legs $ARGS 2> $T/err.txt > $T/line.txt; rc=$?
    [ $rc -eq 0 ] || { echo "bench.py ended with status $rc: stopping.  Its last lines:"; tail -5 $T/err.txt; break 2; }
    python -c "
import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d.get('roofline',{}); g=r.get('gather',{}); a=r.get('active_lanes',{})
print(d['value'], d['ms_per_step'], 'nodes/ray', g.get('bvh_nodes_per_ray'), 'tris/ray', g.get('tris_per_ray'), 'lanes node', a.get('node_steps'), 'tri', a.get('triangle_steps'), 'valu/64', r.get('valu_wave_instr_per_64_rays'), 'ext_ms', r.get('extend_ms'), 'sh_ms', r.get('shade_ms'))" < $T/line.txt
  done
done
cp /tmp/keep.so $L
rm -rf $T
exit $rc
