#!/bin/bash
set -u
OUT=gpurun_out/r05_fused; mkdir -p $OUT; rm -f $OUT/ab3.txt
q() { python3 -c "
import json,sys; p=json.loads([l for l in sys.stdin if l.startswith('{')][0]); s=p.get('sharded_world1', p)
print('value', p['value'], 'sharded', s['value'], 'ratio', round(s['value']/p['value'],3) if 'sharded_world1' in p else '-', 'launch us', s['roofline']['us_per_launch'])"; }
for i in 1 2; do
for v in gen8 gen12 gen16; do echo -n "fused $v: " | tee -a $OUT/ab3.txt; VOXELHASH_LIB=voxelhashing_demo_amd/lib/alt/v_$v.so python3 bench.py --sharded --legs none 2>/dev/null | q | tee -a $OUT/ab3.txt; done
echo -n "separate: " | tee -a $OUT/ab3.txt; python3 bench.py --sharded --legs none --option fused_generation=0 2>/dev/null | q | tee -a $OUT/ab3.txt
done
echo -n "unsharded + fused groups=4: " | tee -a $OUT/ab3.txt; python3 bench.py --full --legs sharded 2>/dev/null | q | tee -a $OUT/ab3.txt
