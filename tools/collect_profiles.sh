#!/bin/bash
ulimit -c 0  # a GPU memory fault must not leave a core dump that fills the box's disk
# Run on the GPU box (gpurun -- bash tools/collect_profiles.sh <tag>): bench line, rocprofv3 kernel
# stats and the PMC passes the roofline object cites.  Results land in gpurun_out/<tag>_*.
tag=${1:-r06}
root=${GRAFT_REPO_ROOT:-/root/repo}
out=$root/gpurun_out
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
H="$root/bench.py --full --headline-only --steps 6 --warmup 1 --map-cache /tmp/lslam_${tag}_map"
timeout 600 python3 $H > $out/${tag}_headline.json 2> $out/${tag}_headline.err   # builds and saves the map once
timeout 1500 python3 $root/bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
cp $out/bench_report.json $out/${tag}_bench_report.json   # the full report of THIS run (later runs overwrite bench_report.json)
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_stats -o s -- python3 $root/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --pg-iters 20 --map-cache /tmp/lslam_${tag}_map > $out/${tag}_stats.log 2>&1
cp $out/${tag}_stats/s_kernel_stats.csv $out/${tag}_kernel_stats.csv
# ... and of the headline command alone (the one the counter passes wrap): (sweep_kernel + sweep_queue_kernel + cert_plan_kernel
# total) / sweep_kernel calls is the average sweep that roofline.avg_kernel_ms of <tag>_headline.json measures with its HIP events
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_hstats -o s -- python3 $H > $out/${tag}_hstats.log 2>&1
cp $out/${tag}_hstats/s_kernel_stats.csv $out/${tag}_headline_kernel_stats.csv
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" \
  "SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD" \
  "SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_F32 SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE" \
  "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum" \
  "TA_BUSY_avr TA_TA_BUSY_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TA_FLAT_READ_WAVEFRONTS_sum" \
  "SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INST_CYCLES_VMEM_RD"; do
  i=$((i+1))
  timeout 900 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $out/${tag}_pmc/p$i -o p -- python3 $H > $out/${tag}_pmc_p$i.log 2>&1
done
# the headline's sweep is the grid sweep (search AUTO): sweep_grid_kernel + its second pass, mean per sweep
python3 $root/tools/summarize_pmc.py sweep_grid_kernel,sweep_queue_kernel,cert_plan_kernel $out/${tag}_pmc_sweep.csv $out/${tag}_pmc/p1 $out/${tag}_pmc/p2 $out/${tag}_pmc/p3 $out/${tag}_pmc/p4 $out/${tag}_pmc/p5 $out/${tag}_pmc/p6 $out/${tag}_pmc/p7 > /dev/null
python3 $root/tools/summarize_pmc_by_name.py $out/${tag}_pmc_sweep_by_kernel.csv "rocprofv3 --kernel-trace --pmc <set> --output-format csv -- python3 bench.py --full --headline-only --steps 6 --warmup 1 (one pass per counter set): the dispatches of a sweep, per kernel; FETCH_SIZE / WRITE_SIZE in KiB as reported" sweep_grid_kernel,sweep_queue_kernel,cert_plan_kernel,sweep_kernel $out/${tag}_pmc/p1 $out/${tag}_pmc/p2 $out/${tag}_pmc/p3 $out/${tag}_pmc/p4 > /dev/null 2>&1
# the same command through the kd-tree walk (--search lane: round 3's kernel + certificate sweep): kernel stats and the
# instruction / lane counters, for the before / after of the search
HL="$H --search lane"
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_lstats -o s -- python3 $HL > $out/${tag}_lane_headline.json 2> $out/${tag}_lstats.log
cp $out/${tag}_lstats/s_kernel_stats.csv $out/${tag}_lane_headline_kernel_stats.csv
i=0
for set in "SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD" \
  "SQ_ACTIVE_INST_VALU SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_F32 SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"; do
  i=$((i+1))
  timeout 900 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $out/${tag}_lpmc/p$i -o p -- python3 $HL > $out/${tag}_lpmc_p$i.log 2>&1
done
python3 $root/tools/summarize_pmc.py sweep_kernel,sweep_queue_kernel,cert_plan_kernel $out/${tag}_lane_pmc_sweep.csv $out/${tag}_lpmc/p1 $out/${tag}_lpmc/p2 > /dev/null
# (six timed steps: the statistics also hold the warm-up step and the step that counts the second pass's share, whose first
# sweeps run on cold caches -- 10.9 and 10.7 ms against 9.7 -- and with two timed steps those two were half the mean: +3.4 %)
# The kept kernel statistics must reproduce the line they are kept beside (round 4's did not: the profiled command timed one
# more step with a debug tap that cost two atomics per workgroup; the tap now counts in the planner's launch and the sweep
# kernel is the same code with it on).  Fails loudly: a profile that disagrees with the line is not evidence.
rc=0
python3 $root/tools/check_profile_consistency.py $out/${tag}_headline.json $out/${tag}_headline_kernel_stats.csv > $out/${tag}_profile_check.txt 2>&1 || rc=1
python3 $root/tools/check_profile_consistency.py $out/${tag}_lane_headline.json $out/${tag}_lane_headline_kernel_stats.csv >> $out/${tag}_profile_check.txt 2>&1 || rc=1
cat $out/${tag}_profile_check.txt
rm -rf $out/${tag}_lpmc $out/${tag}_lstats
rm -rf $out/${tag}_pmc $out/${tag}_stats $out/${tag}_hstats   # raw traces are gigabytes; the summaries above are what is kept
du -sh $out | tail -1
if [ $rc -ne 0 ]; then echo "collect_profiles: PROFILE INCONSISTENT WITH THE LINE (see ${tag}_profile_check.txt)" >&2; exit 1; fi
