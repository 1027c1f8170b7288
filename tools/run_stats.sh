# rocprofv3 kernel-trace stats of the HEADLINE workload only (the summary committed under profiles/): no other_configs,
# no end-to-end leg, no CPU baseline, so conv_halo_kernel<0> shows 44 launches per UNet forward at ~100 us -- the unit the
# bench line's roofline is quoted on (the program itself follows `--`: no env / shell hop under the profiler)
# usage: tools/run_stats.sh OUT_DIR      (writes OUT_DIR/stats/ and OUT_DIR/stats_bench.log)
[ $# -eq 1 ] || { echo "usage: tools/run_stats.sh OUT_DIR"; exit 1; }
R=$(cd "$(dirname "$0")/.." && pwd) && mkdir -p "$1" && O=$(cd "$1" && pwd) || exit 1
cd /tmp; export TMPDIR=/tmp
rm -rf $O/stats
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -- python $R/bench.py --full --steps 1 --warmup 1 --no-cpu-baseline --no-e2e --no-other-configs > $O/stats_bench.log 2>&1 || { grep -v "^    @" $O/stats_bench.log | tail -5; exit 1; }
tail -1 $O/stats_bench.log | cut -c1-300
