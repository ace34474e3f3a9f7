mkdir -p gpurun_out
export TS_BENCH_WATCHDOG=100
for flags in "--full --no-cpu-baseline --no-face --no-modes --no-roofline" "--full --no-cpu-baseline --no-face --no-roofline" "--full --no-cpu-baseline --no-face --no-modes" "--full --no-cpu-baseline --no-modes --no-roofline" "--full --no-face --no-modes --no-roofline"; do
  echo "=== $flags" >> gpurun_out/bisect.log
  timeout 150 python bench.py --steps 20 --warmup 5 $flags >> gpurun_out/bisect.log 2>> gpurun_out/bisect.err
  echo "rc=$?" >> gpurun_out/bisect.log
done
tail -c 3000 gpurun_out/bisect.err
