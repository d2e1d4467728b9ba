#!/bin/bash
# Round-3 profiles of the bench itself, from the library in this tree:
#   gpurun_out/r03_stream_kernel_stats.csv   rocprofv3 --kernel-trace --stats of the DEFAULT bench command
#   gpurun_out/r03_frame_timeline_b1.txt     per-dispatch timeline of one batch-1 frame (latency mode: --no-pipeline)
#   $D/bench.json                            the --full bench line, unprofiled
export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
D=$R/gpurun_out/prof_bench; rm -rf $D; mkdir -p $D
cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $D/stream -- python3 $R/bench.py --full > $D/stream.json 2> $D/stream.err
cd /tmp && timeout 300 rocprofv3 --kernel-trace --output-format csv -d $D/frame -- python3 $R/bench.py --full --steps 40 --warmup 10 --no-pipeline --no-train-line --no-config3 --no-hn128 --no-cpu-baseline --no-plain-f32 > $D/frame.json 2> $D/frame.err
cd $R
python tools_dev/kstats.py $(ls $D/stream/*/*kernel_stats.csv | tail -1) --top 60 --out gpurun_out/r03_stream_kernel_stats.csv | head -24
python tools_dev/frame_timeline.py $(ls $D/frame/*/*kernel_trace.csv | tail -1) --all > gpurun_out/r03_frame_timeline_b1.txt; tail -16 gpurun_out/r03_frame_timeline_b1.txt
timeout 900 python bench.py --full > $D/bench.json 2> $D/bench.err; python tools_dev/bench_summary.py $D/bench.json
