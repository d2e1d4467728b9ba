"""Kernel time per streamed frame from a rocprofv3 --kernel-trace CSV of a plain bench.py run: the window between the first and the
last of the trace's last N + 1 k_nchw3_to_nhwc4 dispatches (one per frame, all streams) holds N frames' kernels in steady state.
Prints per kernel (and per grid for k_conv_wino_h3) calls and microseconds per frame.
    python tools_dev/frame_window_stats.py <kernel_trace.csv> [N = 200]
    python tools_dev/frame_window_stats.py <kernel_trace.csv> --frame      every dispatch of ONE streamed frame: those on the queue of
                                                                           the fifth-last frame start, up to that queue's next one"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
marks = [i for i, r in enumerate(rows) if "nchw3_to_nhwc4" in r["Kernel_Name"]]
if "--frame" in sys.argv:
    s = marks[-5]
    key = "Stream_Id" if "Stream_Id" in rows[s] else "Queue_Id"
    q = rows[s][key]
    mine = [r for r in rows[s:] if r[key] == q]
    end = next(i for i, r in enumerate(mine[1:], 1) if "nchw3_to_nhwc4" in r["Kernel_Name"])
    t0, tot = int(mine[0]["Start_Timestamp"]), 0.0
    for r in mine[:end]:
        d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        tot += d
        print("%9.1f %8.2f grid=(%d,%s,%s) %s" % ((int(r["Start_Timestamp"]) - t0) / 1e3, d, int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]),
                                                 r["Grid_Size_Y"], r["Grid_Size_Z"], r["Kernel_Name"][:80]))
    print("sum of kernels %.1f us, span %.1f us, %d dispatches on stream / queue %s" % (tot, (int(mine[end]["Start_Timestamp"]) - t0) / 1e3, end, q))
    sys.exit(0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
assert len(marks) > N, "fewer frames in the trace than asked for"
s, e = marks[-N - 1], marks[-1]
span = (int(rows[e]["Start_Timestamp"]) - int(rows[s]["Start_Timestamp"])) / 1e3
tot = collections.OrderedDict()
for r in rows[s:e]:
    nm = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("fpc::", "")
    if "k_conv_wino_h3" in nm:
        nm += " grid=%d" % (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
    d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    c = tot.setdefault(nm[:80], [0, 0.0])
    c[0] += 1; c[1] += d
allk = sum(v[1] for v in tot.values())
wino = sum(v[1] for k, v in tot.items() if "k_conv_wino_h3" in k)
print("%d frames, span %.1f us per frame, kernels %.1f us per frame, k_conv_wino_h3 %.1f us per frame (%.1f %%)"
      % (N, span / N, allk / N, wino / N, 100.0 * wino / allk))
for k, v in sorted(tot.items(), key=lambda kv: -kv[1][1]):
    print("%10.1f us/frame  %7.2f calls/frame  %9.1f us mean  %s" % (v[1] / N, v[0] / N, v[1] / v[0], k))
