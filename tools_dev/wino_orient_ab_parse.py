"""Per-shape medians of the plain and the -11 launches from the kernel trace of tools_dev/wino_orient_ab.py.
    python tools_dev/wino_orient_ab_parse.py <kernel_trace.csv> HEADING
"""
import csv, sys, statistics
SHAPES = ["layer1 32x64x120x160->64", "s2.0-unfolded 32x256x120x160->128", "layer2 32x128x60x80->128", "s3.0 32x256x60x80->128"]
WARM, N = 3, 20
rows = [r for r in csv.DictReader(open(sys.argv[1])) if "k_conv_wino_h3" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
per = 2 * (WARM + N)
assert len(rows) == per * len(SHAPES), len(rows)
print(sys.argv[2])
for si, name in enumerate(SHAPES):
    blk = rows[si * per:(si + 1) * per]
    res = []
    for v in (0, 1):
        rs = blk[2 * WARM + v::2]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs]
        grid = int(rs[0]["Grid_Size_X"]) // int(rs[0]["Workgroup_Size_X"])
        tmpl = rs[0]["Kernel_Name"].split("k_conv_wino_h3")[1].split("(")[0]
        res.append((tmpl, grid, statistics.median(us), min(us), max(us)))
    (t0, g0, m0, lo0, hi0), (t1, g1, m1, lo1, hi1) = res
    print("%-36s plain%s grid %5d  %8.1f us (%.1f-%.1f) | -11%s grid %5d  %8.1f us (%.1f-%.1f) | %+.2f %% time, %+.2f %% workgroups"
          % (name, t0, g0, m0, lo0, hi0, t1, g1, m1, lo1, hi1, 100 * (m1 / m0 - 1), 100 * (g1 / g0 - 1)))
