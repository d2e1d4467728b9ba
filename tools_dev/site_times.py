"""Per-site times of the LAST frame of a single-stream kernel trace of tools_dev/site_prof.py (rocprofv3 --kernel-trace CSV): the encoder convs and the p5/p4/p3 laterals
in launch order (a k_conv_splitk_epilogue belongs to the launch before it)."""
import csv, sys
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r['Start_Timestamp']))
idx = [i for i, r in enumerate(rows) if 'nchw3_to_nhwc4' in r['Kernel_Name']]
rows = rows[idx[-1]:]
sites = []
for L, n in enumerate([3, 4, 6, 3]):
    for b in range(n):
        sites.append(f"layer{L+1}.{b} conv1")
        if b == 0 and L > 0: sites.append(f"layer{L+1}.0 downsample")
        sites.append(f"layer{L+1}.{b} conv2")
sites += ["p5 lateral", "p4 lateral", "p3 lateral"]
i = 3      # nchw3_to_nhwc4, stem, maxpool
out = []
for s in sites:
    r = rows[i]; d = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3; nm = r['Kernel_Name'].replace('void ', '').replace('fpc::', '').split('(fpc')[0]
    i += 1
    if i < len(rows) and 'splitk_epilogue' in rows[i]['Kernel_Name']:
        d += (int(rows[i]['End_Timestamp']) - int(rows[i]['Start_Timestamp'])) / 1e3; nm += " + splitk_epilogue"; i += 1
    out.append((s, nm, d))
nine = 0.0
for s, nm, d in out:
    key = ('.0 conv1' in s and not s.startswith('layer1')) or 'downsample' in s or 'lateral' in s
    if key: nine += d
    print(f"{'*' if key else ' '} {s:22s} {d:8.1f} us  {nm}")
print(f"nine direct sites (*) together: {nine:.1f} us")
