"""Per-kernel instruction statistics of a hipcc -S --cuda-device-only listing.
    python tools_dev/isa_stats.py /tmp/nk.s [name-substring]
Prints MFMA / other vector / scratch / LDS-DMA counts and the register & LDS footprint.

    python tools_dev/isa_stats.py --compare parent.s[,more.s] result.s[,more.s] [name-substring]
Compares every kernel the two sides share (by mangled name; a side may be several listings): `same` = the instruction sequences
are identical once labels and comments are stripped and the .amdhsa footprint (next_free_vgpr, accum_offset, group / private segment
size) is equal.  For a kernel that differs: the footprint of both sides, whether any column grew, and the K loop(s) — the text from
a loop header's label to its last backward branch — compared as sequences of opcodes (and, where they differ, once more without the
wait instructions, whose number and counts follow from what the compiler knows to be in flight), with the scratch instructions
inside counted."""
import re, sys

KERNEL = re.compile(r'^(_Z\w+):[^\n]*\n(.*?)\n\s*\.amdhsa_kernel (.*?)\.end_amdhsa_kernel', re.S | re.M)      # code up to the descriptor (every s_endpgm)
FOOT = ('next_free_vgpr', 'accum_offset', 'group_segment_fixed_size', 'private_segment_fixed_size')


def kernels(paths):
    out = {}
    for p in paths.split(','):
        for m in KERNEL.finditer(open(p).read()):
            out[m.group(1)] = (m.group(2), m.group(3))
    return out


def instructions(body):
    """(label or None, instruction text) per line, comments and directives dropped, label names kept only as positions."""
    out = []
    for l in body.split('\n'):
        l = l.split(';')[0].strip()
        if not l or l.startswith('.') and not l.endswith(':'):
            continue
        if l.endswith(':'):
            out.append((l[:-1], None))
        else:
            out.append((None, l))
    return out


def stripped(ins):
    """instruction texts with branch targets replaced by their distance in instructions (label names differ between builds)"""
    pos, n = {}, 0
    for lab, txt in ins:
        if lab is not None:
            pos[lab] = n
        else:
            n += 1
    out, n = [], 0
    for lab, txt in ins:
        if txt is None:
            continue
        out.append(re.sub(r'\.?LBB\w+', lambda m: 'L%+d' % (pos.get(m.group(0), 0) - n), txt))
        n += 1
    return out


def loops(ins):
    """[(opcodes, scratch instructions)] of every K loop: a loop header's label ... the last conditional backward branch to it, with
    matrix instructions inside and no other such loop inside it (branch islands behind the code and outer loops are not K loops)"""
    pos, seq = {}, []
    for lab, txt in ins:
        if lab is not None:
            pos[lab] = len(seq)
        else:
            seq.append(txt)
    back = {}
    for i, txt in enumerate(seq):
        m = re.match(r's_cbranch\w*\s+(\.?LBB\w+)', txt)
        if m and m.group(1) in pos and pos[m.group(1)] <= i:
            back[pos[m.group(1)]] = i      # the last one wins
    cand = [(a, b) for a, b in sorted(back.items()) if any(t.startswith('v_mfma') for t in seq[a:b + 1])]
    out = []
    for a, b in cand:
        if not any((c, d) != (a, b) and a <= c and d <= b for c, d in cand):
            ops = [t.split()[0] for t in seq[a:b + 1]]
            out.append((ops, sum(o.startswith('scratch_') for o in ops)))
    return out


def foot(meta):
    return tuple(int((re.search(k + r'\s+(\d+)', meta) or [0, '-1'])[1]) for k in FOOT)


def compare(pa, pb, flt):
    A, B = kernels(pa), kernels(pb)
    bad = 0
    for name in sorted(set(A) & set(B)):
        if flt not in name:
            continue
        ia, ib = instructions(A[name][0]), instructions(B[name][0])
        fa, fb = foot(A[name][1]), foot(B[name][1])
        if stripped(ia) == stripped(ib) and fa == fb:
            print(f"{name}: same ({len(stripped(ia))} instructions; vgpr {fa[0]} agpr-offset {fa[1]} lds {fa[2]} priv {fa[3]})")
            continue
        bad += 1
        la, lb = loops(ia), loops(ib)
        big = [len(o) for o, _ in la], [len(o) for o, _ in lb]
        same = [o for o, _ in la] == [o for o, _ in lb]
        nowait = lambda ls: [[x for x in o if x != 's_waitcnt'] for o, _ in ls]
        waits = lambda ls: sum(o.count('s_waitcnt') for o, _ in ls)
        verdict = ('same opcode sequence' if same else
                   f'same opcode sequence but for its waits (s_waitcnt {waits(la)} -> {waits(lb)})' if nowait(la) == nowait(lb) else 'DIFFERENT')
        sc = lambda s: sum(l.strip().startswith('scratch_') for l in s.split('\n'))
        print(f"{name}: DIFFERS  instructions {len(stripped(ia))} -> {len(stripped(ib))}  footprint {fa} -> {fb} "
              f"{'GREW' if any(y > x for x, y in zip(fa, fb)) else 'no column larger'}  scratch instr. {sc(A[name][0])} -> {sc(B[name][0])}  "
              f"K loops {big[0]} -> {big[1]} ops: {verdict}, "
              f"scratch inside {sum(s for o, s in la)} -> {sum(s for o, s in lb)}")
    for name in sorted(set(A) ^ set(B)):
        if flt in name:
            print(f"{name}: only in {'the first' if name in A else 'the second'} side")
    return bad


def stats(path, flt):
    for name, (body, meta) in kernels(path).items():
        if flt not in name:
            continue
        lines = [l.strip() for l in body.split('\n')]
        nm = sum(l.startswith('v_mfma') for l in lines)
        nv = sum(l.startswith('v_') and not l.startswith('v_mfma') for l in lines)
        sc = sum(l.startswith('scratch_') for l in lines)
        dma = sum(l.startswith('global_load_lds') for l in lines)
        g = lambda k: (re.search(k + r'\s+(\d+)', meta) or [0, '?'])[1]
        print(f"{name}: mfma {nm} valu {nv} scratch {sc} lds-dma {dma} vgpr {g('next_free_vgpr')} agpr {g('accum_offset')} "
              f"lds {g('group_segment_fixed_size')} priv {g('private_segment_fixed_size')}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "")
    else:
        stats(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
