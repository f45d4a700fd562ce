#!/usr/bin/env python
"""Static instruction counts of a tile-loop kernel's front end, from `hipcc -S` output (no GPU needed): everything between
the header of the loop over point tiles and the first MFMA, and where the global loads of the loop body sit relative to
the counted `s_waitcnt vmcnt` of the tiles.

    hipcc <the flags of nerfactor_amd/build.py for the file> --cuda-device-only -S nerf_mlp_v6.hip -o v6.s
    python scripts/front_end_counts.py v6.s [substring of the mangled kernel name]

The loop header is the last label marked "Loop Header" in front of the first v_mfma of the function.  Counts are static:
the 64-bit division's slow path (a block the 32-bit case skips) is listed apart."""
import re
import sys


def function(lines, sub):
    start = next(i for i, l in enumerate(lines) if re.match(r'^_Z\S*:', l) and sub in l.split(':')[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith('.Lfunc_end'))
    return lines[start:end]


def kind(op):
    if op.startswith('v_mfma'):
        return 'mfma'
    if op.startswith('v_accvgpr'):
        return 'valu (v_accvgpr moves)'
    if op.startswith('v_'):
        return 'valu'
    if op == 's_waitcnt':
        return 's_waitcnt'
    if op in ('s_nop', 's_barrier') or op.startswith(('s_cbranch', 's_branch')):
        return op if op in ('s_nop', 's_barrier') else 'branch'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith('global_load_lds'):
        return 'lds-dma piece'
    if op.startswith('global_load'):
        return 'global load'
    if op.startswith('global_store'):
        return 'global store'
    if op == 'ds_bpermute_b32':
        return 'ds_bpermute'
    if op.startswith('ds_'):
        return 'ds other'
    return 'other'


def main():
    path = sys.argv[1]
    sub = sys.argv[2] if len(sys.argv) > 2 else 'fold23nerf_mlp_bf16_v6_kernelILi0ELi1E'
    fn = function(open(path).read().split('\n'), sub)
    ins = []     # (line index, opcode, text, block label)
    label = None
    headers = []
    for i, l in enumerate(fn):
        m = re.match(r'^(\.LBB\d+_\d+):', l)
        if m:
            label = m.group(1)
            if 'Loop Header' in l:
                headers.append((i, label))
            continue
        m = re.match(r'^\s+([a-z_0-9]+)\b', l)
        if m and not l.lstrip().startswith(('.', ';')):
            ins.append((i, m.group(1), l.strip(), label))
    first_mfma = next(i for i, op, _, _ in ins if op.startswith('v_mfma'))
    head_line, head = [h for h in headers if h[0] < first_mfma][-1]
    print('%s\nloop header %s, first MFMA %d lines on' % (fn[0].split(':')[0], head, first_mfma - head_line))
    front = [x for x in ins if head_line < x[0] < first_mfma]
    blocks = []
    for x in front:
        if not blocks or blocks[-1][0] != x[3]:
            blocks.append((x[3], []))
        blocks[-1][1].append(x)
    total = {}
    for lab, xs in blocks:
        c = {}
        for _, op, _, _ in xs:
            c[kind(op)] = c.get(kind(op), 0) + 1
            total[kind(op)] = total.get(kind(op), 0) + 1
        print('  block %-10s %s' % (lab, ', '.join('%s %d' % kv for kv in sorted(c.items()))))
    print('  front end, all blocks: %s' % ', '.join('%s %d' % kv for kv in sorted(total.items())))
    print('  its loads and vmcnt waits, in order: %s' % '; '.join(t.split(';')[0].strip() for _, op, t, _ in front
                                                                  if kind(op) == 'global load' or (op == 's_waitcnt' and 'vmcnt' in t)))
    # the loop body behind the first MFMA: plain global loads between the tiles' counted waits
    body = [x for x in ins if x[0] >= first_mfma]
    waits = 0
    mfma_since = 0
    pending = None
    for _, op, t, _ in body:
        if op.startswith('v_mfma'):
            mfma_since += 1
        if op == 's_waitcnt' and 'vmcnt' in t:
            if pending is not None:
                print('  ... the next vmcnt wait after them: "%s", %d MFMAs later' % (t.split(';')[0].strip(), mfma_since - pending))
                pending = None
            waits += 1
        if kind(op) == 'global load':
            if pending is None:
                print('  loop body: plain global load(s) behind vmcnt wait number %d of the pass, %d MFMAs into the pass:' % (waits, mfma_since))
                pending = mfma_since
            print('      %s' % t.split(';')[0].strip())
        if op.startswith(('s_cbranch', 's_branch')) and pending is None and waits > 60:
            break


if __name__ == '__main__':
    main()
