#!/usr/bin/env python3
"""Per-kernel ISA comparison of two builds of the library:  kernel_isa_diff.py <dirA> <dirB>

Each directory holds the `*-hip-amdgcn-amd-amdhsa-gfx950.s` files of one build: every unit of csrc/ compiled with the flags of
wct_tf_amd/build.py plus --save-temps, from inside the directory.  A kernel is the text from its `_Z...:` label to
`.Lfunc_end`, comments stripped and the `.LBB<n>_` label numbers normalised.  Exit status 0 iff both builds have the same set
of kernel symbols, every symbol is emitted by exactly one unit of its build, and every kernel's instruction text is identical.
Under a kernel that differs: its line counts and the opcodes whose counts differ."""
import collections
import glob
import os
import re
import sys


def kernels(d):
    """{symbol: [(unit, [instruction lines]), ...]} over the device assembly files of directory d"""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, '*-hip-amdgcn-amd-amdhsa-gfx950.s'))):
        unit = os.path.basename(path).split('-hip-')[0]
        names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', open(path).read(), re.M))
        cur = None
        for line in open(path):
            m = re.match(r'^(_Z\w+):', line)
            if m and m.group(1) in names:
                cur = []
                out.setdefault(m.group(1), []).append((unit, cur))
            elif cur is not None:
                if line.startswith('.Lfunc_end'):
                    cur = None
                    continue
                s = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0].rstrip())
                if s.strip():
                    cur.append(s)
    return out


def opcodes(lines):
    """histogram of the opcodes of a kernel's instruction lines (labels and directives left out); a DPP-modified instruction
    counts under its opcode and once more under 'dpp'"""
    h = collections.Counter()
    for s in lines:
        op = s.split()[0]
        if s[0].isspace() and not op.startswith('.'):
            h[op] += 1
            h['dpp'] += op.endswith('_dpp') or 'row_mask:' in s or 'quad_perm:' in s
    return h


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    print('%-8s %-10s %-10s %6s  kernel' % ('status', 'unit A', 'unit B', 'lines'))
    for k in sorted(set(a) | set(b)):
        ea, eb = a.get(k, []), b.get(k, [])
        if len(ea) > 1 or len(eb) > 1:
            status = 'MULTIPLE'
        elif not ea or not eb:
            status = 'MISSING'
        else:
            status = 'same' if ea[0][1] == eb[0][1] else 'DIFF'
        bad += status != 'same'
        print('%-8s %-10s %-10s %6d  %s' % (status, ','.join(u for u, _ in ea) or '-', ','.join(u for u, _ in eb) or '-',
                                            len(eb[0][1]) if eb else 0, k))
        if status == 'DIFF':
            ha, hb = opcodes(ea[0][1]), opcodes(eb[0][1])
            print('         %d -> %d lines; opcode counts that differ (A -> B): %s' % (
                len(ea[0][1]), len(eb[0][1]), ', '.join('%s %d -> %d' % (o, ha[o], hb[o]) for o in sorted(ha + hb) if ha[o] != hb[o]) or 'none'))
    print('%d kernels in A, %d in B, %d not identical' % (len(a), len(b), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
