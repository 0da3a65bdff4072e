#!/usr/bin/env python3
"""Per-kernel ISA comparison of two builds of the library:  kernel_isa_diff.py [--rename OLD_SYMBOL=NEW_SYMBOL]... <dirA> <dirB>

Each directory holds the `*-hip-amdgcn-amd-amdhsa-gfx950.s` files of one build: every unit of csrc/ compiled with the flags of
wct_tf_amd/build.py plus --save-temps, from inside the directory.  A kernel is the text from its `_Z...:` label to
`.Lfunc_end` (instructions and kernel descriptor), comments stripped, the `.LBB<n>_` label numbers normalised and the closing
switch back to the text section written as `.text` whether or not the kernel is an instance of a template.  Exit status 0 iff both builds have the same set
of kernel symbols, every symbol is emitted by exactly one unit of its build, and every kernel's instruction text is identical.
Under a kernel that differs: its line counts and the opcodes whose counts differ.
--rename (repeatable): a kernel of build A whose mangled name changed (template arguments dropped, say) is compared under its new
name: OLD_SYMBOL becomes NEW_SYMBOL as build A's symbol and wherever its text names it, before the comparison."""
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
                # the way back to the text section behind the kernel descriptor: `.section .text.<symbol>,...,comdat` for an
                # instance of a template, plain `.text` for a kernel that is none -- where the code lies, not what it is
                s = re.sub(r'^\s*\.section\s+\.text\.\S+,comdat$', '\t.text', s)
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


def renamed(ks, renames):
    """ks with every OLD symbol of renames [(OLD, NEW), ...] called NEW, as a key and wherever a kernel's text names it"""
    for old, new in renames:
        out = {}
        for k, es in ks.items():      # (a NEW that the build has already: both entries under it, reported as MULTIPLE)
            out.setdefault(new if k == old else k, []).extend((unit, [s.replace(old, new) for s in lines]) for unit, lines in es)
        ks = out
    return ks


def main():
    args, renames = [], []
    argv = sys.argv[1:]
    while argv:
        x = argv.pop(0)
        if x == '--rename':
            renames.append(tuple(argv.pop(0).split('=', 1)))
        elif x.startswith('--rename='):
            renames.append(tuple(x[len('--rename='):].split('=', 1)))
        else:
            args.append(x)
    a, b = renamed(kernels(args[0]), renames), kernels(args[1])
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
