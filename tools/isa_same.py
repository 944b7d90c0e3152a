"""Do two sets of device assembly files hold the same functions, instruction for instruction?
    tools/isa_same.py a.s b1.s b2.s ...          a.s against the others together
    tools/isa_same.py a1.s a2.s -- b1.s b2.s     one set against the other
(device assembly: hipcc <the Makefile's flags> --offload-device-only -S file.hip -o file.s)
A function is the lines between its label and its .Lfunc_end, without `;` comments and blank lines, the function's ordinal
in local labels (.LBB<n>_, .LJTI<n>_, .LCPI<n>_) replaced by a fixed token: what is left is instructions, labels and
directives.  A kernel's descriptor is its .amdhsa_* lines (registers, LDS, scratch).  Compared: the sets of function
symbols, every function's lines, every kernel's descriptor.  A function that one set holds in several files (an inline
function that was not inlined) must be the same in all of them.  Exit status 1 if anything differs."""
import re
import sys

ORDINAL = re.compile(r'\.L(BB|JTI|CPI)\d+_')


def clean(line):
    line = line.split(';')[0].strip()
    return ORDINAL.sub(r'.L\1#_', line)


def read_set(paths):
    """({function: lines}, {kernel: descriptor lines}, [complaints]) of the files together"""
    funcs, descs, bad = {}, {}, []

    def put(table, what, sym, body, path):
        if sym in table and table[sym] != body:
            bad.append('%s %s differs between files of one set (%s)' % (what, sym, path))
        table[sym] = body

    for path in paths:
        is_func, cur, body, kd = set(), None, [], None
        for raw in open(path):
            m = re.match(r'\s*\.type\s+([^,\s]+),@function', raw)
            if m:
                is_func.add(m.group(1))
                continue
            line = clean(raw)
            if not line:
                continue
            if kd is not None:                     # (a descriptor stands between its kernel's last instruction and .Lfunc_end)
                if line == '.end_amdhsa_kernel':
                    put(descs, 'descriptor', kd, desc, path)
                    kd = None
                else:
                    desc.append(line)
                continue
            m = re.match(r'\.amdhsa_kernel\s+(\S+)', line)
            if m:
                kd, desc = m.group(1), []
            elif cur is None:
                m = re.match(r'([^\s:]+):$', line)
                if m and m.group(1) in is_func:
                    cur, body = m.group(1), []
            elif line.startswith('.Lfunc_end'):
                put(funcs, 'function', cur, body, path)
                cur = None
            else:
                body.append(line)
        if cur is not None or kd is not None:
            bad.append('%s ends inside %s' % (path, cur or kd))
    return funcs, descs, bad


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return 'line %d: %r / %r' % (i + 1, x, y)
    return '%d / %d lines' % (len(a), len(b))


def main(argv):
    if '--' in argv:
        left, right = argv[:argv.index('--')], argv[argv.index('--') + 1:]
    else:
        left, right = argv[:1], argv[1:]
    if not left or not right:
        sys.exit(__doc__)
    fa, da, bad = read_set(left)
    fb, db, bad_b = read_set(right)
    bad += bad_b
    for what, a, b in (('function', fa, fb), ('descriptor', da, db)):
        for sym in sorted(set(a) - set(b)):
            bad.append('%s %s: in the first set only' % (what, sym))
        for sym in sorted(set(b) - set(a)):
            bad.append('%s %s: in the second set only' % (what, sym))
        for sym in sorted(set(a) & set(b)):
            if a[sym] != b[sym]:
                bad.append('%s %s differs, %s' % (what, sym, first_difference(a[sym], b[sym])))
    print('functions: %d / %d, %d instruction and label lines / %d; kernels: %d / %d' %
          (len(fa), len(fb), sum(map(len, fa.values())), sum(map(len, fb.values())), len(da), len(db)))
    for b in bad:
        print('DIFFERENT:', b)
    print('same' if not bad else '%d differences' % len(bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
