#!/usr/bin/env python3
"""Do two sets of hipcc -S listings hold the same kernels (tools only)?
   python tools/listing_diff.py --old old/*.s --new rsock_amd/build/*.s
Kernels are paired by base name plus template arguments, whatever file or namespace they sit in.  Per
kernel, the instruction stream and the .amdhsa_ resource block are compared as text after taking out what
moving code between units changes: label numbers, and the types mangled into symbols.  Prints the number
of equal kernels and a unified diff of the others; exit status 1 on any difference or unpaired kernel."""
import argparse
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_count import body  # noqa: E402


def kernel_key(sym):
    """k_name<template arguments> of a mangled symbol: the last name of a (nested) name, and its template
    arguments when they are all literals (integers, bools) -- as every kernel of this project's has.
    Anything else keys as the whole symbol."""
    m = re.match(r'_ZN?', sym)
    if not m:
        return sym
    i, name = m.end(), None
    while True:
        d = re.match(r'\d+', sym[i:])
        if not d:
            break
        n = int(d.group())
        name = sym[i + d.end(): i + d.end() + n]
        i += d.end() + n
    if name is None:
        return sym
    if sym[i:i + 1] != 'I':
        return name
    j, depth = i + 1, 1
    while j < len(sym) and depth:
        depth += {'L': 1, 'E': -1}.get(sym[j], 0)
        j += 1
    args = sym[i + 1: j - 1]
    if depth or not re.fullmatch(r'(L[a-z]n?\d+E)+', args):
        return sym
    return name + '<' + ','.join(re.findall(r'L([a-z]n?\d+)E', args)) + '>'


def normalise(line, own):
    line = line.split(';')[0].rstrip()
    line = line.replace(own, '<kernel>')
    line = re.sub(r'\.LBB\d+_', '.LBB_', line)
    line = re.sub(r'\.L(func_[a-z]+|post_getpc)\d+', r'.L\1', line)  # numbered through the whole unit
    return re.sub(r'_Z\w+', lambda m: kernel_key(m.group()), line)


def kernels(paths):
    """{key: (instruction lines, resource lines)} of every kernel in the listings."""
    out = {}
    for p in paths:
        lines = open(p).read().split('\n')
        for sym, b in body(lines, ''):
            if not any(l.strip().startswith('.amdhsa_kernel') for l in b):
                continue  # a device function
            norm = [normalise(l, sym) for l in b]
            cut = next((k for k, l in enumerate(norm) if l.strip().startswith(('.section', '.amdhsa_kernel'))),
                       len(norm))
            ins = [l for l in norm[:cut] if l.strip()]
            res = [l.strip() for l in norm[cut:] if l.strip().startswith('.amdhsa_')]
            key = kernel_key(sym)
            if key in out:
                raise SystemExit('%s: kernel %s appears twice in one set' % (p, key))
            out[key] = (ins, res)
    return out


def compare(old, new, out=sys.stdout):
    """Prints the report; returns the number of kernels that differ or have no partner."""
    bad = equal = 0
    for key in sorted(set(old) | set(new)):
        if key not in old or key not in new:
            out.write('UNPAIRED %s: only in the %s set\n' % (key, 'old' if key in old else 'new'))
            bad += 1
            continue
        parts = [(what, a, b) for what, a, b in zip(('instructions', 'resources'), old[key], new[key]) if a != b]
        if not parts:
            equal += 1
            continue
        bad += 1
        for what, a, b in parts:
            out.write('DIFFERENT %s: %s\n' % (key, what))
            out.writelines(l + '\n' for l in difflib.unified_diff(a, b, 'old', 'new', lineterm='', n=2))
    out.write('%d kernels equal, %d different or unpaired (old %d, new %d)\n'
              % (equal, bad, len(old), len(new)))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--old', nargs='+', required=True)
    ap.add_argument('--new', nargs='+', required=True)
    a = ap.parse_args()
    sys.exit(1 if compare(kernels(a.old), kernels(a.new)) else 0)


if __name__ == '__main__':
    main()
