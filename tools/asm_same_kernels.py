#!/usr/bin/env python3
"""Are the kernels of two sets of device-assembly files the same instruction for instruction, whichever file and order they come in?
usage: tools/asm_same_kernels.py A.s [A2.s ...] -- B.s [B2.s ...]
A kernel is the text from its label to its .Lfunc_end (the .amdhsa_kernel block with its resources included).  Kernels are matched by
DEMANGLED name with the namespace qualifiers dropped, so a type that moved from one namespace to another (which changes every mangled
name that mentions it) still pairs up.  Comments are dropped, and the labels that carry the function's index in its file (.LBB<n>_,
.Lfunc_end<n>, ...) are renumbered.  Prints one SAME / DIFF line per kernel and a final count of kernels (device functions left out of line,
if any, are compared too and counted apart); the exit status is 0 when all are SAME.
The comparison is of instruction text and nothing else."""
import re, subprocess, sys


def plain_names(mangled):
    try:                                        # (binutils' demangler: the ROCm toolchain ships none)
        out = subprocess.run(['c++filt'], input='\n'.join(mangled), capture_output=True, text=True, check=True).stdout.split('\n')
    except (OSError, subprocess.CalledProcessError) as e:
        sys.exit(f'asm_same_kernels.py: c++filt is needed to pair kernels by demangled name and did not run: {e}')
    if len(out) < len(mangled): sys.exit('asm_same_kernels.py: c++filt returned fewer names than it was given')
    return {m: re.sub(r'(\(anonymous namespace\)|\w+)::', '', d) for m, d in zip(mangled, out)}


def functions(path):
    """{mangled name: [lines]} of every function of one assembly file, and which of them are kernels"""
    funcs, kernels, cur, name = {}, set(), None, None
    for line in open(path):
        m = re.match(r'^\s*\.type\s+([\w.$]+),@function', line)
        if m: name = m.group(1); continue
        if name and cur is None and line.startswith(name + ':'): cur = []; continue
        if cur is None: continue
        if re.match(r'^\.Lfunc_end\d+:', line): funcs[name] = cur; cur = name = None; continue
        if re.match(r'^\s*\.amdhsa_kernel\s', line): kernels.add(name)
        cur.append(line)
    return funcs, kernels


def normal(lines, names):
    out = []
    for line in lines:
        line = re.sub(r'\s*(;|//).*$', '', line.rstrip('\n'))                     # comments, and the padding in front of them
        if not line.strip(): continue
        line = re.sub(r'\.L([A-Za-z_]+?)\d+(_\d+)?\b', lambda m: '.L' + m.group(1) + '#' + (m.group(2) or ''), line)
        line = re.sub(r'\b_Z\w+', lambda m: names.get(m.group(0), m.group(0)), line)  # symbols: by the same plain names as the kernels
        out.append(re.sub(r'\s+', ' ', line.strip()))
    return out


def side(paths):
    funcs, kernels = {}, set()
    for p in paths:
        f, k = functions(p)
        for n in f:
            if n in funcs: print(f'{n}: defined in more than one file of a side ({p})')
        funcs.update(f); kernels |= k
    symbols = sorted({s for body in funcs.values() for line in body for s in re.findall(r'\b_Z\w+', line)} | set(funcs))
    names = plain_names(symbols)
    return {names[n]: normal(body, names) for n, body in funcs.items()}, {names[n] for n in kernels}


def main(argv):
    if '--' not in argv or argv[0] == '--' or argv[-1] == '--':
        print(__doc__, file=sys.stderr)
        return 2
    a, ka = side(argv[:argv.index('--')])
    b, kb = side(argv[argv.index('--') + 1:])
    same = diff = 0
    for name in sorted(ka | kb):                 # kernels only: a device function that was not inlined is part of no kernel's text
        if name not in a or name not in b:
            print(f'DIFF  only in the {"first" if name in a else "second"} set: {name}'); diff += 1
        elif a[name] == b[name]:
            print(f'SAME  {name}  ({len(a[name])} lines)'); same += 1
        else:
            at = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
            print(f'DIFF  {name}  ({len(a[name])} / {len(b[name])} lines; first difference at line {at}: '
                  f'{a[name][at] if at < len(a[name]) else "<end>"!r} / {b[name][at] if at < len(b[name]) else "<end>"!r})'); diff += 1
    # device functions that were left out of line are part of some kernel's code: compared the same way, counted apart
    other = sorted((set(a) | set(b)) - ka - kb)
    other_diff = [n for n in other if a.get(n) != b.get(n)]
    for n in other: print(f'{"DIFF" if n in other_diff else "SAME"}  function (not a kernel) {n}')
    if other: print(f'{len(other) - len(other_diff)} SAME, {len(other_diff)} DIFF of {len(other)} device functions that are not kernels')
    diff += len(other_diff)
    print(f'{same} SAME, {len(ka | kb) - same} DIFF of {len(ka | kb)} kernels ({len(ka)} / {len(kb)} per side)')
    return 0 if diff == 0 else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
