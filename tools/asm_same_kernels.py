"""Are two device-assembly files the same kernels, whatever their order?  Splits at function sections and kernel-metadata entries,
renumbers the labels that carry the function's index (.LBB<n>_, BB<n>_ in comments, .Lfunc_end<n>, ...) and compares multisets."""
import re, sys, collections
def chunks(path):
    out, cur = [], []
    for line in open(path):
        if re.match(r'^\t\.section\t\.text\.|^  - \.|^\t\.amdgpu_metadata|^\.\.\.', line):
            out.append(''.join(cur)); cur = []
        cur.append(line)
    out.append(''.join(cur))
    return out
def norm(c):
    c = re.sub(r'\.L([A-Za-z_]+?)\d+(_\d+)?\b', lambda m: '.L' + m.group(1) + '#' + (m.group(2) or ''), c)
    return re.sub(r'\bBB\d+_(\d+)\b', r'BB#_\1', c)
a, b = [norm(c) for c in chunks(sys.argv[1])], [norm(c) for c in chunks(sys.argv[2])]
same_seq = a == b
same_set = collections.Counter(a) == collections.Counter(b)
moved = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
print(f'chunks {len(a)} / {len(b)}; identical in order: {same_seq}; identical as multisets: {same_set}; positions holding another chunk: {len(moved)}')
for i in moved:
    print(' ', i, a[i].split('\n')[0].strip()[:150])
