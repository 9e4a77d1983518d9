#!/bin/bash
# Is the device code of two trees the same?     scripts/isa_compare.sh TREE_A TREE_B FILE.hip [FILE.hip ...]
# Every named file of diverseseq_amd/csrc is compiled to gfx950 assembly (device side only) in both trees, each with the
# flags its own tree's Makefile gives that file (EXTRA= from the environment included); a file one tree does not have is
# skipped there.  One line per kernel and device function: same, differs (and in what), or only in A / only in B -- a
# function counts as present wherever among the named files it is found, so it may change translation unit.  Compared
# are the instruction text, the .amdhsa_ block and resource symbols, and the metadata entry (registers, spills, scratch,
# LDS, kernarg); comments, .file/.loc/.ident and the function ordinal inside local labels are left out.  No GPU needed.
# Exit status 0 only if everything is the same.  The assembly is kept (and its directory named) when it is not.
set -euo pipefail
[ $# -ge 3 ] || { echo "usage: $0 TREE_A TREE_B FILE.hip [FILE.hip ...]" >&2; exit 2; }
A=$(realpath "$1"); B=$(realpath "$2"); shift 2
out=$(mktemp -d)
for side in A B; do
    csrc=${!side}/diverseseq_amd/csrc
    mkdir -p "$out/$side"
    for f in "$@"; do
        [ -f "$csrc/$f" ] || continue
        cmd=$(make -C "$csrc" --no-print-directory -n -B "build/$f.o" | grep -- " -c $f ")
        cmd=${cmd/ -c $f -o build\/$f.o/ --cuda-device-only -S $f -o $out/$side/$f.s}
        (cd "$csrc" && eval "$cmd" 2> "$out/$side/$f.log" || echo "$side: $f does not compile, see $out/$side/$f.log" >&2) &
    done
done
wait
python3 - "$out" <<'EOF' && rm -rf "$out" || { echo "assembly kept in $out" >&2; exit 1; }
import glob, re, shutil, subprocess, sys

def functions(side):
    """symbol -> {'instructions': ..., 'resources': ..., 'metadata': ...} over every .s file of one side"""
    found = {}
    for path in sorted(glob.glob(f'{sys.argv[1]}/{side}/*.s')):
        lines = []
        for ln in open(path):
            ln = re.sub(r'\s*;.*', '', ln.rstrip())
            if ln.strip() and not re.match(r'\s*\.(file|loc|ident)\b', ln):
                lines.append(re.sub(r'(\.L[A-Za-z_]+?)\d+(_\d+)?\b', r'\1\2', ln))
        sym, body = None, None
        for i, ln in enumerate(lines):
            m = re.match(r'\s*\.type\s+(\S+),@function', ln)
            if m:
                sym, body = m.group(1), []
            elif sym and re.match(r'\s*\.size\s+' + re.escape(sym) + ',', ln):
                hsa = [b for b in body if re.match(r'\s*\.(end_)?amdhsa_', b)]
                sets = [l for l in lines[i + 1:i + 40] if l.strip().startswith('.set ' + sym + '.')]
                found[sym] = {'instructions': [b for b in body if b not in hsa], 'resources': hsa + sets, 'metadata': None}
                sym = None
            elif sym:
                body.append(ln)
        text = '\n'.join(lines)
        meta = text[text.find('amdhsa.kernels:'):text.find('amdhsa.target:')] if 'amdhsa.kernels:' in text else ''
        for entry in re.split(r'\n  - ', meta)[1:]:
            found[re.search(r'\.name:\s+(\S+)', entry).group(1)]['metadata'] = entry.strip()
    return found

a, b = functions('A'), functions('B')
names = sorted(set(a) | set(b))
pretty = dict(zip(names, names))
if names and shutil.which('c++filt'):
    pretty = dict(zip(names, subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.splitlines()))
bad = 0 if names else 1
for n in names:
    if n not in a or n not in b:
        verdict = 'only in B' if n not in a else 'only in A'
    else:
        diff = [k for k in ('instructions', 'resources', 'metadata') if a[n][k] != b[n][k]]
        verdict = 'differs (' + ', '.join(diff) + ')' if diff else 'same'
    bad += verdict != 'same'
    print(f'{verdict:12s} {pretty[n]}')
print(f'{len(names)} functions, {bad} not the same' if names else 'no function found')
sys.exit(1 if bad else 0)
EOF
