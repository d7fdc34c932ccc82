#!/usr/bin/env python3
"""compare two llvm-objdump disassemblies kernel by kernel, ignoring addresses / encodings:  tools/isa_diff.py a.s b.s [renames]
renames: a file of `old-substring new-substring` lines for kernels whose names changed; both disassemblies demangled (llvm-objdump --demangle), and the
substrings written without spaces (with a renames file, names are compared with their spaces removed).  The first line whose old-substring occurs in a name
of a.s renames it."""
import re, sys
strip = len(sys.argv) > 3
def load(p):
    ks, cur = {}, None
    for l in open(p):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", l)
        if m:
            cur = m.group(1).replace(" ", "") if strip else m.group(1); ks[cur] = []; continue
        if cur is None or not l.strip():
            continue
        l = re.sub(r"//.*$", "", l).strip()
        l = re.sub(r"<[^>]+>", "", l)          # branch target symbols
        ks[cur].append(l)
    return ks
a, b = load(sys.argv[1]), load(sys.argv[2])
if strip:
    pairs = [l.split() for l in open(sys.argv[3]) if l.strip() and not l.startswith("#")]
    def rename(k):
        for old, new in pairs:
            if old in k:
                return k.replace(old, new)
        return k
    a = {rename(k): v for k, v in a.items()}
same = diff = 0
for k in sorted(set(a) | set(b)):
    if a.get(k) == b.get(k):
        same += 1
    else:
        diff += 1
        print("DIFF", k[:120], len(a.get(k, [])), len(b.get(k, [])))
print(f"{same} kernels identical, {diff} differ")
