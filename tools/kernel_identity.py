#!/usr/bin/env python3
"""Kernel-by-kernel identity of two device-assembly files of one unit.

    python tools/kernel_identity.py PARENT.s PR.s

For a unit that tools/asm_identity.py reports as DIFFERENT because kernels
were added to it: every kernel's text from its label to its .Lfunc_end, with
the numbering of the local labels (.LBB<n>_, .Lfunc_end<n>, .Lpost_getpc<n>,
.Ltmp<n>) taken out (it shifts when a kernel is inserted before), hashed and
compared by name.
The resource lines of the kernel's .amdhsa descriptor and metadata are part of
asm_identity's whole-file hash; here the instruction stream and the comments
the compiler prints after it (register counts, scratch, occupancy) are.
"""
import hashlib
import re
import sys


def kernels(path):
    out, name, buf, tail = {}, None, [], 0
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, buf, tail = m.group(1), [], 0
            continue
        if name is None:
            continue
        ln = re.sub(r"BB\d+_", "BB_", ln)
        ln = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", ln)
        ln = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln)
        ln = re.sub(r"\.Ltmp\d+", ".Ltmp", ln)
        buf.append(ln)
        # the resource comments follow .Lfunc_end up to the next section
        if ln.startswith(".Lfunc_end"):
            tail = 1
        elif tail and (ln.startswith("\t.section") or ln.startswith("\t.text")):
            n = sum(1 for x in buf if x.startswith("\t") and not x.startswith("\t.")
                    and not x.startswith("\t;"))
            out[name] = (hashlib.sha256("".join(buf).encode()).hexdigest()[:16], n)
            name = None
    return out


def main(a, b):
    ka, kb = kernels(a), kernels(b)
    same = True
    for k in sorted(set(ka) | set(kb)):
        x, y = ka.get(k), kb.get(k)
        if x is None or y is None:
            verdict = "only in " + ("pr" if x is None else "parent")
        else:
            verdict = "IDENTICAL" if x == y else "DIFFERENT"
            same &= x == y
        print(f"{k}\n  parent {x}\n  pr     {y}\n  {verdict}")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
