#!/usr/bin/env python3
"""tools/kernel_isa_diff.py OLD.s NEW.s - compares two device-only assemblies (as tools/kernel_resources.sh writes them) kernel by kernel.

Per kernel: comments and directives are dropped and the local labels renamed in their order of appearance; then
  SAME       the instruction streams are equal,
  REORDERED  they differ, with equal opcode multisets (so equal instruction counts),
  DIFF       anything else (also a kernel that one side lacks),
each with both instruction counts.  Exit status 1 if any kernel is DIFF.  It only compares."""
import collections
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for name in re.findall(r"^\s+\.amdhsa_kernel (\S+)", txt, re.M):
        body = txt[txt.index("\n" + name + ":"):txt.index(".amdhsa_kernel " + name)]
        labels, ins = {}, []
        for line in body.split("\n")[2:]:
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.endswith(":")):
                continue                                  # comment or directive; a label (".LBB3_7:") stays, as a position in the stream
            line = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), line)
            ins.append(re.sub(r"\s+", " ", line))
        out[name] = ins
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    worst = 0
    for name in list(old) + [n for n in new if n not in old]:
        a, b = old.get(name), new.get(name)
        ops = lambda ins: collections.Counter(i.split(" ")[0] for i in ins if not i.endswith(":"))
        n = lambda ins: "-" if ins is None else str(sum(ops(ins).values()))
        if a is not None and a == b:
            verdict = "SAME"
        elif a is not None and b is not None and ops(a) == ops(b):
            verdict = "REORDERED"
        else:
            verdict, worst = "DIFF", 1
        print(f"{verdict:9s} {n(a):>6s} {n(b):>6s}  {name}")
    return worst


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
