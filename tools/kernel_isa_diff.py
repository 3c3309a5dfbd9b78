#!/usr/bin/env python3
"""Compare device assembly kernel by kernel across two sets of files.

    tools/kernel_isa_diff.py OLD.s... -- NEW.s...

The inputs are `hipcc --cuda-device-only -S` outputs (the Makefile's HIPFLAGS). Each side is cut
into one block per kernel or device-function symbol: its instructions and, for a kernel, its
.amdhsa_ resource directives. Only what the compiler numbers per file is normalised: local labels
(.LBB3_7, .Lfunc_end3, ...) are renumbered in order of appearance within the block, and comments
and line-number directives are dropped. Everything else is compared as text. Prints the symbols
removed, added and changed, then one summary line; exits 1 if the sides differ (like diff).
A refactor that only moves kernels between translation units must report "0 changed".
"""
import difflib
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")
DEBUG = re.compile(r"^\.(loc|file|cfi_\w+)\b")


def blocks(paths):
    """symbol -> normalised lines, from its label to its .Lfunc_end label"""
    out = {}
    for path in paths:
        sym, lines, names = None, [], {}
        for raw in open(path):
            line = raw.split(";", 1)[0].strip()
            if not line or DEBUG.match(line):
                continue
            m = LABEL.match(line)
            if sym is None:
                if m and raw.rstrip().endswith("; @" + m.group(1)):
                    sym, lines, names = m.group(1), [], {}
                continue
            lines.append(LOCAL.sub(lambda t: names.setdefault(t.group(0), ".L%d" % len(names)), line))
            if line.startswith(".Lfunc_end"):
                if sym in out and out[sym] != lines:
                    sys.exit("%s: %s differs from an earlier definition on the same side" % (path, sym))
                out[sym], sym = lines, None
    return out


def demangled(syms):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not syms:
        return dict(zip(syms, syms))
    res = subprocess.run([tool], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(syms, res))


def main(argv):
    if "--" not in argv:
        sys.exit(__doc__)
    cut = argv.index("--")
    old, new = blocks(argv[:cut]), blocks(argv[cut + 1:])
    removed = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    changed = sorted(s for s in set(old) & set(new) if old[s] != new[s])
    names = demangled(removed + added + changed)
    for title, syms in (("removed", removed), ("added", added), ("changed", changed)):
        for s in syms:
            print("%s: %s" % (title, names[s]))
            if title == "changed":
                for d in list(difflib.unified_diff(old[s], new[s], "old", "new", n=1, lineterm=""))[:40]:
                    print("    " + d)
    print("kernel_isa_diff: %d symbols old, %d new: %d changed, %d added, %d removed"
          % (len(old), len(new), len(changed), len(added), len(removed)))
    return 1 if removed or added or changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
