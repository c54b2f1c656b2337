#!/usr/bin/env python3
"""Are the device functions of two builds the same instructions?

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S csrc/lh_kernels.hip -o new/lh_kernels.s   (and so on)
    scripts/isa_same.py PARENT NEW      two directories of .s files, or two .s files, or "a.s,b.s" lists

The -S output is split into functions (.type NAME,@function up to .size NAME, the kernel descriptor included).
Comments, .loc / .file / .cfi lines and the per-unit __hip_cuid_* symbol are dropped and each function's local
labels (.L...) are renumbered in order of appearance, so moved, reordered or re-included source compares equal.
The text is never interpreted.  Prints same / DIFF / MISSING per function; exit status 1 unless all are the same.
Run by hand against a build of the parent commit (a refactor's "same instructions" claim); no build target uses it.
"""
import glob
import os
import re
import sys

DROP = re.compile(r"^\.(loc|file|cfi_\w+)\b|__hip_cuid_")
START = re.compile(r"^\.type\s+([^,\s]+),@function")
LABEL = re.compile(r"\.L[\w$.]+")


def files(arg):
    if os.path.isdir(arg):
        return sorted(glob.glob(os.path.join(arg, "*.s")))
    return arg.split(",")


def functions(paths):
    out = {}
    for path in paths:
        name, body = None, []
        for raw in open(path):
            line = " ".join(raw.split(";", 1)[0].split())
            if not line or DROP.search(line):
                continue
            m = START.match(line)
            if m:
                name, body = m.group(1), []
            if name is None:
                continue
            body.append(line)
            if line.startswith(".size " + name + ","):
                ids = {}
                text = "\n".join(body)
                out[name] = LABEL.sub(lambda l: ids.setdefault(l.group(0), ".L%d" % len(ids)), text)
                name = None
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(files(sys.argv[1])), functions(files(sys.argv[2]))
    bad = 0
    for name in sorted(set(a) | set(b)):
        verdict = "MISSING" if name not in a or name not in b else "same" if a[name] == b[name] else "DIFF"
        bad += verdict != "same"
        print(f"{verdict:8s}{name}")
    print(f"{len(a)} and {len(b)} functions, {bad} not the same")
    sys.exit(1 if bad or not a else 0)


if __name__ == "__main__":
    main()
