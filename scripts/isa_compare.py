#!/usr/bin/env python3
"""Same instructions before and after a change that should only move code.

    python scripts/isa_compare.py emit DIR [file.hip ...]   device assembly of the kernels, built with the Makefile's HIPFLAGS
    python scripts/isa_compare.py diff DIR_A DIR_B          per function: instruction text and resource counts

`emit` writes DIR/<file>.s (default: the four per-slot image products).  Run it on the tree before the change and on
the tree after it, then `diff` the two directories.  The comparison drops comments and directives, numbers the local
labels of a function by first appearance, and reads .vgpr_count, .sgpr_count, .group_segment_fixed_size and
.private_segment_fixed_size (scratch) from the code object metadata.  Exit status 1 when anything differs."""
import difflib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ripcurrents_amd", "csrc")
DEFAULT = ["timex_kernels.hip", "stab_kernels.hip", "warp_kernels.hip", "ripmap_kernels.hip"]
COUNTS = [".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size"]


def makefile_var(text, name):
    m = re.search(r"^%s \?= ((?:.*\\\n)*.*)" % name, text, re.M)
    return m.group(1).replace("\\\n", " ")


def emit(outdir, files):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = makefile_var(mk, "HIPFLAGS").replace("$(ARCH)", makefile_var(mk, "ARCH")).split()
    os.makedirs(outdir, exist_ok=True)
    for f in files:
        out = os.path.join(outdir, os.path.splitext(os.path.basename(f))[0] + ".s")
        extra = makefile_var(mk, "EXTRA_" + os.path.splitext(f)[0]).split() if "EXTRA_" + os.path.splitext(f)[0] in mk else []
        subprocess.check_call([makefile_var(mk, "HIPCC")] + flags + extra + ["-S", "--cuda-device-only", "-o", out, f], cwd=CSRC)
        print("wrote", out)


def functions(text):
    """name -> normalised instruction lines of every function in a device assembly listing"""
    out = {}
    names = re.findall(r"^\t\.type\t(\S+),@function", text, re.M)
    for name in names:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
        labels = {}
        lines = []
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or ln.lstrip().startswith("."):
                if re.match(r"^\.L\w+:", ln):
                    lines.append(labels.setdefault(ln.rstrip(":"), "L%d" % len(labels)) + ":")
                continue
            ln = re.sub(r"\.L\w+", lambda k: labels.setdefault(k.group(0), "L%d" % len(labels)), ln)
            lines.append(" ".join(ln.split()))
        out[name] = lines
    return out


def counts(text):
    """kernel name -> the resource counts of its metadata entry"""
    out = {}
    meta = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if name:                          # the version list after the kernels splits the same way
            out[name.group(1)] = {c: int(re.search(r"^    %s:\s+(\d+)" % re.escape(c), entry, re.M).group(1)) for c in COUNTS}
    return out


def diff(a, b):
    bad = 0
    for f in sorted(os.listdir(a)):
        if not f.endswith(".s"):
            continue
        ta, tb = open(os.path.join(a, f)).read(), open(os.path.join(b, f)).read()
        fa, fb, ca, cb = functions(ta), functions(tb), counts(ta), counts(tb)
        for name in sorted(set(fa) | set(fb)):
            la, lb = fa.get(name), fb.get(name)
            if la is None or lb is None:
                print("%s %s: only in %s" % (f, name, a if lb is None else b))
                bad += 1
                continue
            same = la == lb and ca.get(name) == cb.get(name)
            n = sum(1 for x in la if not x.endswith(":"))
            print("%s %-60s %5d instructions %s  %s" % (f, name, n, ca.get(name, ""), "same" if same else "DIFFERENT"))
            if not same:
                bad += 1
                print("  after: %d instructions %s" % (sum(1 for x in lb if not x.endswith(":")), cb.get(name, "")))
                sys.stdout.writelines("  " + d + "\n" for d in list(difflib.unified_diff(la, lb, "before", "after", lineterm="", n=1))[:60])
    print("%d function(s) differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3:] or DEFAULT)
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
