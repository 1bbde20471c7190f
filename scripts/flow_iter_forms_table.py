#!/usr/bin/env python3
"""Turns a log of tests/test_gpu_flow_forms.py (pytest -s: its "[flow-forms] ..." lines) into the table of
profiles/flow_iter_forms_parity.md:

    python -m pytest -m gpu -q -s tests/test_gpu_flow_forms.py > forms.log
    python scripts/flow_iter_forms_table.py forms.log > profiles/flow_iter_forms_parity.md

One row per form and case for the three cases of every form with the largest ratio to the oracle's figure, and the number of
cases behind them.  q = e (det + 1e-3) over every pixel, e over the pixels with det > 1e-2; ratio = the larger of the two
kernel / oracle quotients.  A quotient above the factor with nothing missed passed under the ulp floor (8 float32 ulps of the
field's largest flow, the "floor" column; "under floor" counts the pixels it decided) or, where the case column names a float32
restatement, within 1.25x of that restatement and 5x the oracle.
"""
import collections
import re
import sys

LINE = re.compile(r"\[flow-forms\] (?P<part>[^|]+?) \| (?P<form>[^|]+?) \| (?P<size>\d+x\d+) \| (?P<what>[^|]+?) \| q oracle (?P<qo>\S+) kernel (?P<qk>\S+) \| "
                  r"e\(det>1e-2\) oracle (?P<eo>\S+) kernel (?P<ek>\S+) \| e\(all\) oracle \S+ kernel \S+ \| ratio (?P<ratio>\S+) of (?P<factor>\S+) \| "
                  r"floor (?P<floor>\S+) \| under floor (?P<under>\d+) \| excluded (?P<excl>\S+) % \| miss (?P<miss>\d+)(?P<restated> \| restated .*)?")
COPY = re.compile(r"\[flow-forms\] (?P<part>[^|]+?) \| (?P<form>[^|]+? solve=0 [^|]+?) \| (?P<size>\d+x\d+) \| (?P<what>[^|]+?) \| max err (?P<err>\S+) \| bar (?P<bar>\S+)")


def main(path):
    forms, copies = collections.OrderedDict(), []
    for line in open(path, errors="replace"):
        m = LINE.search(line)
        if m:
            forms.setdefault((m["part"], m["form"]), []).append(m.groupdict())
            continue
        m = COPY.search(line)
        if m:
            copies.append(m.groupdict())
    print("# Flow-iteration forms against the float64 reference of one launch\n")
    print("Measured by tests/test_gpu_flow_forms.py on an MI355X; regenerate with scripts/flow_iter_forms_table.py.  The oracle column")
    print("is the C++ float oracle against the same float64 reference on the same inputs (the yardstick), the kernel column the HIP")
    print("kernel.  q = e (det + 1e-3) over every pixel; e over the pixels with det > 1e-2.  floor = 8 float32 ulps of the field's")
    print("largest flow, in px; under floor = pixels beyond the factor that pass because their error is below that floor: where a")
    print("ratio exceeds its factor and nothing is missed, the floor (or the named float32 restatement) decided the row.\n")
    print("| part | form | cases | worst cases: size, input | q oracle | q kernel | e oracle | e kernel | ratio | factor | floor | under floor | excluded % | missed |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for (part, form), rows in forms.items():
        rows.sort(key=lambda r: -float(r["ratio"]))
        for i, r in enumerate(rows[:3]):
            case = "%s, %s%s" % (r["size"], r["what"], " (float32 restatement:%s)" % r["restated"].replace(" | restated", "") if r["restated"] else "")
            print("| %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (
                part, form, len(rows) if i == 0 else "", case, r["qo"], r["qk"], r["eo"], r["ek"], r["ratio"], r["factor"], r["floor"], r["under"],
                r["excl"], r["miss"]))
    if copies:
        print("\n## iterations = 0: the up-sampled field itself against oracle.resize_linear\n")
        print("| form | size | pyr_scale | max error | bar (4 ulp of the largest flow) |")
        print("|---|---|---|---|---|")
        for r in copies:
            print("| %s | %s | %s | %s | %s |" % (r["form"], r["size"], r["what"].replace("ps", ""), r["err"], r["bar"]))
    total = sum(len(v) for v in forms.values())
    missed = sum(int(r["miss"]) > 0 for v in forms.values() for r in v)
    floored = sum(int(r["under"]) > 0 for v in forms.values() for r in v)
    restated = sum(bool(r["restated"]) for v in forms.values() for r in v)
    print("\n%d launches compared, %d with a pixel beyond its bar; %d launches have pixels that pass under the ulp floor alone, %d on "
          "the float32 restatement." % (total, missed, floored, restated))


if __name__ == "__main__":
    main(sys.argv[1])
