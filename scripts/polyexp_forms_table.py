#!/usr/bin/env python3
"""profiles/polyexp_forms_parity.md from a log of tests/test_gpu_polyexp_forms.py:

    python -m pytest -m gpu -s tests/test_gpu_polyexp_forms.py > forms.log
    python scripts/polyexp_forms_table.py forms.log > profiles/polyexp_forms_parity.md

Every "[forms] part | form | parameters | case | per-channel maxima | max | oracle noise | bar" line is one comparison of a
launch's R with oracle.polyexp.  The table has one row per (part, form, parameters): the number of comparisons, the largest
|dR| among them, where it occurred, its channels, and the oracle's own rounding noise (against float64) on that image.
"""
import re
import sys
from collections import OrderedDict


def main(path):
    rows = OrderedDict()
    total = 0
    for line in open(path):
        m = re.search(r"\[forms\] (.+?) \| (.+?) \| (.+?) \| (.+?) \| (.+?) \| max (\S+) \| oracle noise (\S+) \| bar (\S+)", line)
        if not m:
            continue
        part, form, prm, case, chans, mx, noise, bar = m.groups()
        total += 1
        key = (part, form, prm)
        r = rows.setdefault(key, dict(n=0, max=-1.0))
        r["n"] += 1
        if float(mx) > r["max"]:
            r.update(max=float(mx), case=case, chans=chans, noise=float(noise), bar=float(bar))
    worst = max(rows.items(), key=lambda kv: kv[1]["max"] / kv[1]["bar"])
    print("# Polynomial expansion: every form against the oracle\n")
    print("Measured on an MI355X by tests/test_gpu_polyexp_forms.py (this table: scripts/polyexp_forms_table.py).  |dR| is the")
    print("largest absolute difference from oracle.polyexp over the comparisons of a row (sizes, scales, frames); \"noise\" is the")
    print("oracle's own rounding against the float64 np_oracle.polyexp on the image of the worst comparison.  Bar: 2e-4, for the")
    print("hostile bytes 2e-4 x max(1, s_hostile / s_surf) from the reference alone.\n")
    print("%d comparisons in %d rows.  Worst against its bar: %s, %s, %s, %s: %.3g (noise %.3g, bar %.3g).\n" % (
        total, len(rows), worst[0][0], worst[0][1], worst[0][2], worst[1]["case"], worst[1]["max"], worst[1]["noise"], worst[1]["bar"]))
    print("| part | form | parameters | comparisons | max |dR| | at | channels there | oracle noise | bar |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (part, form, prm), r in rows.items():
        print("| %s | `%s` | %s | %d | %.3g | %s | %s | %.3g | %.3g |" % (part, form, prm, r["n"], r["max"], r["case"], r["chans"], r["noise"], r["bar"]))


if __name__ == "__main__":
    main(sys.argv[1])
