#!/usr/bin/env python
"""Per kernel family, what a change of the output stores' cache policy did inside the frame (write-through A/B).

  python tools/wt_compare.py <frame_trace_base.csv> <frame_trace_variant.csv> [--classes]
  python tools/wt_compare.py profiles/wt_frame_traces.csv:b2_parent profiles/wt_frame_traces.csv:b2_head [--classes]

Both inputs are tools/frame_trace.py outputs of the SAME plan (one row per launch: in-frame duration and the gap to the next
dispatch), or `file:column` of a table that holds several traces side by side (columns <column>_us, <column>_gap).  For every
family the table gives, summed over its launches: their duration (base, variant), the gaps behind them (duration + gap is the
start-to-start interval to the successor; the gaps are bimodal under the profiler, so they are shown, not judged), and the
duration of the launches that directly FOLLOW one of its launches (they read what it wrote: a write-through store drops the line
from the producing XCD's L2).  The last line is the sum over all launches, i.e. the frame.  --classes: the same per launch and
launch class (kernel, dims), largest classes first."""
import csv
import sys


def load(spec):
    path, _, col = spec.partition(":")
    us, gap = (col + "_us", col + "_gap") if col else ("us_in_frame", "gap_us")
    return [(r["kernel"], r["dims"], float(r[us]), float(r[gap])) for r in csv.DictReader(open(path))]


def row(name, idx, succ, base, var, per):
    s = lambda t, S, c: sum(t[j][c] for j in S) / per
    print(f"{name[:56]:56s} {len(idx):4d} {s(base, idx, 2):9.2f} {s(var, idx, 2):9.2f} {s(base, idx, 3):9.2f} {s(var, idx, 3):9.2f} "
          f"{s(base, succ, 2):9.2f} {s(var, succ, 2):9.2f} {s(var, idx, 2) + s(var, succ, 2) - s(base, idx, 2) - s(base, succ, 2):+9.2f}")


def main():
    base, var = load(sys.argv[1]), load(sys.argv[2])
    assert [b[:2] for b in base] == [v[:2] for v in var], "the two traces are not of the same plan"
    n = len(base)
    head = f"{'n':>4s} {'dur base':>9s} {'dur var':>9s} {'gap base':>9s} {'gap var':>9s} {'succ base':>9s} {'succ var':>9s} {'d(dur+succ)':>9s}"
    print(f"{'family (us per frame)':56s} {head}")
    for f in sorted({b[0] for b in base}):
        idx = [j for j in range(n) if base[j][0] == f]
        succ = [j + 1 for j in idx if j + 1 < n and base[j + 1][0] != f]       # (a same-family successor is already in `dur`)
        row(f, idx, succ, base, var, 1)
    row("frame (all launches)", list(range(n)), [], base, var, 1)
    if "--classes" in sys.argv:
        cls = {}
        for j in range(n):
            cls.setdefault(base[j][:2], []).append(j)
        print(f"\n{'class (us per launch)':56s} {head}")
        for (k, d), idx in sorted(cls.items(), key=lambda kv: -sum(base[j][2] for j in kv[1])):
            row(k + " " + d, idx, [j + 1 for j in idx if j + 1 < n], base, var, len(idx))


if __name__ == "__main__":
    main()
