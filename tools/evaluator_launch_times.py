"""Per-launch times of the four NeO-360 evaluator launches of a frame, from `rocprofv3 --kernel-trace -f csv` output directories of
`bench.py --gpus 1 --steps K --warmup W` (one directory per side, e.g. the parent commit's library and this tree's).
usage: evaluator_launch_times.py <label>=<dir> [<label>=<dir> ...] [--skip N]
Prints mean (min .. max) in ms per launch kind and side - the first N launches of every kind are skipped (default 1: the first frame
loads code objects) - and, with two sides, whether the second side's slowest launch is below the first side's fastest (the
criterion of profiles/quad_order.log)."""
import csv
import glob
import json
import os
import re
import sys

KINDS = ("inside coarse", "outside coarse", "inside fine", "outside fine")


def kind_of(name):
    """The launch kind behind a kernel name of the default frame (pre-projection mode 3, density-only coarse level):
    k_tp_mlp_hp<3, ..> inside, k_tp_mlp_hpp<4, ..> outside the sphere; <.., false, true> (DENS) is the coarse level."""
    m = re.search(r"k_tp_mlp_(hpp?)<(\d), (\w+), (\w+)>", name)
    if not m or m.group(3) != "false" or (m.group(1), m.group(2)) not in (("hp", "3"), ("hpp", "4")):
        return None
    return ("inside " if m.group(1) == "hp" else "outside ") + ("coarse" if m.group(4) == "true" else "fine")


def by_kind(root):
    """kind -> [ms] of every evaluator dispatch under a rocprofv3 output directory, in time order."""
    rows = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = kind_of(r["Kernel_Name"])
            if k:
                rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, k))
    out = {k: [] for k in KINDS}
    for _, ms, k in sorted(rows):
        out[k].append(ms)
    assert all(out.values()), "no evaluator launches of some kind under %s: %s" % (root, {k: len(v) for k, v in out.items()})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    skip = int(sys.argv[sys.argv.index("--skip") + 1]) if "--skip" in sys.argv else 1
    args = [a for a in args if "=" in a]
    sides = [(a.split("=", 1)[0], by_kind(a.split("=", 1)[1])) for a in args]
    rec = {}
    for kind in KINDS:
        line = "%-15s" % kind
        for label, d in sides:
            v = d[kind][skip:]
            rec.setdefault(kind, {})[label] = v
            line += "  %s %8.2f (%8.2f .. %8.2f) ms, %d launches" % (label, sum(v) / len(v), min(v), max(v), len(v))
        if len(sides) == 2:
            a, b = rec[kind][sides[0][0]], rec[kind][sides[1][0]]
            line += "  %+5.1f %%  %s" % (100.0 * (sum(b) / len(b) / (sum(a) / len(a)) - 1.0),
                                         "CLEARS (slowest %s < fastest %s)" % (sides[1][0], sides[0][0]) if max(b) < min(a) else "does not clear")
        print(line)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
