"""What the small "glue" launches of a training step cost: from a rocprofv3 --kernel-trace CSV, for every kernel whose name matches one of
the glue patterns, its own duration AND the idle time of the GPU directly before and after it (the gap between the end of the last kernel
that ran before it and its start, and between its end and the start of the next kernel; time in which another kernel -- the dB / dC fold
on its side stream -- runs is not idle).  A gap shared by two neighbouring glue launches is counted once.  The sum of the two columns is
what removing these launches can give back at most.
    python tools/trace_glue.py <dir or kernel_trace.csv> [steps] [pattern ...]"""
import sys
from collections import defaultdict

from trace_overlap import load

GLUE = ("FillFunctor", "fold_f32_multi_kernel", "direct_copy", "MulFunctor", "__amd_rocclr_copyBuffer", "CatArrayBatchedCopy",
        "reduce_partials", "mixer_finish_kernel", "__amd_rocclr_fillBuffer")
MAX_GAP_NS = 100_000  # a longer hole is the host (step boundary, synchronisation), not a drain-and-ramp around a small launch


def main():
    rows = load(sys.argv[1])
    steps = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    pats = tuple(sys.argv[3:]) or GLUE
    # busy intervals of the whole GPU (union over streams), then the holes between them
    merged = []  # [start, end, [row indices]]
    for i, (a, b, _n) in enumerate(rows):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
            merged[-1][2].append(i)
        else:
            merged.append([a, b, [i]])
    is_glue = lambda i: any(p in rows[i][2] for p in pats)
    key = lambda i: next(p for p in pats if p in rows[i][2])
    dur, cnt, gap = defaultdict(int), defaultdict(int), defaultdict(int)
    for i, (a, b, _n) in enumerate(rows):
        if is_glue(i):
            dur[key(i)] += b - a
            cnt[key(i)] += 1
    holes = holes_all = 0
    for j in range(1, len(merged)):
        g = merged[j][0] - merged[j - 1][1]
        if g > MAX_GAP_NS:
            continue
        holes_all += g
        # the hole belongs to a glue launch if the busy interval on either side of it is glue only (a glue launch covered by a big
        # kernel of another stream drains nothing)
        left = merged[j - 1][2] if all(is_glue(i) for i in merged[j - 1][2]) else None
        right = merged[j][2] if all(is_glue(i) for i in merged[j][2]) else None
        if left is None and right is None:
            continue
        holes += g
        owners = ([left[-1]] if left else []) + ([right[0]] if right else [])
        for i in owners:
            gap[key(i)] += g / len(owners)
    print(f"{steps:g} steps traced; holes of at most {MAX_GAP_NS / 1e3:.0f} us between busy intervals: {holes_all / steps / 1e6:.3f} ms/step in all, "
          f"{holes / steps / 1e6:.3f} ms/step next to a glue launch")
    print(f"{'kernel ms/step':>15} {'idle next to it ms/step':>24} {'calls/step':>11}  kernel")
    for p in sorted(dur, key=lambda k: -(dur[k] + gap[k])):
        print(f"{dur[p] / steps / 1e6:15.3f} {gap[p] / steps / 1e6:24.3f} {cnt[p] / steps:11.1f}  {p}")
    td, tg = sum(dur.values()), sum(gap.values())
    print(f"{td / steps / 1e6:15.3f} {tg / steps / 1e6:24.3f} {sum(cnt.values()) / steps:11.1f}  total; ceiling = {(td + tg) / steps / 1e6:.3f} ms/step")


if __name__ == "__main__":
    main()
