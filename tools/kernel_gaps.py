"""gaps between the kernels of an EM step in a rocprofv3 kernel trace: the M-step's end to the next weight pass's start, the weight
pass's end to the sweep's start, the step from weight pass to weight pass, and every kernel's average and deviation.

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 bench.py --config c4 --steps 40 --warmup 3 \
      --no-cpu-baseline --no-secondary --no-exchange-loopback
  python3 tools/kernel_gaps.py OUT/.../*_kernel_trace.csv [label]

(profiles/measurement_log_weights_ahead.md)"""
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
names = [r["Kernel_Name"] for r in rows]
S = [int(r["Start_Timestamp"]) for r in rows]
E = [int(r["End_Timestamp"]) for r in rows]


def first_after(i, pat):
    for j in range(i + 1, min(i + 12, len(rows))):
        if pat in names[j]:
            return j
    return None


m2w, w2s, step = [], [], []
last_w = None
for i, n in enumerate(names):
    if "mstep_wide_kernel" in n:
        j = first_after(i, "trans_w_bucket_kernel")
        if j is not None:
            m2w.append((S[j] - E[i]) / 1e3)
    if "trans_w_bucket_kernel" in n:
        j = first_after(i, "tile_sweep_kernel")
        if j is None:
            j = i + 1 if i + 1 < len(rows) else None
        if j is not None:
            w2s.append((S[j] - E[i]) / 1e3)
        if last_w is not None:
            step.append((S[i] - last_w) / 1e3)
        last_w = S[i]


def q(v):
    v = sorted(v)
    if not v:
        return "none"
    return "n=%d median %.2f p10 %.2f p90 %.2f us" % (len(v), statistics.median(v), v[len(v) // 10], v[(9 * len(v)) // 10])


print(sys.argv[2] if len(sys.argv) > 2 else "", "mstep_wide end -> trans_w_bucket start:", q(m2w[3:]))
print(sys.argv[2] if len(sys.argv) > 2 else "", "trans_w_bucket end -> next kernel start:", q(w2s[3:]))
print(sys.argv[2] if len(sys.argv) > 2 else "", "weight pass start to weight pass start:", q(step[3:]))
kn = {}
for n, s, e in zip(names, S, E):
    k = n.replace("carmel_hip::", "").replace("void ", "")[:70]
    kn.setdefault(k, []).append((e - s) / 1e3)
for k, v in sorted(kn.items(), key=lambda kv: -sum(kv[1])):
    if len(v) > 5:
        print("   %-72s calls %4d avg %8.1f us sd %6.1f" % (k, len(v), statistics.mean(v), statistics.pstdev(v)))
