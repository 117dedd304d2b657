#!/usr/bin/env python3
"""Time hifihr_amd.evaluate.fscore and pck_auc on the GPU at the FreiHAND evaluation split's size (n = 3960, 778 vertices, 21 joints)
and at one val_batch = 8 call, next to the float64 numpy restatement of tests/benchmark_ref.py on the same box's host.

    python tools/time_benchmark_metrics.py [--out profiles/benchmark_metrics_time.txt]

GPU figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call;
`fscore` is the memset + kernel, `pck_auc` the kernel + the two device-to-host copies + the host's float64 curve arithmetic (a host
clock around a call that ends synchronised).  The restatement is timed on `--cpu-samples` samples and scaled to n (it is a per-sample
loop); there is no pass threshold, the file is the record."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def gpu_ms(fn, warmup, repeats, rounds):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / repeats)
    return statistics.median(out), min(out), max(out)


def host_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return statistics.median(out), min(out), max(out)


def main():
    import benchmark_ref as br
    from hifihr_amd import evaluate
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "benchmark_metrics_time.txt"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-samples", type=int, default=24)
    cli = ap.parse_args()
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    rng = np.random.default_rng(0)
    lines = ["benchmark metrics: time per call (ms), median [min .. max]",
             "command: python tools/time_benchmark_metrics.py " + " ".join(sys.argv[1:]),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    thr = np.linspace(0.0, 0.05, 100)
    for n in (3960, 8):
        gt_v = (0.05 * rng.standard_normal((n, 778, 3))).astype(np.float32)
        pr_v = (gt_v + 0.006 * rng.standard_normal((n, 778, 3))).astype(np.float32)
        gt_j, pr_j = gt_v[:, :21].copy(), pr_v[:, :21].copy()
        d = {k: torch.from_numpy(v).cuda() for k, v in dict(gt_v=gt_v, pr_v=pr_v, gt_j=gt_j, pr_j=pr_j).items()}
        rows = [("fscore         [n,778]x[n,778], 2 thresholds", "gpu", lambda: evaluate.fscore(d["pr_v"], d["gt_v"])),
                ("hist kernel    [n,778,3], 100 thresholds", "gpu", lambda: evaluate.point_error_counts(d["pr_v"], d["gt_v"], None, thr)),
                ("hist kernel    [n,21,3], 100 thresholds", "gpu", lambda: evaluate.point_error_counts(d["pr_j"], d["gt_j"], None, thr)),
                ("pck_auc        [n,778,3] (kernel + copies + host curves)", "host", lambda: evaluate.pck_auc(d["pr_v"], d["gt_v"])),
                ("pck_auc        [n,21,3]  (kernel + copies + host curves)", "host", lambda: evaluate.pck_auc(d["pr_j"], d["gt_j"]))]
        lines.append(f"n = {n}")
        for name, how, fn in rows:
            med, lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds) if how == "gpu" else host_ms(fn, cli.warmup, cli.repeats)
            lines.append(f"  MI355X  {name:62s} {med:10.4f}  [{lo:.4f} .. {hi:.4f}]  ({'HIP events' if how == 'gpu' else 'host clock, synchronised'})")
        m = min(n, cli.cpu_samples)
        t = time.perf_counter()
        br.fscore_counts(pr_v[:m], gt_v[:m], (0.005, 0.015))
        cpu_f = 1e3 * (time.perf_counter() - t) * n / m
        t = time.perf_counter()
        br.pck_measures(*br.hist_counts(pr_v[:m], gt_v[:m], None, thr), thr)
        cpu_v = 1e3 * (time.perf_counter() - t) * n / m
        t = time.perf_counter()
        br.pck_measures(*br.hist_counts(pr_j, gt_j, None, thr), thr)
        cpu_j = 1e3 * (time.perf_counter() - t)
        scaled = f"timed on {m} samples, scaled to {n}" if m < n else "timed whole"
        lines.append(f"  host    numpy float64 restatement, F-score counts                     {cpu_f:10.1f}  ({scaled}; {os.cpu_count()} CPUs visible, one used)")
        lines.append(f"  host    numpy float64 restatement, PCK/AUC [n,778,3]                  {cpu_v:10.1f}  ({scaled})")
        lines.append(f"  host    numpy float64 restatement, PCK/AUC [n,21,3]                   {cpu_j:10.1f}  (timed whole)")
        if n == 3960:
            pairs = 2.0 * n * 778 * 778
            med = gpu_ms(rows[0][2], 1, cli.repeats, 3)[0]
            lines.append(f"  F-score: {pairs / 1e9:.2f} G point pairs (both directions) -> {pairs / (med * 1e-3) / 1e9:.0f} G pairs/s; "
                         f"8 fp64 operations a pair (3 subtractions, 3 products, 2 sums) + a compare / select")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
