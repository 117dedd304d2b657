"""Times one LPIPS(net="alex") call (hifihr_amd/lpips.py) at N = 32, 224 x 224 and writes profiles/lpips_time.txt:
the milliseconds per call (device events around warmed calls, profiler off), a `rocprofv3 --kernel-trace --stats` table of the same
call taken in a run of its own, and the achieved GB/s of each tap launch against its compulsory bytes 2 * B * HW * C * 4.

usage: python tools/time_lpips.py [--out profiles/lpips_time.txt] [--n 32] [--precision reference]
Each GPU step is a child process under its own `timeout`; after a step that fails nothing more is started."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# tap -> (HW, C, the kernel instance that serves it) at 224 x 224
TAPS = ((3025, 64, "lpips_tap_kernel<16, 1>"), (729, 192, "lpips_tap_kernel<16, 3>"), (169, 384, "lpips_tap_kernel<32, 3>"),
        (169, 256, "lpips_tap_kernel<64, 1>"), (169, 256, "lpips_tap_kernel<64, 1>"))


def worker(mode, n, precision, calls):
    import torch
    from hifihr_amd.lpips import LPIPS
    assert torch.cuda.is_available(), "time_lpips needs a GPU: there is no fallback"
    torch.cuda.set_stream(torch.cuda.Stream())
    gen = torch.Generator().manual_seed(0)
    in0 = (torch.rand(n, 3, 224, 224, generator=gen) * 2 - 1).cuda()
    in1 = (torch.rand(n, 3, 224, 224, generator=gen) * 2 - 1).cuda()
    m = LPIPS(conv_precision=precision).cuda()
    for _ in range(5):
        out = m(in0, in1)
    torch.cuda.synchronize()
    if mode == "call":                       # under rocprofv3
        for _ in range(calls):
            out = m(in0, in1)
        torch.cuda.synchronize()
        return
    reps = []
    for _ in range(5):                       # five windows of `calls` calls: the spread is reported with the figure
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = m(in0, in1)
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) / calls)
    print("RESULT " + json.dumps({"ms": reps, "n": n, "precision": precision, "calls": calls, "value0": float(out.reshape(-1)[0]),
                                  "device": torch.cuda.get_device_name(0)}))


def run(cmd, seconds):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, cwd=REPO, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {' '.join(cmd[:6])} ... ended with status {r.returncode}: nothing more is started")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_time.txt"))
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--precision", default="reference", choices=["reference", "fast"])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--worker", default=None, choices=["time", "call"])
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.n, a.precision, a.calls)
    me = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--calls", str(a.calls)]
    lines = [f"LPIPS(net='alex') forward, N = {a.n}, 224 x 224 (tools/time_lpips.py).  Recorded, not gated: there is no parent to compare with.", ""]
    results = {}
    for prec in ("reference", "fast"):
        out = run(me + ["--precision", prec, "--worker", "time"], 300)
        res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
        results[prec] = res
        ms = sorted(res["ms"])
        lines.append(f"conv_precision={prec!r:12s} {ms[len(ms) // 2]:.3f} ms per call (median of 5 windows of {res['calls']} calls, device events, "
                     f"profiler off; min {ms[0]:.3f}, max {ms[-1]:.3f}) on {res['device']}")
    lines.append("")
    if shutil.which("rocprofv3") is None:
        lines.append("rocprofv3 not found: kernel table not measured")
    else:
        tmp = tempfile.mkdtemp(prefix="lpips_prof_")
        calls = 10
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
             "--n", str(a.n), "--calls", str(calls), "--precision", a.precision, "--worker", "call"], 600)
        stats = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            lines.append("rocprofv3 wrote no kernel_stats.csv: kernel table not measured")
        else:
            rows = list(csv.DictReader(open(stats[0])))
            total = sum(float(r["TotalDurationNs"]) for r in rows)
            lines.append(f"rocprofv3 --kernel-trace --stats of the same call (conv_precision={a.precision!r}; 5 warm-up + {calls} calls in the trace; "
                         f"a run of its own, tracing on):")
            lines.append(f"{'calls':>6s} {'avg us':>9s} {'share':>7s}  kernel")
            for r in rows:
                lines.append(f"{int(r['Calls']):6d} {float(r['AverageNs']) / 1e3:9.1f} {float(r['TotalDurationNs']) / total * 100:6.1f}%  {r['Name'][:150]}")
            lines.append("")
            lines.append(f"tap launches against their compulsory bytes 2 * B * HW * C * 4 (B = {a.n}; kernel time = rocprofv3 average of the instance):")
            for i, (hw, c, inst) in enumerate(TAPS):
                hit = [r for r in rows if inst in r["Name"]]
                nb = 2 * a.n * hw * c * 4
                if hit:
                    us = float(hit[0]["AverageNs"]) / 1e3
                    lines.append(f"  tap {i + 1}: HW {hw:5d} C {c:3d}  {nb / 1e6:7.2f} MB  {us:7.1f} us  {nb / us / 1e3:8.1f} GB/s   ({inst})")
                else:
                    lines.append(f"  tap {i + 1}: HW {hw:5d} C {c:3d}  {nb / 1e6:7.2f} MB  not measured ({inst} not in the table)")
            # the launches of the LAST call in the trace, in order: the stem is the first launch after the two repacks
            traces = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True))
            if traces:
                tr = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"]))
                firsts = [i for i, r in enumerate(tr) if "image_scale_to_nhwc4_kernel" in r["Kernel_Name"]
                          and (i == 0 or "image_scale_to_nhwc4_kernel" not in tr[i - 1]["Kernel_Name"])]
                last = tr[firsts[-1]:] if firsts else []
                busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in last)
                lines.append("")
                lines.append(f"the last call of the trace, launch by launch ({len(last)} launches, {busy / 1e3:.1f} us of kernel time, "
                             f"{(int(last[-1]['End_Timestamp']) - int(last[0]['Start_Timestamp'])) / 1e3:.1f} us first start to last end):" if last else "no call found in the trace")
                for j, r in enumerate(last):
                    d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                    note = "   <- the 11 x 11 stem (C = 4, one plane zero)" if j == 2 else ""
                    lines.append(f"  {d / 1e3:8.1f} us {d / busy * 100:5.1f}%  {r['Kernel_Name'][:110]}{note}")
                if len(last) > 2:
                    d = int(last[2]["End_Timestamp"]) - int(last[2]["Start_Timestamp"])
                    lines.append(f"the stem takes {d / busy * 100:.1f} % of the call's kernel time: " + ("MORE than half -- the input a later change would need"
                                                                                                      if d > busy / 2 else "not more than half"))
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
