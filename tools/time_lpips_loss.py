#!/usr/bin/env python3
"""Time the `lpips` loss term: LPIPS(differentiable=True) forward + backward at B = 32, 224 x 224 (and the forward-only metric beside it),
the captured BASELINE config-2 training step with the term added against the step without it -- in this tree and, with --parent, in a
checkout of the parent commit (built: its hifihr_amd/libhifihr.so exists) in the same run.

    python tools/time_lpips_loss.py [--parent PATH] [--out profiles/lpips_loss_time.txt]

Module figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: every step is captured and timed in a process of its own (the same script text in either tree, so both are measured the
same way), HIP events around `--steps` replays, the median of `--rounds` windows, per step; the processes run one after the other, the
whole sequence `--alternations` times.  There is no pass threshold: the file is the record."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# runs with cwd = the tree to measure; uses only what both this tree and its parent have
STEP_SCRIPT = r"""
import json, statistics, sys, warnings
sys.path.insert(0, ".")
import torch
from hifihr_amd import options, synth
from hifihr_amd.losses import LossFunction
from hifihr_amd.mano_tables import synthetic_mano_tables
from hifihr_amd.models import Model
from hifihr_amd.optim import FlatParams, FusedAdam
from hifihr_amd.traineval import GraphedTrainStep, data_dic
warnings.simplefilter("ignore")
B, extra, warmup, steps, rounds = int(sys.argv[1]), [k for k in sys.argv[2].split(",") if k], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
dev, tables = torch.device("cuda"), synthetic_mano_tables(0)
torch.cuda.set_stream(torch.cuda.Stream())
base = options.baseline_config2_args(train_batch=B)
args = options.baseline_config2_args(train_batch=B, losses=base.losses + extra)
torch.manual_seed(0)
model = Model(True, dev, False, "mano", False, "res18", mano_tables=tables).to(dev).train()
opt = FusedAdam(FlatParams(model), lr=1e-6)
ex = data_dic(synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, device=dev), "FreiHand", "training", args, device=dev)
g = GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=3)
for _ in range(warmup):
    g()
torch.cuda.synchronize()
out = []
for _ in range(rounds):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        g()
    b.record()
    b.synchronize()
    out.append(a.elapsed_time(b) / steps)
print("STEP_MS " + json.dumps(out))
"""


def gpu_ms(fn, warmup, repeats, rounds):
    import torch
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


def module_rows(cli, lines):
    import torch
    sys.path.insert(0, REPO)
    from hifihr_amd.lpips import LPIPS
    B = cli.batch
    gen = torch.Generator().manual_seed(0)
    in0 = torch.rand(B, 3, 224, 224, generator=gen).cuda().requires_grad_(True)
    in1 = torch.rand(B, 3, 224, 224, generator=gen).cuda()
    lines.append(f"LPIPS(net='alex') at B = {B}, 224 x 224, inputs in [0, 1] (normalize=True), seeded weights")
    for prec in ("reference", "fast"):
        metric, diff = LPIPS(conv_precision=prec).cuda(), LPIPS(conv_precision=prec, differentiable=True).cuda()

        def fwd_only():
            with torch.no_grad():
                metric(in0, in1, normalize=True)

        def fwd_diff():
            diff(in0, in1, normalize=True)

        def fwd_bwd():
            in0.grad = None
            diff(in0, in1, normalize=True).mean().backward()

        for name, fn in ((f"conv_precision={prec}: forward-only metric", fwd_only), (f"conv_precision={prec}: differentiable forward (maps kept)", fwd_diff),
                         (f"conv_precision={prec}: differentiable forward + backward", fwd_bwd)):
            med, lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds)
            lines.append(f"  MI355X  {name:62s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]")
    lines.append("")


def step_ms(tree, cli, extra):
    """One process per measurement: a fresh child (never a replaced program) that captures the step and prints its windows."""
    r = subprocess.run([sys.executable, "-c", STEP_SCRIPT, str(cli.batch), ",".join(extra), str(cli.warmup), str(cli.steps), str(cli.rounds)],
                       cwd=tree, capture_output=True, text=True, timeout=cli.child_timeout)
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_MS ")]
    if r.returncode != 0 or not rows:
        raise RuntimeError(f"the step measurement in {tree} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(rows[-1][len("STEP_MS "):])


def step_rows(cli, lines):
    runs = [("this tree, config 2 as it is", REPO, []), ("this tree, config 2 + lpips", REPO, ["lpips"])]
    if cli.parent:
        runs.insert(0, ("parent commit, config 2 as it is", os.path.abspath(cli.parent), []))
    samples = {tag: [] for tag, _, _ in runs}
    for _ in range(cli.alternations):
        for tag, tree, extra in runs:
            samples[tag] += step_ms(tree, cli, extra)
    lines.append(f"captured training step, ResNet-18 + MANO + render, B = {cli.batch}: ms/step, median [min .. max] of {cli.alternations} x {cli.rounds} "
                 f"windows of {cli.steps} replays, one process per measurement, the rows alternated")
    med = {}
    for tag, v in samples.items():
        med[tag] = statistics.median(v)
        lines.append(f"  MI355X  {tag:62s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    a, b = med[runs[-2][0]], med[runs[-1][0]]
    lines.append(f"  cost of the term: {b - a:+.4f} ms/step ({100 * (b - a) / a:+.2f} %)")
    if cli.parent:
        p, v = med[runs[0][0]], samples[runs[0][0]]
        lines.append(f"  this tree without the term against the parent commit: {a - p:+.4f} ms/step ({100 * (a - p) / p:+.2f} %); "
                     f"the parent's own windows spread over {max(v) - min(v):.4f} ms")
    else:
        lines.append("  (no --parent tree was given: the parent commit was not measured)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_loss_time.txt"))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    cli = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    argv = [a if not (i > 0 and sys.argv[1:][i - 1] in ("--parent", "--out")) else "<path>" for i, a in enumerate(sys.argv[1:])]
    lines = ["`lpips` loss term (LPIPS(alex) with a HIP backward): time per call / per step (ms), median [min .. max]",
             "command: python tools/time_lpips_loss.py " + " ".join(argv),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    module_rows(cli, lines)
    step_rows(cli, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
