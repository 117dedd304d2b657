#!/usr/bin/env python3
"""Time the Chamfer distance (hifihr_chamfer_fwd / _bwd: the loss term "chamfer") against the formulation a user would otherwise write in
ATen -- torch.cdist(x, y) ** 2, a min over each axis, autograd -- at (B, N, M) = (32, 778, 778) and (48, 5990, 778) in the same run; the
achieved fp64 rate of the search loop; and the captured BASELINE config-2 training step with the term added against the step without it
-- in this tree twice (the run's own A/A noise) and, with --parent, in a checkout of the parent commit (built: its
hifihr_amd/libhifihr.so exists) in the same run.

    python tools/time_chamfer.py [--part kernels|steps|all] [--parent PATH] [--out profiles/chamfer_time.txt]

Kernel figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: every step is captured and timed in a process of its own (the same script text in either tree, so both are measured the
same way), HIP events around `--steps` replays, the median of `--rounds` windows, per step; the processes run one after the other, the
whole sequence `--alternations` times; a child that fails ends the run.  `--part steps` appends to the file `--part kernels` wrote.
There is no pass threshold: the file is the record."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((32, 778, 778), (48, 5990, 778))
# the chip's public fp64 VECTOR figure (AMD's MI355X product page [recalled]; NOT measured in this repository), counted as fused
# multiply-adds = 2 operations each.  The search loop is built without contraction: 8 separate operations per pair, no fma
PUBLIC_FP64_VECTOR_TFLOPS = 78.6
OPS_PER_PAIR = 8                    # 3 subtractions, 3 multiplications, 2 additions; the compare and the selects are not counted

# runs with cwd = the tree to measure; uses only what both this tree and its parent have
STEP_SCRIPT = r"""
import json, statistics, sys
sys.path.insert(0, ".")
import torch
from hifihr_amd import options, synth
from hifihr_amd.losses import LossFunction
from hifihr_amd.mano_tables import synthetic_mano_tables
from hifihr_amd.models import Model
from hifihr_amd.optim import FlatParams, FusedAdam
from hifihr_amd.traineval import GraphedTrainStep, data_dic
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


def aten_chamfer(x, y, w_xy=1.0, w_yx=1.0):
    import torch
    d = torch.cdist(x, y) ** 2
    return w_xy * d.min(2).values.mean(1).mean() + w_yx * d.min(1).values.mean(1).mean()


def kernel_rows(cli, lines):
    import torch
    sys.path.insert(0, REPO)
    from hifihr_amd import ops
    from hifihr_amd._lib import get_lib
    lib = get_lib()
    q, t = lib.chamfer_geometry()
    lines.append(f"kernels: {q} queries per workgroup (4 per lane), {t} searched points per LDS pass; unit weights; ms per call")
    for B, N, M in SHAPES:
        g = torch.Generator().manual_seed(N + M)
        x = ((torch.rand(B, N, 3, generator=g) - 0.5) * 0.2).cuda()
        y = ((torch.rand(B, M, 3, generator=g) - 0.5) * 0.2 + 0.01).cuda()
        idx_xy, idx_yx = torch.empty(B, N, dtype=torch.int32, device="cuda"), torch.empty(B, M, dtype=torch.int32, device="cuda")
        min_xy, min_yx = torch.empty(B, N, dtype=torch.float64, device="cuda"), torch.empty(B, M, dtype=torch.float64, device="cuda")
        sums, out, gout = torch.empty(B, 2, dtype=torch.float64, device="cuda"), torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
        ws = torch.empty(lib.chamfer_workspace_bytes(B, N, M) // 8, dtype=torch.float64, device="cuda")
        gx, gy = torch.empty_like(x), torch.empty_like(y)
        xg = x.clone().requires_grad_(True)
        fwd = lambda: lib.chamfer_fwd(x, y, 1.0, 1.0, idx_xy, idx_yx, min_xy, min_yx, sums, out, ws)

        def ours_autograd():
            xg.grad = None
            ops.chamfer_distance(xg, y).backward()

        def aten_fwd():
            with torch.no_grad():
                aten_chamfer(x, y)

        def aten_autograd():
            xg.grad = None
            aten_chamfer(xg, y).backward()

        rows = [("hifihr_chamfer_fwd (search + finish)", fwd),
                ("hifihr_chamfer_bwd, gx and gy", lambda: lib.chamfer_bwd(x, y, idx_xy, idx_yx, gout, 1.0, 1.0, gx, gy)),
                ("hifihr_chamfer_bwd, gx alone", lambda: lib.chamfer_bwd(x, y, idx_xy, idx_yx, gout, 1.0, 1.0, gx, None)),
                ("ops.chamfer_distance forward + backward to x (autograd)", ours_autograd),
                ("ATen cdist ** 2 + two mins, forward (no_grad)", aten_fwd),
                ("ATen cdist ** 2 + two mins, forward + backward to x", aten_autograd)]
        lines.append(f"  (B, N, M) = ({B}, {N}, {M}); the ATen form materialises B N M floats = {B * N * M * 4 / 1e9:.3f} GB")
        med = {}
        for name, fn in rows:
            med[name], lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds)
            lines.append(f"    MI355X  {name:58s} {med[name]:9.4f}  [{lo:.4f} .. {hi:.4f}]")
        rf, rb = med[rows[4][0]] / med[rows[0][0]], med[rows[5][0]] / med[rows[3][0]]
        lines.append(f"    ATen / kernels: forward {rf:.2f} x, forward + backward {rb:.2f} x"
                     + ("" if rf >= 1.0 and rb >= 1.0 else "   <-- the kernels are SLOWER than the ATen form here"))
        pairs = 2.0 * B * N * M
        rate = pairs * OPS_PER_PAIR / (med[rows[0][0]] * 1e-3) / 1e12
        lines.append(f"    search loop: {pairs:.3e} pairs x {OPS_PER_PAIR} fp64 operations in the forward's time = {rate:.2f} Top/s fp64; the chip's public "
                     f"fp64 vector figure is {PUBLIC_FP64_VECTOR_TFLOPS} TFLOPS counted as fused multiply-adds, i.e. {PUBLIC_FP64_VECTOR_TFLOPS / 2:.1f} "
                     f"T instructions/s for a loop without fma (public figure, UNMEASURED in this repository): {100 * rate / (PUBLIC_FP64_VECTOR_TFLOPS / 2):.0f} % of it")
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
    runs = [("this tree, config 2 as it is (A)", REPO, []), ("this tree, config 2 as it is (A', the same again)", REPO, []),
            ("this tree, config 2 + chamfer", REPO, ["chamfer"])]
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
        lines.append(f"  MI355X  {tag:58s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    a, a2, c = med[runs[-3][0]], med[runs[-2][0]], med[runs[-1][0]]
    noise = abs(a - a2)
    lines.append(f"  A/A noise of this run (|A - A'|): {noise:.4f} ms/step ({100 * noise / a:.2f} %)")
    lines.append(f"  cost of the term: {c - a:+.4f} ms/step ({100 * (c - a) / a:+.2f} %)")
    if cli.parent:
        p = med[runs[0][0]]
        verdict = "within" if abs(a - p) <= noise or abs(a2 - p) <= noise else "OUTSIDE"
        lines.append(f"  this tree without the term against the parent commit: A {a - p:+.4f}, A' {a2 - p:+.4f} ms/step ({100 * (a - p) / p:+.2f} %): "
                     f"{verdict} the A/A noise")
    else:
        lines.append("  (no --parent tree was given: the parent commit was not measured)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chamfer_time.txt"))
    ap.add_argument("--part", choices=("kernels", "steps", "all"), default="all")
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
    lines = ["Chamfer distance (loss term chamfer): time per call / per step (ms), median [min .. max]",
             "command: python tools/time_chamfer.py " + " ".join(argv),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    if cli.part in ("kernels", "all"):
        kernel_rows(cli, lines)
    if cli.part in ("steps", "all"):
        step_rows(cli, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "a" if cli.part == "steps" else "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
