#!/usr/bin/env python3
"""Time the point-to-mesh distance (hifihr_point_mesh_fwd / _bwd: the loss term "point_mesh") at (B, N, V, F) = (32, 778, 778, 1538), the
MANO topology, and at (48, 778, 5990, 11976), the NIMBLE-shaped skin against 778 target points, one-sided (points -> faces only, the
default of the loss term) and two-sided; the float64 torch restatement of the same definition (tests/point_mesh_ref.py point_mesh_torch) in
the same run at the largest batch that fits the device, labelled with that batch; the achieved fp64 rate of the search loop; and the
captured BASELINE config-2 training step with the term added against the step without it -- in this tree twice (the run's own A/A noise)
and, with --parent, in a checkout of the parent commit (built: its hifihr_amd/libhifihr.so exists) in the same run.

    python tools/time_point_mesh.py [--part kernels|steps|all] [--parent PATH] [--out profiles/point_mesh_time.txt]

Kernel figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: every step is captured and timed in a process of its own (the same script text in either tree, so both are measured the
same way), HIP events around `--steps` replays, the median of `--rounds` windows, per step; the processes run one after the other, the
whole sequence `--alternations` times, its order rotated each time; a child that fails ends the run.  `--part steps` appends to the file `--part kernels` wrote.
There is no pass threshold: the file is the record."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the chip's public fp64 VECTOR figure (AMD's MI355X product page [recalled]; NOT measured in this repository), counted as fused
# multiply-adds = 2 operations each.  The search loop is built without contraction: separate operations, no fma
PUBLIC_FP64_VECTOR_TFLOPS = 78.6
# per (point, face) pair, csrc/point_mesh.hip pair_d2: 3 (ap) + 10 (d1, d2) + 4 (d3 .. d6) + 9 (va, vb, vc) + 4 (e1, e2, e3a, e3b) + 3 (e3, den)
# + 1 division (one operation here; the device expands it to some tens of instructions) + 4 (1 - q, vb q, vc q, 1 - w1) + 12 (the residual)
# + 5 (d2); the compares and selects of the region chain are not counted
OPS_PER_PAIR = 55

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


def shapes():
    """(name, B, points [B, N, 3], verts [B, V, 3], faces [F, 3]) as CPU tensors: seeded millimetre noise round the layers' templates"""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.nimble_tables import synthetic_nimble_tables
    mano, nimble = synthetic_mano_tables(0), synthetic_nimble_tables(0)
    g = torch.Generator().manual_seed(0)
    out = []
    for name, B, t in (("MANO topology", 32, mano), ("NIMBLE-shaped skin", 48, nimble)):
        vt = torch.as_tensor(np.asarray(t.v_template, np.float32))
        verts = vt[None] * 1.02 + 0.002 * torch.randn(B, vt.shape[0], 3, generator=g)
        pick = torch.randperm(vt.shape[0], generator=g)[:778]
        points = vt[pick][None] + 0.003 * torch.randn(B, 778, 3, generator=g)
        out.append((name, B, points, verts, torch.as_tensor(np.asarray(t.faces, np.int32))))
    return out


def restatement_rows(cli, lines, points, verts, faces, w):
    """The float64 torch restatement on the device at the largest batch (B, B / 2, ...) that fits: forward under no_grad, and forward +
    backward to the vertices.  Not a ratio: another formulation in another precision path, reported for scale."""
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import point_mesh_ref as pr
    B = points.shape[0]
    while B >= 1:
        try:
            p, v = points[:B].double().cuda(), verts[:B].double().cuda()
            vg = v.clone().requires_grad_(True)

            def fwd():
                with torch.no_grad():
                    pr.point_mesh_torch(p, v, faces, *w)

            def fwd_bwd():
                vg.grad = None
                pr.point_mesh_torch(p, vg, faces, *w).backward()

            rows = [(f"float64 torch restatement, forward (no_grad), B = {B}", fwd), (f"float64 torch restatement, forward + backward to verts, B = {B}", fwd_bwd)]
            got = [(name, gpu_ms(fn, 1, max(1, cli.repeats // 10), 3)) for name, fn in rows]
            for name, (med, lo, hi) in got:
                lines.append(f"    MI355X  {name:66s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]")
            return
        except torch.cuda.OutOfMemoryError:
            p = v = vg = None
            torch.cuda.empty_cache()
            B //= 2
    lines.append("    the float64 torch restatement does not fit the device at any batch")


def kernel_rows(cli, lines):
    import torch
    sys.path.insert(0, REPO)
    from hifihr_amd import ops
    from hifihr_amd._lib import get_lib
    lib = get_lib()
    qp, tf, qf, tp = lib.point_mesh_geometry()
    lines.append(f"kernels: points -> faces {qp} points per workgroup ({qp // 64} per lane), {tf} face records per LDS pass; faces -> points {qf} faces "
                 f"per workgroup ({qf // 64} per lane), {tp} points per LDS pass; ms per call")
    for name, B, points, verts, faces in shapes():
        p, v, f = points.cuda(), verts.cuda(), faces.cuda()
        N, V, F = p.shape[1], v.shape[1], f.shape[0]
        f32, off, corner = ops.point_mesh_tables_of(f, V)
        dev = "cuda"
        idx_pf, idx_fp = torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, F, dtype=torch.int32, device=dev)
        bary_pf, bary_fp = torch.empty(B, N, 3, dtype=torch.float64, device=dev), torch.empty(B, F, 3, dtype=torch.float64, device=dev)
        min_pf, min_fp = torch.empty(B, N, dtype=torch.float64, device=dev), torch.empty(B, F, dtype=torch.float64, device=dev)
        sums, out, gout = torch.empty(B, 2, dtype=torch.float64, device=dev), torch.empty(1, device=dev), torch.ones(1, device=dev)
        ws = torch.empty(lib.point_mesh_workspace_bytes(B, N, V, F) // 8, dtype=torch.float64, device=dev)
        gp, gv = torch.empty_like(p), torch.empty_like(v)
        vg = v.clone().requires_grad_(True)
        lines.append(f"  {name}: (B, N, V, F) = ({B}, {N}, {V}, {F})")
        for side, w in (("one-sided (w_fp = 0)", (1.0, 0.0)), ("two-sided", (1.0, 1.0))):
            fwd = lambda: lib.point_mesh_fwd(p, v, f32, w[0], w[1], idx_pf, bary_pf, min_pf, idx_fp, bary_fp, min_fp, sums, out, ws)
            lib.point_mesh_fwd(p, v, f32, 1.0, 1.0, idx_pf, bary_pf, min_pf, idx_fp, bary_fp, min_fp, sums, out, ws)   # both directions' arrays are valid

            def autograd():
                vg.grad = None
                ops.point_mesh_distance(p, vg, f, *w).backward()

            rows = [(f"hifihr_point_mesh_fwd (search + finish), {side}", fwd),
                    (f"hifihr_point_mesh_bwd, gp and gv, {side}",
                     lambda: lib.point_mesh_bwd(p, v, f32, idx_pf, bary_pf, idx_fp, bary_fp, gout, off, corner, w[0], w[1], gp, gv, ws)),
                    (f"hifihr_point_mesh_bwd, gv alone, {side}",
                     lambda: lib.point_mesh_bwd(p, v, f32, idx_pf, bary_pf, idx_fp, bary_fp, gout, off, corner, w[0], w[1], None, gv, ws)),
                    (f"ops.point_mesh_distance forward + backward to verts, {side}", autograd)]
            med = {}
            for rname, fn in rows:
                med[rname], lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds)
                lines.append(f"    MI355X  {rname:66s} {med[rname]:9.4f}  [{lo:.4f} .. {hi:.4f}]")
            pairs = (2.0 if w[1] else 1.0) * B * N * F
            rate = pairs * OPS_PER_PAIR / (med[rows[0][0]] * 1e-3) / 1e12
            lines.append(f"    search loop: {pairs:.3e} pairs x {OPS_PER_PAIR} fp64 operations (a division counted as one) in the forward's time = {rate:.2f} "
                         f"Top/s fp64; the chip's public fp64 vector figure is {PUBLIC_FP64_VECTOR_TFLOPS} TFLOPS counted as fused multiply-adds, i.e. "
                         f"{PUBLIC_FP64_VECTOR_TFLOPS / 2:.1f} T instructions/s for a loop without fma (public figure, UNMEASURED in this repository): "
                         f"{100 * rate / (PUBLIC_FP64_VECTOR_TFLOPS / 2):.0f} % of it")
            restatement_rows(cli, lines, points, verts, f, w)
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
            ("this tree, config 2 + point_mesh (one-sided, the default)", REPO, ["point_mesh"])]
    if cli.parent:
        runs.insert(0, ("parent commit, config 2 as it is", os.path.abspath(cli.parent), []))
    samples = {tag: [] for tag, _, _ in runs}
    for k in range(cli.alternations):
        for tag, tree, extra in runs[k % len(runs):] + runs[:k % len(runs)]:      # rotated: no row always runs first (on the coolest chip)
            samples[tag] += step_ms(tree, cli, extra)
    lines.append(f"captured training step, ResNet-18 + MANO + render, B = {cli.batch}: ms/step, median [min .. max] of {cli.alternations} x {cli.rounds} "
                 f"windows of {cli.steps} replays, one process per measurement, the rows alternated and their order rotated")
    med = {}
    for tag, v in samples.items():
        med[tag] = statistics.median(v)
        lines.append(f"  MI355X  {tag:58s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    a, a2, c = med[runs[-3][0]], med[runs[-2][0]], med[runs[-1][0]]
    noise = abs(a - a2)
    aa = samples[runs[-3][0]] + samples[runs[-2][0]]
    lines.append(f"  A/A noise of this run: |A - A'| of the medians {noise:.4f} ms/step ({100 * noise / a:.2f} %); spread of all A and A' windows "
                 f"[{min(aa):.4f} .. {max(aa):.4f}] ({100 * (max(aa) - min(aa)) / a:.2f} %)")
    lines.append(f"  cost of the term: {c - a:+.4f} ms/step ({100 * (c - a) / a:+.2f} %)")
    if cli.parent:
        p = med[runs[0][0]]
        verdict = "within" if min(aa) <= p <= max(aa) else "OUTSIDE"
        lines.append(f"  this tree without the term against the parent commit: A {a - p:+.4f}, A' {a2 - p:+.4f} ms/step ({100 * (a - p) / p:+.2f} %): the "
                     f"parent's median is {verdict} the A/A spread")
    else:
        lines.append("  (no --parent tree was given: the parent commit was not measured)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "point_mesh_time.txt"))
    ap.add_argument("--part", choices=("kernels", "steps", "all"), default="all")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--child-timeout", type=int, default=240)
    cli = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    argv = [a if not (i > 0 and sys.argv[1:][i - 1] in ("--parent", "--out")) else "<path>" for i, a in enumerate(sys.argv[1:])]
    lines = ["Point-to-mesh distance (loss term point_mesh): time per call / per step (ms), median [min .. max]",
             "command: python tools/time_point_mesh.py " + " ".join(argv),
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
