#!/usr/bin/env python3
"""Time the depth map (hifihr_render_depth_fwd / _bwd) and its loss at B = 32, 224 x 224, aa = 3 on the MANO topology and on the
NIMBLE-shaped skin at B = 48, beside the hard renderer's hifihr_render_fwd / _bwd and a float32 torch restatement (gathers + autograd) of
the same definition in the same run; then the captured BASELINE config-2 training step with the term "depth" against the step without it.

    python tools/time_depth.py [--out profiles/depth_time.txt] [--parent-tree DIR]

Kernel figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: HIP events around `--steps` replays of the captured step (hifihr_amd.traineval.GraphedTrainStep), per step.  Three steps are
timed alternately: the step as it is TWICE (two models built the same way: their difference is the run's own A/A spread) and the step
with the option and the term.  --parent-tree DIR: a checkout of the parent commit, built in place; its step is timed by this file's
--step-only mode in a child process between two blocks of the windows above, so that drift over the run shows.  There is no pass
threshold: the file is the record."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
COPY_TBS = 6.29          # measured copy rate of the MI355X, TB/s (the microarchitecture guide's figure)


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


def face_tile_pairs(face_id, H, aa):
    """(face, 8 x 8-pixel tile) pairs with a covered sample: the backward issues at most 9 float atomics for each."""
    B, T = face_id.shape[0], (H + 7) // 8
    assert H % 8 == 0
    t = face_id.view(B, T, 8 * aa, T, 8 * aa).permute(0, 1, 3, 2, 4).reshape(B * T * T, -1)
    s, _ = t.sort(dim=1)
    new = torch.ones_like(s, dtype=torch.bool)
    new[:, 1:] = s[:, 1:] != s[:, :-1]
    return int((new & (s >= 0)).sum())


def kernel_rows(cli, lines, name, B, verts, vcol, cam, lc, ld, faces):
    import depth_ref as dr
    from hifihr_amd import ops
    from hifihr_amd._lib import get_lib
    lib, H, aa = get_lib(), 224, 3
    V, S = verts.shape[1], 224 * 3
    handle = ops.RendererHandle(faces, V, image_size=H, aa=aa)
    rgba, face_id = torch.empty(B, 4, H, H, device="cuda"), torch.empty(B, S, S, dtype=torch.int32, device="cuda")
    rws = handle.workspace(B, "cuda")
    lib.render_fwd(handle.h, verts, vcol, cam, lc, ld, rgba, face_id, rws)
    depth, hits = torch.empty(B, 1, H, H, device="cuda"), torch.empty(B, H, H, dtype=torch.int32, device="cuda")
    lib.render_depth_fwd(handle.h, verts, cam, face_id, depth, hits)
    target = (depth[:, 0] + 0.01 * torch.randn(B, H, H, device="cuda")) * (hits > 0)
    sums, out = torch.empty(B, 2, dtype=torch.float64, device="cuda"), torch.empty(1, device="cuda")
    gout, gdepth, gverts = torch.ones(1, device="cuda"), torch.empty_like(depth), torch.empty_like(verts)
    lib.depth_loss_fwd(depth, hits, target, None, 1.0, 0.0, sums, out)
    lib.depth_loss_bwd(depth, hits, target, None, sums, gout, 1.0, 0.0, gdepth)           # what the L1 term sends back: +-1 / count on the covered pixels
    ws = torch.empty(lib.render_depth_workspace_bytes(handle.h, B), dtype=torch.uint8, device="cuda")
    grgba = torch.randn(B, 4, H, H, device="cuda") / rgba.numel()
    gv, gc, gl = torch.empty_like(verts), torch.empty_like(verts), torch.empty(2, B, 3, device="cuda")
    covered = int((face_id >= 0).sum())
    pairs = face_tile_pairs(face_id, H, aa)
    lines.append(f"{name}: B = {B}, V = {V}, F = {len(faces)}, 224 x 224, aa = 3; {covered} of {face_id.numel()} samples covered "
                 f"({100.0 * covered / face_id.numel():.1f} %), {int((hits > 0).sum())} of {hits.numel()} pixels")
    lines.append(f"  backward: {pairs} (face, tile) pairs -> at most {9 * pairs} float atomics per call, against {9 * covered} with one per "
                 f"component and covered sample ({9.0 * covered / max(9 * pairs, 1):.1f} x fewer)")

    def torch_pair():
        v = verts.detach().clone().requires_grad_(True)
        d = dr.depth_torch(v, cam, faces, face_id, hits, H, aa, dtype=torch.float32)
        d.backward(gdepth[:, 0])
        return v.grad

    res = {}
    rows = [("render_depth_fwd", lambda: lib.render_depth_fwd(handle.h, verts, cam, face_id, depth, hits)),
            ("render_depth_bwd (fill + tiles + projection)", lambda: lib.render_depth_bwd(handle.h, verts, cam, face_id, gdepth, hits, gverts, ws)),
            ("depth_loss_fwd (sums + finish)", lambda: lib.depth_loss_fwd(depth, hits, target, None, 1.0, 0.0, sums, out)),
            ("depth_loss_bwd", lambda: lib.depth_loss_bwd(depth, hits, target, None, sums, gout, 1.0, 0.0, gdepth)),
            ("render_fwd (aa = 3)", lambda: lib.render_fwd(handle.h, verts, vcol, cam, lc, ld, rgba, face_id, rws)),
            # the renderer's backward consumes what its forward left in the workspace: time the pair and subtract the forward
            ("render_fwd + render_bwd, the pair", lambda: (lib.render_fwd(handle.h, verts, vcol, cam, lc, ld, rgba, face_id, rws),
                                                           lib.render_bwd(handle.h, verts, cam, lc, ld, face_id, grgba, gv, gc, gl[0], gl[1], rws))),
            ("float32 torch restatement, forward + backward", torch_pair)]
    for tag, fn in rows:
        heavy = tag.startswith("float32")
        med, lo, hi = gpu_ms(fn, 2 if heavy else cli.warmup, 3 if heavy else cli.repeats, 3 if heavy else cli.rounds)
        res[tag] = med
        lines.append(f"  MI355X  {tag:50s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]")
    rbwd = res["render_fwd + render_bwd, the pair"] - res["render_fwd (aa = 3)"]
    lines.append(f"  MI355X  {'render_bwd = the pair - render_fwd (medians)':50s} {rbwd:9.4f}")
    lines.append(f"  render_depth_bwd / render_bwd = {res['render_depth_bwd (fill + tiles + projection)'] / rbwd:.3f}; "
                 f"render_depth_fwd / render_fwd = {res['render_depth_fwd'] / res['render_fwd (aa = 3)']:.3f}; the kernels' forward + backward are "
                 f"{res['float32 torch restatement, forward + backward'] / (res['render_depth_fwd'] + res['render_depth_bwd (fill + tiles + projection)']):.0f} x "
                 "faster than the torch restatement")
    nbytes = face_id.numel() * 4 + depth.numel() * 4 + hits.numel() * 4
    rate = nbytes / (res["render_depth_fwd"] * 1e-3) / 1e12
    lines.append(f"  forward bytes (face_id read + depth and hits written): {nbytes / 1e6:.1f} MB -> {rate:.3f} TB/s, {100 * rate / COPY_TBS:.1f} % of the "
                 f"{COPY_TBS} TB/s copy rate (the vertex gathers of the covered samples are not counted)")
    # the same gradient from the float64 restatement: how far the kernel and the float32 restatement are from it at this size
    v64 = verts.double().requires_grad_(True)
    dr.depth_torch(v64, cam, faces, face_id, hits, H, aa).backward(gdepth[:, 0].double())
    ref = v64.grad
    scale = float(ref.abs().max())
    lib.render_depth_bwd(handle.h, verts, cam, face_id, gdepth, hits, gverts, ws)
    lines.append(f"  gverts against float64 autograd of the restatement, max-abs over max-abs-ref: kernel {float((gverts.double() - ref).abs().max()) / scale:.2e}, "
                 f"float32 torch restatement {float((torch_pair().double() - ref).abs().max()) / scale:.2e}")
    lines.append("")


def build_step(with_term, B):
    """A captured config-2 step.  The option-off form uses nothing that the parent commit lacks (--step-only runs there)."""
    from hifihr_amd import options, synth
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, data_dic
    dev, tables = torch.device("cuda"), synthetic_mano_tables(0)
    base = options.baseline_config2_args(train_batch=B)
    args = options.baseline_config2_args(train_batch=B, losses=base.losses + (["depth"] if with_term else []))
    kw = dict(render_depth=True) if with_term else {}
    torch.manual_seed(0)
    model = Model(True, dev, False, "mano", False, "res18", mano_tables=tables, **kw).to(dev).train()
    opt = FusedAdam(FlatParams(model), lr=1e-6)
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, device=dev, **(dict(depth=True) if with_term else {}))
    ex = data_dic(sample, "FreiHand", "training", args, device=dev)
    return GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=3)


def step_windows(steps, cli, samples):
    for _ in range(cli.rounds):
        for tag, g in steps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(cli.steps):
                g()
            b.record()
            b.synchronize()
            samples[tag].append(a.elapsed_time(b) / cli.steps)


def step_only(cli):
    """The option-off step alone, windows as one JSON line: what the child process of --parent-tree prints."""
    torch.cuda.set_stream(torch.cuda.Stream())
    steps = {"step": build_step(False, cli.batch)}
    for _ in range(cli.warmup):
        steps["step"]()
    torch.cuda.synchronize()
    samples = {"step": []}
    step_windows(steps, cli, samples)
    print("STEP_WINDOWS " + json.dumps(samples["step"]))


def step_rows(cli, lines):
    B = cli.batch
    torch.cuda.set_stream(torch.cuda.Stream())                                    # never the legacy default stream before a capture
    tags = ("config 2 as it is (A)", "config 2 as it is (B)", "config 2 + render_depth + depth")
    steps = {tags[0]: build_step(False, B), tags[1]: build_step(False, B), tags[2]: build_step(True, B)}
    for g in steps.values():
        for _ in range(cli.warmup):
            g()
    torch.cuda.synchronize()
    samples = {t: [] for t in steps}
    step_windows(steps, cli, samples)
    parent = None
    if cli.parent_tree:
        tree = os.path.abspath(cli.parent_tree)
        cmd = [sys.executable, os.path.join(tree, "tools", os.path.basename(__file__)), "--step-only", "--batch", str(B), "--warmup",
               str(cli.warmup), "--rounds", str(2 * cli.rounds), "--steps", str(cli.steps)]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("STEP_WINDOWS ")]
        if r.returncode != 0 or not got:
            lines.append(f"  the parent tree's step could not be timed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:] or r.stdout[-200:]}")
        else:
            parent = json.loads(got[0][len("STEP_WINDOWS "):])
        step_windows(steps, cli, samples)                                         # a second block behind the child: drift over the run shows
    lines.append(f"captured training step, ResNet-18 + MANO + render, B = {B}: ms/step, median [min .. max] of {len(samples[tags[0]])} windows of "
                 f"{cli.steps} replays" + (" (two blocks, the parent's child process between them)" if cli.parent_tree else ""))
    med = {}
    for tag, v in samples.items():
        med[tag] = statistics.median(v)
        lines.append(f"  MI355X  {tag:50s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    if parent is not None:
        med["parent"] = statistics.median(parent)
        lines.append(f"  MI355X  {'the parent commit, config 2 as it is (child)':50s} {med['parent']:9.4f}  [{min(parent):.4f} .. {max(parent):.4f}]")
    a, a2, b = (med[t] for t in tags)
    lines.append(f"  A/A spread (two builds of the same step): {a2 - a:+.4f} ms/step ({100 * (a2 - a) / a:+.2f} %)")
    if parent is not None:
        lines.append(f"  option off against the parent: {0.5 * (a + a2) - med['parent']:+.4f} ms/step ({100 * (0.5 * (a + a2) - med['parent']) / med['parent']:+.2f} %)")
    lines.append(f"  cost of the option with the term: {b - 0.5 * (a + a2):+.4f} ms/step ({100 * (b - 0.5 * (a + a2)) / (0.5 * (a + a2)):+.2f} %)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_time.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, built in place: its config-2 step is timed in a child process")
    ap.add_argument("--step-only", action="store_true", help="time the option-off step alone and print its windows as JSON (what --parent-tree runs)")
    ap.add_argument("--skip-kernels", action="store_true")
    cli = ap.parse_args()
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    if cli.step_only:
        return step_only(cli)
    import kernel_cases as kc
    from hifihr_amd.mano_tables import synthetic_mano_tables
    lines = ["depth map: time per call / per step (ms), median [min .. max]",
             f"command: python tools/time_depth.py --batch {cli.batch} --warmup {cli.warmup} --repeats {cli.repeats} --rounds {cli.rounds} "
             f"--steps {cli.steps}" + (" --parent-tree DIR" if cli.parent_tree else ""),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    if not cli.skip_kernels:
        tables = synthetic_mano_tables(0)
        verts, vcol, cam, lc, ld = (t.cuda().contiguous() for t in kc.make_render_inputs(tables, 32, 0, 224))
        kernel_rows(cli, lines, "MANO topology", 32, verts, vcol, cam, lc, ld, tables.faces)
        B = 48
        mv, faces = kc.nimble_sized_mesh(B, 0)
        placed, _, cam, lc, ld = kc.make_render_inputs(tables, B, 0, 224)
        verts = (mv + placed.mean(1, keepdim=True)).cuda().contiguous()                   # the same placements in front of the camera
        vcol = (0.3 + 0.6 * torch.rand(B, mv.shape[1], 3, generator=torch.Generator().manual_seed(5))).cuda()
        kernel_rows(cli, lines, "NIMBLE-shaped skin", B, verts, vcol, cam.cuda().contiguous(), lc.cuda().contiguous(), ld.cuda().contiguous(), faces)
    step_rows(cli, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
