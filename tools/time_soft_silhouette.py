#!/usr/bin/env python3
"""Time the soft silhouette (hifihr_soft_sil_fwd / _bwd) at B = 32, H = 224 on the MANO topology beside the hard renderer's
hifihr_render_fwd / _bwd (aa = 3) in the same run, and the captured BASELINE config-2 training step with the terms "sil_soft" + "iou_soft"
added against the step without them.

    python tools/time_soft_silhouette.py [--out profiles/soft_silhouette_time.txt]

Kernel figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: HIP events around `--steps` replays of the captured step (hifihr_amd.traineval.GraphedTrainStep), the median of `--rounds`
windows, per step; the two steps are timed alternately.  There is no pass threshold: the file is the record."""
import argparse
import os
import statistics
import sys

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


def kernel_rows(cli, lines):
    import kernel_cases as kc
    from hifihr_amd import ops
    from hifihr_amd._lib import get_lib
    from hifihr_amd.mano_tables import synthetic_mano_tables
    lib, tables, B, H = get_lib(), synthetic_mano_tables(0), cli.batch, 224
    verts, vcol, cam, lc, ld = (t.cuda().contiguous() for t in kc.make_render_inputs(tables, B, 0, H))
    handle = ops.RendererHandle(tables.faces, 778, image_size=H, aa=3)
    sigma, blur = ops.SOFT_SIL_SIGMA, ops.soft_sil_default_blur(ops.SOFT_SIL_SIGMA)
    alpha, neglog = torch.empty(B, 1, H, H, device="cuda"), torch.empty(B, H, H, device="cuda")
    ws = torch.empty(lib.soft_sil_workspace_bytes(handle.h, B), dtype=torch.uint8, device="cuda")
    gverts = torch.empty_like(verts)
    lib.soft_sil_fwd(handle.h, verts, cam, sigma, blur, alpha, neglog, ws)
    mask = (torch.rand(B, H, H, device="cuda") > 0.5).float()
    galpha = ((alpha[:, 0] - mask).sign() / alpha.numel()).contiguous()           # what an L1 term against a mask sends back: dense
    rgba, face_id = torch.empty(B, 4, H, H, device="cuda"), torch.empty(B, 3 * H, 3 * H, dtype=torch.int32, device="cuda")
    rws = handle.workspace(B, "cuda")
    grgba = torch.randn(B, 4, H, H, device="cuda") / rgba.numel()
    gv, gc, gl = torch.empty_like(verts), torch.empty_like(verts), torch.empty(2, B, 3, device="cuda")
    lib.render_fwd(handle.h, verts, vcol, cam, lc, ld, rgba, face_id, rws)
    sums, out = torch.empty(B, 3, dtype=torch.float64, device="cuda"), torch.empty(2, device="cuda")
    gout, ga = torch.ones(2, device="cuda"), torch.empty_like(alpha)
    lib.soft_sil_loss_fwd(alpha, mask, 0.005, 1e-3, sums, out)
    rows = [("soft_sil_fwd   (vertex pass + tiles)", lambda: lib.soft_sil_fwd(handle.h, verts, cam, sigma, blur, alpha, neglog, ws)),
            ("soft_sil_bwd   (fill + vertex pass + tiles + projection)", lambda: lib.soft_sil_bwd(handle.h, verts, cam, neglog, galpha, sigma, blur, gverts, ws)),
            ("render_fwd     (aa = 3)", lambda: lib.render_fwd(handle.h, verts, vcol, cam, lc, ld, rgba, face_id, rws)),
            ("render_bwd", None),
            ("soft_sil_loss_fwd (sums + finish)", lambda: lib.soft_sil_loss_fwd(alpha, mask, 0.005, 1e-3, sums, out)),
            ("soft_sil_loss_bwd", lambda: lib.soft_sil_loss_bwd(alpha, mask, sums, gout, 0.005, 1e-3, ga))]
    cover = float((alpha > 0.5).float().mean())
    lines.append(f"kernels at B = {B}, H = {H}, MANO topology (778 vertices, 1538 faces), sigma = {sigma:g}, blur_radius = {blur:.4g}; "
                 f"{100 * cover:.1f} % of the pixels have alpha > 0.5")
    fwd_ms = None
    for name, fn in rows:
        if fn is None:
            # the renderer's backward consumes what its forward left in the workspace: time the pair and subtract the forward
            pair = lambda: (lib.render_fwd(handle.h, verts, vcol, cam, lc, ld, rgba, face_id, rws),
                            lib.render_bwd(handle.h, verts, cam, lc, ld, face_id, grgba, gv, gc, gl[0], gl[1], rws))
            med, lo, hi = gpu_ms(pair, cli.warmup, cli.repeats, cli.rounds)
            lines.append(f"  MI355X  {'render_fwd + render_bwd (aa = 3), the pair':58s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]")
            lines.append(f"  MI355X  {'render_bwd = median of the pair - median of render_fwd':58s} {med - fwd_ms:9.4f}")
            continue
        else:
            med, lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds)
            if name.startswith("render_fwd"):
                fwd_ms = med
        lines.append(f"  MI355X  {name:58s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]")
    lines.append("")


def step_rows(cli, lines):
    from hifihr_amd import options, synth
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, data_dic
    dev, B, tables = torch.device("cuda"), cli.batch, synthetic_mano_tables(0)
    torch.cuda.set_stream(torch.cuda.Stream())                                    # never the legacy default stream before a capture
    base = options.baseline_config2_args(train_batch=B)
    steps = {}
    for tag, soft in (("config 2 as it is", False), ("config 2 + sil_soft + iou_soft", True)):
        args = options.baseline_config2_args(train_batch=B, losses=base.losses + (["sil_soft", "iou_soft"] if soft else []))
        torch.manual_seed(0)
        model = Model(True, dev, False, "mano", False, "res18", mano_tables=tables, soft_silhouette=soft).to(dev).train()
        opt = FusedAdam(FlatParams(model), lr=1e-6)
        ex = data_dic(synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, device=dev), "FreiHand", "training", args, device=dev)
        steps[tag] = GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=3)
    samples = {tag: [] for tag in steps}
    for tag, g in steps.items():
        for _ in range(cli.warmup):
            g()
    torch.cuda.synchronize()
    for _ in range(cli.rounds):
        for tag, g in steps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(cli.steps):
                g()
            b.record()
            b.synchronize()
            samples[tag].append(a.elapsed_time(b) / cli.steps)
    lines.append(f"captured training step, ResNet-18 + MANO + render, B = {B}: ms/step, median [min .. max] of {cli.rounds} windows of {cli.steps} replays")
    med = {}
    for tag, v in samples.items():
        med[tag] = statistics.median(v)
        lines.append(f"  MI355X  {tag:58s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    a, b = med["config 2 as it is"], med["config 2 + sil_soft + iou_soft"]
    lines.append(f"  cost of the option with both terms: {b - a:+.4f} ms/step ({100 * (b - a) / a:+.2f} %)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "soft_silhouette_time.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    cli = ap.parse_args()
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    lines = ["soft silhouette: time per call / per step (ms), median [min .. max]",
             "command: python tools/time_soft_silhouette.py " + " ".join(sys.argv[1:]),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    kernel_rows(cli, lines)
    step_rows(cli, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
