#!/usr/bin/env python3
"""Time the gradient guard (hifihr_grad_norm / hifihr_adam_step_guarded, FusedAdam(max_grad_norm=...)): the norm pass and its finish at
the flat size of the ResNet-18 model as bytes over time against the HBM peak, the guarded Adam launch beside the unguarded one, and the
captured BASELINE config-2 training step with the guard off and on, alternated in the same run.

    python tools/time_grad_guard.py [--out profiles/grad_guard_time.txt]

Kernel figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: HIP events around `--steps` replays of the captured step (hifihr_amd.traineval.GraphedTrainStep), the median of `--rounds`
windows, per step; the steps are timed alternately, and the spread of the windows is printed beside every median.  There is no pass
threshold: the file is the record."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

HBM_PEAK_TBS = 8.0          # MI355X HBM3E, specification


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


def build(cli, max_grad_norm):
    from hifihr_amd import options, synth
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import data_dic
    dev, B, tables = torch.device("cuda"), cli.batch, synthetic_mano_tables(0)
    args = options.baseline_config2_args(train_batch=B)
    torch.manual_seed(0)
    model = Model(True, dev, False, "mano", False, "res18", mano_tables=tables).to(dev).train()
    flat = FlatParams(model)
    opt = FusedAdam(flat, lr=1e-6, max_grad_norm=max_grad_norm)
    ex = data_dic(synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, device=dev), "FreiHand", "training", args, device=dev)
    return model, flat, opt, ex, args


def kernel_rows(cli, lines, n):
    from hifihr_amd._lib import get_lib
    lib = get_lib()
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    p, m, v = torch.randn(n, device="cuda", generator=gen), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    guard, ws = lib.grad_guard_alloc(n, "cuda")
    state = lib.adam_state_image(1e-6, 0.9, 0.999, 0).cuda()
    ring, turn = [g] + [g.clone() for _ in range(7)], [0]          # 8 gradient buffers in turn: more bytes than the Infinity Cache holds

    def norm_rotating():
        turn[0] = (turn[0] + 1) % len(ring)
        lib.grad_norm(ring[turn[0]], 1.0, float("inf"), guard, ws)
    rows = [("grad_norm (sum of squares + finish: two launches)", 4 * n, lambda: lib.grad_norm(g, 1.0, float("inf"), guard, ws)),
            ("grad_norm, 8 buffers in turn (past the Infinity Cache)", 4 * n, norm_rotating),
            ("adam_step_counted (unguarded)", 28 * n, lambda: lib.adam_step_counted(p, g, m, v, 1.0, 1e-8, 0.0, state)),
            ("adam_step_guarded, counted form (guard block read)", 28 * n,
             lambda: lib.adam_step_guarded(p, g, m, v, 1.0, 0.0, 0.0, 0.0, 1e-8, 0.0, 0, state, guard)),
            ("grad_norm + adam_step_guarded (what a guarded step launches)", 32 * n,
             lambda: (lib.grad_norm(g, 1.0, float("inf"), guard, ws),
                      lib.adam_step_guarded(p, g, m, v, 1.0, 0.0, 0.0, 0.0, 1e-8, 0.0, 0, state, guard)))]
    lines.append(f"launches at the flat size of the ResNet-18 model, n = {n} floats ({4 * n / 1e6:.1f} MB per buffer); back-to-back calls on one "
                 f"stream (one buffer fits the 256 MB Infinity Cache: the first row is the cached rate, the second the HBM rate)")
    lines.append(f"  {'':66s} {'ms':>9s}  {'[min .. max]':22s} {'bytes':>8s} {'TB/s':>6s} {'of 8 TB/s':>9s}")
    for name, nbytes, fn in rows:
        med, lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds)
        tbs = nbytes / (med * 1e-3) / 1e12
        lines.append(f"  MI355X  {name:58s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]   {nbytes / 1e6:6.1f}MB {tbs:6.2f} {100 * tbs / HBM_PEAK_TBS:8.1f}%")
    s = lib.grad_guard_unpack(guard.cpu().numpy().tobytes())
    lines.append(f"  (norm {s['norm']:.6e} against float64 {float(g.double().norm()):.6e}; finite {s['finite']}, coef {s['clip_coef']})")
    lines.append("")


def step_rows(cli, lines):
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.traineval import GraphedTrainStep
    torch.cuda.set_stream(torch.cuda.Stream())                                    # never the legacy default stream before a capture
    steps, opts, n = {}, {}, 0
    for tag, mgn in (("config 2, guard off", None), ("config 2, max_grad_norm = inf (skip alone)", float("inf")),
                     ("config 2, max_grad_norm = 1.0", 1.0)):
        model, flat, opt, ex, args = build(cli, mgn)
        steps[tag] = GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=3)
        opts[tag], n = opt, flat.numel
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
    lines.append(f"captured training step, ResNet-18 + MANO + render, B = {cli.batch}: ms/step, median [min .. max] of {cli.rounds} windows of "
                 f"{cli.steps} replays, the three steps alternated window by window")
    med = {}
    for tag, v in samples.items():
        med[tag] = statistics.median(v)
        lines.append(f"  MI355X  {tag:58s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    off = med["config 2, guard off"]
    spread = max(samples["config 2, guard off"]) - min(samples["config 2, guard off"])
    for tag in list(steps)[1:]:
        lines.append(f"  cost of {tag.split(', ')[1]}: {med[tag] - off:+.4f} ms/step ({100 * (med[tag] - off) / off:+.2f} %); "
                     f"spread of the guard-off windows: {spread:.4f} ms")
    for tag in list(steps)[1:]:
        lines.append(f"  counters after the run, {tag.split(', ')[1]}: {opts[tag].grad_stats()}")
    lines.append("")
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_guard_time.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    cli = ap.parse_args()
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    lines = ["gradient guard: time per call / per step (ms), median [min .. max]",
             "command: python tools/time_grad_guard.py " + " ".join(sys.argv[1:]),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    step_lines = []
    n = step_rows(cli, step_lines)
    kernel_rows(cli, lines, n)
    text = "\n".join(lines + step_lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
