#!/usr/bin/env python3
"""Time the self-supervised keypoint terms: the kernel pair hifihr_open2d_terms_fwd / _bwd and the keypoint launch
hifihr_freihand_keypoints at B = 32, beside the same terms as float32 torch ops (tests/open2d_ref.py, forward + autograd) in the same run;
then the captured BASELINE config-2 training step with the terms open_2dj + open_bone_direc against the step without them.

    python tools/time_open2d.py [--out profiles/open2d_time.txt] [--parent-tree DIR] [--bench-rounds N]

Kernel figures: HIP events around `--repeats` back-to-back calls after `--warmup` calls, the median of `--rounds` such windows, per call.
Step figures: HIP events around `--steps` replays of the captured step (hifihr_amd.traineval.GraphedTrainStep), per step.  Three steps are
timed alternately: the step as it is TWICE (two models built the same way: their difference is the run's own A/A spread) and the step
with the two terms.  --parent-tree DIR: a checkout of the parent commit, built in place; its step is timed by this file's --step-only
mode in a child process (which imports the package from DIR) between two blocks of the windows above, so that drift over the run shows;
--bench-rounds N then also alternates `bench.py --gpus 1` of this tree and of DIR N times.  There is no pass threshold: the file is the
record."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    import open2d_cases as oc
    import open2d_ref as ref
    from hifihr_amd._lib import get_lib
    from hifihr_amd.data import batch_affine_terms
    lib, B = get_lib(), cli.batch
    j2d, det, con, lam, gout = oc.term_inputs(B, "random", True)
    j, d, c = j2d.cuda(), det.cuda(), con.cuda()
    go, out, g = torch.tensor(gout, device="cuda"), torch.empty(3, device="cuda"), torch.empty(B, 21, 2, device="cuda")

    def torch_pair():
        jj = j.detach().clone().requires_grad_(True)
        o = ref.terms(jj, d, c, lam, zero_weight_is_zero=False)
        (o * go).sum().backward()
        return jj.grad

    cache_det, cache_con = oc.keypoint_cache()
    cd, cc = cache_det.cuda(), cache_con.cuda()
    gen = torch.Generator().manual_seed(0)
    idx = torch.randint(0, oc.CACHE_N, (B,), generator=gen)
    rots = ((2 * torch.rand(B, generator=gen, dtype=torch.float64) - 1) * 3.141592653589793).numpy()
    total = torch.from_numpy(batch_affine_terms([112, 112], 224, [224, 224], rots, with_total=True)[3]).cuda()
    idx_d, gt = idx.int().cuda(), (224 * torch.rand(B, 21, 2, generator=gen)).cuda()
    od, oc_, ot = torch.empty(B, 21, 2, device="cuda"), torch.empty(B, 21, 1, device="cuda"), torch.empty(B, device="cuda")
    il = idx.cuda()

    def torch_keypoints():
        w = ref.warp(cd[il], total)
        cb = cc[il]
        c2 = cb.reshape(B, 21)
        gate = (c2.min(1)[0] > 0.1).float().unsqueeze(1)
        tex = torch.mean(gate * c2, 1) * ((il < ref.TRAIN_SIZE).float() + 0.1)
        pick = (il % ref.TRAIN_SIZE) < ref.TRAIN_SIZE * 0.5
        return torch.where(pick.view(-1, 1, 1), gt, w), torch.where(pick.view(-1, 1, 1), torch.ones_like(cb), cb), tex

    lines.append(f"kernels at B = {B} (21 joints, 20 bones per sample)")
    rows = [("open2d_terms_fwd", lambda: lib.open2d_terms_fwd(j, d, c, lam, out)),
            ("open2d_terms_bwd", lambda: lib.open2d_terms_bwd(j, d, c, lam, go, g)),
            ("the same terms as float32 torch ops, forward + backward", torch_pair),
            ("freihand_keypoints (semi_ratio 0.5)", lambda: lib.freihand_keypoints(cd, cc, idx_d, total, gt, 16280, od, oc_, ot)),
            ("the same as float32 torch ops", torch_keypoints)]
    res = {}
    for tag, fn in rows:
        med, lo, hi = gpu_ms(fn, cli.warmup, cli.repeats, cli.rounds)
        res[tag] = med
        lines.append(f"  MI355X  {tag:58s} {med:9.4f}  [{lo:.4f} .. {hi:.4f}]")
    pair = res["open2d_terms_fwd"] + res["open2d_terms_bwd"]
    lines.append(f"  the kernel pair is {res['the same terms as float32 torch ops, forward + backward'] / pair:.0f} x faster than the torch ops; the keypoint launch "
                 f"{res['the same as float32 torch ops'] / res['freihand_keypoints (semi_ratio 0.5)']:.0f} x (eager launches: these are launch-bound sizes)")
    lines.append("")


def build_step(with_terms, B):
    """A captured config-2 step.  The terms-off form uses nothing that the parent commit lacks (--step-only runs there)."""
    from hifihr_amd import options, synth
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, data_dic
    dev, tables = torch.device("cuda"), synthetic_mano_tables(0)
    base = options.baseline_config2_args(train_batch=B)
    args = options.baseline_config2_args(train_batch=B, losses=base.losses + (["open_2dj", "open_bone_direc"] if with_terms else []))
    torch.manual_seed(0)
    model = Model(True, dev, False, "mano", False, "res18", mano_tables=tables).to(dev).train()
    opt = FusedAdam(FlatParams(model), lr=1e-6)
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, device=dev, **(dict(open_2dj=True) if with_terms else {}))
    ex = data_dic(sample, "FreiHand", "training", args, device=dev)
    if with_terms:
        ex.pop("texture_con")          # the `*_self` photometric terms switch on with this key; they are not what is timed here
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
    """The terms-off step alone, windows as one JSON line: what the child process of --parent-tree prints."""
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
    tags = ("config 2 as it is (A)", "config 2 as it is (B)", "config 2 + open_2dj + open_bone_direc")
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
        cmd = [sys.executable, os.path.abspath(__file__), "--step-only", "--import-from", tree, "--batch", str(B), "--warmup", str(cli.warmup),
               "--rounds", str(2 * cli.rounds), "--steps", str(cli.steps)]
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
        lines.append(f"  MI355X  {tag:58s} {med[tag]:9.4f}  [{min(v):.4f} .. {max(v):.4f}]")
    if parent is not None:
        med["parent"] = statistics.median(parent)
        lines.append(f"  MI355X  {'the parent commit, config 2 as it is (child)':58s} {med['parent']:9.4f}  [{min(parent):.4f} .. {max(parent):.4f}]")
    a, a2, b = (med[t] for t in tags)
    lines.append(f"  A/A spread (two builds of the same step): {a2 - a:+.4f} ms/step ({100 * (a2 - a) / a:+.2f} %)")
    if parent is not None:
        lines.append(f"  terms off against the parent: {0.5 * (a + a2) - med['parent']:+.4f} ms/step ({100 * (0.5 * (a + a2) - med['parent']) / med['parent']:+.2f} %)")
    lines.append(f"  cost of the two terms: {b - 0.5 * (a + a2):+.4f} ms/step ({100 * (b - 0.5 * (a + a2)) / (0.5 * (a + a2)):+.2f} %)")
    lines.append("")


def bench_rows(cli, lines):
    """bench.py of this tree and of the parent's, alternated: the headline figure of each run."""
    tree = os.path.abspath(cli.parent_tree)
    got = {"this tree": [], "the parent commit": []}
    for _ in range(cli.bench_rounds):
        for tag, root in (("this tree", REPO), ("the parent commit", tree)):
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(cli.bench_steps), "--warmup", "10"],
                               cwd=root, capture_output=True, text=True, timeout=900)
            rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not rows:
                lines.append(f"  bench.py of {tag} failed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:]}")
                continue
            res = json.loads(rows[-1])
            got[tag].append(res.get("value", res.get("images_per_sec")))
    lines.append(f"bench.py --gpus 1 --steps {cli.bench_steps} --warmup 10, alternated {cli.bench_rounds} times: the headline of each run")
    for tag, v in got.items():
        lines.append(f"  MI355X  {tag:58s} " + "  ".join(f"{x:.1f}" if isinstance(x, (int, float)) else str(x) for x in v))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "open2d_time.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, built in place: its config-2 step is timed in a child process")
    ap.add_argument("--bench-rounds", type=int, default=0, help="with --parent-tree: alternate bench.py of both trees this many times")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--step-only", action="store_true", help="time the terms-off step alone and print its windows as JSON (what --parent-tree runs)")
    ap.add_argument("--import-from", default=REPO, help="the tree the package is imported from (--step-only of a parent tree)")
    ap.add_argument("--skip-kernels", action="store_true")
    cli = ap.parse_args()
    sys.path.insert(0, os.path.abspath(cli.import_from))
    sys.path.insert(0, os.path.join(REPO, "tests"))
    assert torch.cuda.is_available(), "the timings are GPU timings: no device, no figure"
    if cli.step_only:
        return step_only(cli)
    lines = ["self-supervised keypoint terms: time per call / per step (ms), median [min .. max]",
             f"command: python tools/time_open2d.py --batch {cli.batch} --warmup {cli.warmup} --repeats {cli.repeats} --rounds {cli.rounds} "
             f"--steps {cli.steps}" + (f" --parent-tree DIR --bench-rounds {cli.bench_rounds}" if cli.parent_tree else ""),
             f"device: {torch.cuda.get_device_name(0)}; warm-up {cli.warmup}, {cli.repeats} calls per window, {cli.rounds} windows", ""]
    if not cli.skip_kernels:
        kernel_rows(cli, lines)
    step_rows(cli, lines)
    if cli.parent_tree and cli.bench_rounds > 0:
        bench_rows(cli, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
