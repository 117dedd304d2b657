#!/usr/bin/env python3
"""Time the HO-3D device-path extras on the GPU: HO3DDeviceCache.batch() as it was, with detections (hifihr_ho3d_keypoints), with depth
frames (hifihr_ho3d_depth_crop) and with both, at B = 32, 480 x 640 -> 224; and ops.depth_points at 224 x 224, P = 1000 beside the torch
form of the reference's routine (nonzero + a per-sample index_select loop) in the same run.

    python tools/time_ho3d_extras.py [--out profiles/ho3d_extras_time.txt] [--parent-tree DIR]

batch(): a host clock around `--repeats` calls that end in a device synchronise (the call holds host work: the crop windows in numpy and
one staged copy), the median of `--rounds` windows after `--warmup` calls, per call; the four caches are timed alternately and the plain
one TWICE: the difference of those two is the run's own A/A spread.  depth_points: HIP events around the same windows.
--parent-tree DIR: a checkout of the parent commit, built in place: `bench.py --gpus 1 --steps 60 --warmup 10` of this tree and of that
one alternately, three rounds, each in a child process of its own.  No pass threshold: the file is the record."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def host_ms(fn, repeats):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / repeats


def event_ms(fn, repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / repeats


def alternate(rows, clock, warmup, repeats, rounds):
    """rows: [(name, fn)] -> {name: (median, min, max)} with the rows timed in turn inside every round."""
    for _, fn in rows:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name, _ in rows}
    for _ in range(rounds):
        for name, fn in rows:
            got[name].append(clock(fn, repeats))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def frames(n, FH=480, FW=640, seed=0):
    """Random frames with a hand-sized spread of joints: the crop window, not the content, decides the work."""
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (n, FH, FW, 3)).astype(np.uint8)
    masks = (rng.random((n, FH, FW)) < 0.5).astype(np.uint8) * 255
    Ks = np.tile(np.asarray([[615.0, 0, 320.0], [0, 615.0, 240.0], [0, 0, 1.0]], np.float32), (n, 1, 1))
    xyz = np.concatenate([0.16 * rng.random((n, 21, 2)) - 0.08, 0.45 + 0.1 * rng.random((n, 21, 1))], -1).astype(np.float32)
    det = (rng.random((n, 21, 2)) * [FW, FH]).astype(np.float32)
    con = rng.random((n, 21, 1)).astype(np.float32)
    d16 = rng.integers(0, 65536, (n, FH, FW)).astype(np.uint16)
    return imgs, masks, Ks, xyz, det, con, d16


def reference_form(depths, Ks, P):
    """The reference's batch_depth2pc written with the same torch calls (nonzero, masked gathers, a per-sample index_select loop)."""
    B, S = depths.shape[0], depths.shape[1]
    uv = torch.nonzero(depths)
    z = depths[depths > 0]
    g = lambda i, j: Ks[:, i, j].view(-1, 1, 1).repeat(1, S, S)[depths > 0]
    x = ((uv[:, 1].float() - g(0, 2)) * z) * torch.reciprocal(g(0, 0) + 1e-5)
    y = ((uv[:, 2].float() - g(1, 2)) * z) * torch.reciprocal(g(1, 1) + 1e-5)
    xyz = torch.zeros(B, P, 3, device=depths.device)
    for i in range(B):
        index = torch.nonzero(uv[:, 0] == i).view(-1)
        if len(index) > 1:
            index = torch.index_select(index, 0, torch.randint(0, index.shape[0] - 1, (P,), device=index.device))
            xyz[i] = torch.stack([x[index], y[index], z[index]], 1)
    return xyz


def bench_value(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "60", "--warmup", "10"], cwd=tree, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"bench.py in {tree} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ho3d_extras_time.txt"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    cli = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU; there is no CPU figure"
    from hifihr_amd import ops
    from hifihr_amd.data import HO3DDeviceCache
    B, n, S, P = 32, 64, 224, 1000
    imgs, masks, Ks, xyz, det, con, d16 = frames(n)
    mk = lambda **kw: HO3DDeviceCache(imgs, masks, Ks, xyz, inp_res=S, **kw)
    caches = [("batch() as on the parent", mk()), ("batch() as on the parent, again (A/A)", mk()),
              ("+ detections", mk(open_2dj=det, open_2dj_con=con)), ("+ depth", mk(depth_u16=d16)),
              ("+ detections + depth", mk(open_2dj=det, open_2dj_con=con, depth_u16=d16))]
    idx = np.random.default_rng(1).permutation(n)[:B]
    noise = dict(center_noise=np.zeros((B, 2), np.float32), scale_noise=np.ones(B, np.float32))
    res = alternate([(name, (lambda c=c: c.batch(idx, **noise))) for name, c in caches], host_ms, cli.warmup, cli.repeats, cli.rounds)
    lines = [f"HO3DDeviceCache.batch(), B = {B}, {n} frames of 480 x 640 -> {S} x {S}; {torch.cuda.get_device_name(0)}",
             f"host clock around {cli.repeats} calls ending in a synchronise, median (min .. max) of {cli.rounds} alternated windows, ms per call"]
    for name, _ in caches:
        m, lo, hi = res[name]
        lines.append(f"  {name:42s} {m:8.4f}  ({lo:.4f} .. {hi:.4f})")
    base = res[caches[0][0]][0]
    lines.append(f"  A/A spread of the plain call: {abs(res[caches[1][0]][0] - base):.4f} ms; + detections {res[caches[2][0]][0] - base:+.4f}, "
                 f"+ depth {res[caches[3][0]][0] - base:+.4f}, + both {res[caches[4][0]][0] - base:+.4f} ms")
    # depth_points against the torch form of the reference's routine
    g = torch.Generator(device="cuda").manual_seed(0)
    depths = (0.3 + 0.5 * torch.rand(B, S, S, device="cuda", generator=g)) * (torch.rand(B, S, S, device="cuda", generator=g) < 0.35)
    Kd = torch.tensor([[500.0, 0, 112.0], [0, 500.0, 112.0], [0, 0, 1.0]], device="cuda").repeat(B, 1, 1)
    mask = (torch.rand(B, S, S, device="cuda", generator=g) < 0.8).float()
    draws = torch.rand(B, P, device="cuda", generator=g)
    rows = [("ops.depth_points (draws given)", lambda: ops.depth_points(depths, Kd, P, mask=mask, draws=draws)),
            ("ops.depth_points (draws given), again (A/A)", lambda: ops.depth_points(depths, Kd, P, mask=mask, draws=draws)),
            ("ops.depth_points (torch.rand inside)", lambda: ops.depth_points(depths, Kd, P, mask=mask)),
            ("torch form of the reference's routine", lambda: reference_form(depths * mask, Kd, P))]
    res = alternate(rows, event_ms, cli.warmup, max(cli.repeats // 4, 5), cli.rounds)
    lines += ["", f"depth_points, B = {B}, {S} x {S}, P = {P}, {int(((depths > 0) & (mask != 0)).sum()) // B} valid pixels per sample on average",
              f"HIP events around {max(cli.repeats // 4, 5)} calls, median (min .. max) of {cli.rounds} alternated windows, ms per call"]
    for name, _ in rows:
        m, lo, hi = res[name]
        lines.append(f"  {name:46s} {m:8.4f}  ({lo:.4f} .. {hi:.4f})")
    lines.append(f"  the reference's form takes {res[rows[3][0]][0] / res[rows[0][0]][0]:.1f} x the one launch (it reads counts back to the host once per sample)")
    if cli.parent_tree:
        vals = [(bench_value(REPO), bench_value(cli.parent_tree)) for _ in range(3)]
        here, there = [v[0] for v in vals], [v[1] for v in vals]
        lines += ["", "bench.py --gpus 1 --steps 60 --warmup 10, this tree and the parent commit's alternately, images/s:",
                  "  this tree: " + ", ".join(f"{v:.1f}" for v in here), "  parent   : " + ", ".join(f"{v:.1f}" for v in there),
                  f"  medians {statistics.median(here):.1f} against {statistics.median(there):.1f}; spread of this tree {max(here) - min(here):.1f}, "
                  f"of the parent {max(there) - min(there):.1f} (nothing in the default step calls the new entries)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(cli.out), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
