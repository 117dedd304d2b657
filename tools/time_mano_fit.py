#!/usr/bin/env python3
"""Time the one-launch keypoint fit (ops.mano_fit, csrc/mano_fit.hip) beside the same kind of fit composed from the project's existing ops.

    python tools/time_mano_fit.py [--out profiles/mano_fit_time.txt]          (on the MI355X)

Per batch size B = 1, 32, 128 with iters = 151:
  one launch   ops.mano_fit: 151 iterations inside one kernel
  composed     ONE iteration captured as a graph and replayed 151 times: ops.mano_full (two launches) -> root offset and proj_func in
               torch -> ops.open2d_terms (2-D and bone-direction terms) -> the TSA prior, shape and coefficient priors in torch -> autograd
               (mano_full's one-launch backward, open2d_terms' backward, torch's) -> torch.optim.Adam(capturable=True), four parameter groups
The composed objective differs in one respect that does not change its launches: ops.open2d_terms normalises the 2-D term over the whole
batch, the kernel per hand.  Times are the median [min .. max] of WINDOWS windows of CALLS fits each, from device events; inputs are the
seeded hands of tests/mano_fit_cases.py."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

ITERS, WARMUP, CALLS, WINDOWS = 151, 2, 5, 5
WEIGHTS = (1.0, 1.0, 0.0, 0.1, 0.1, 0.01)
LR_MULT = (1.0, 1.0, 1.0, 0.1)


def timed(fn):
    """ms per call: median, min, max over WINDOWS windows of CALLS calls."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / CALLS)
    return statistics.median(per), min(per), max(per)


def composed_fit(handle, case, dev, prior):
    """-> a callable that runs ITERS replays of one captured iteration (the parameters are reset first, outside the timing's interest)."""
    from hifihr_amd import ops
    from hifihr_amd.traineval import proj_func
    f = lambda k: case[k].to(dev)
    start = [f("pose")[:, :3].clone(), f("pose")[:, 3:].clone(), f("beta").clone(), f("root").clone()]
    par = [t.clone().requires_grad_(True) for t in start]
    K, kp, conf = f("K"), f("kp2d"), f("conf")
    lo, hi, w = (t.view(1, 48) for t in prior)
    comps = torch.as_tensor(case["tables"].hands_components, dtype=torch.float32, device=dev)
    mean = torch.as_tensor(case["tables"].hands_mean, dtype=torch.float32, device=dev).view(1, 45)
    opt = torch.optim.Adam([dict(params=[p], lr=0.01 * m) for p, m in zip(par, LR_MULT)], capturable=True)

    def iteration():
        opt.zero_grad(set_to_none=True)
        pose = torch.cat([par[0], par[1]], 1)
        joints = ops.mano_full(handle, pose, par[2], 9, None)[0]
        uv = proj_func(joints + par[3].unsqueeze(1), K)
        t2 = ops.open2d_terms(uv, kp, conf, (WEIGHTS[0], WEIGHTS[1], 0.0))
        fp = torch.cat([par[0], mean + par[1] @ comps], 1)
        prior_e = ((torch.relu(fp - hi) + torch.relu(lo - fp)) * w).sum() / (48.0 * fp.shape[0])
        loss = t2[0] + t2[1] + WEIGHTS[3] * prior_e + WEIGHTS[4] * (par[2] ** 2).mean() + WEIGHTS[5] * (par[1] ** 2).mean()
        loss.backward()
        opt.step()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            iteration()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        iteration()

    def run():
        with torch.no_grad():
            for p, s in zip(par, start):
                p.copy_(s)
        for _ in range(ITERS):
            graph.replay()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mano_fit_time.txt"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 32, 128])
    cli = ap.parse_args()
    import mano_fit_cases as fc
    from hifihr_amd import fit, ops
    from hifihr_amd.mano_tables import synthetic_mano_tables
    dev = torch.device("cuda", 0)
    tables = synthetic_mano_tables(0)
    handle = ops.ManoLayerHandle(tables)
    prior = fit.tsa_tables(dev)
    lines = [f"keypoint fit, {ITERS} iterations: ms per fit, median [min .. max] of {WINDOWS} windows of {CALLS} fits",
             "command: python tools/time_mano_fit.py",
             f"device: {torch.cuda.get_device_name(0)}; weights {WEIGHTS}, lr_mult {LR_MULT}, TSA prior on, no 3-D term", ""]
    for B in cli.sizes:
        case = fc.build_case(tables, f"time-b{B}", B, 900 + B, False, True, 9)
        f = lambda k: case[k].to(dev)
        args = (handle, f("pose"), f("beta"), f("root"), f("K"), f("kp2d"), f("conf"))
        one = lambda: ops.mano_fit(*args, iters=ITERS, weights=WEIGHTS, lr_mult=LR_MULT, prior=prior)
        res = one()
        torch.cuda.synchronize()
        t_one = timed(one)
        t_cmp = timed(composed_fit(handle, case, dev, prior))          # (an error here ends the script: nothing more is launched)
        lines.append(f"B = {B:3d}   one launch  {t_one[0]:9.3f}  [{t_one[1]:.3f} .. {t_one[2]:.3f}]   ({1e3 * t_one[0] / ITERS:.1f} us per iteration; "
                     f"E {float(res[3][:, 0, 0].mean()):.3f} -> {float(res[3][:, -1, 0].mean()):.3f}, done {int(res[4].min())})")
        lines.append(f"B = {B:3d}   composed    {t_cmp[0]:9.3f}  [{t_cmp[1]:.3f} .. {t_cmp[2]:.3f}]   ({1e3 * t_cmp[0] / ITERS:.1f} us per replayed iteration)")
        lines.append(f"B = {B:3d}   composed / one launch = {t_cmp[0] / t_one[0]:.2f}")
        lines.append("")
        print("\n".join(lines[-4:]), flush=True)
    text = "\n".join(lines)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")
    print("wrote", cli.out)


if __name__ == "__main__":
    main()
