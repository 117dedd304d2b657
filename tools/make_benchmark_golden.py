#!/usr/bin/env python3
"""Generate tests/golden/benchmark_metrics.npz by running the REFERENCE's own EvalUtil (utils/fh_utils.py:719-815).

    python tools/make_benchmark_golden.py --reference <checkout of the reference>      (or HIFIHR_REFERENCE)

utils/fh_utils.py imports skimage at module level and cannot be imported whole: the EvalUtil class is compiled from its source
unmodified, the way tools/make_golden.py extracts definitions.  numpy >= 2.0 has no np.trapz: it is aliased to np.trapezoid, the same
function under its new name -- bookkeeping, no arithmetic of the reference is replaced.

Three cases, each fed as float64 tensors holding fp32 values and reduced by get_measures(0.0, 0.05, 100):
  joints  n = 64, K = 21         mesh  n = 6, K = 778         masked  n = 48, K = 21 with keypoint 5 hidden in every sample, others in some
The file holds arrays only: the fp32 inputs, the masks and the reference's mean, AUC, PCK curve and thresholds."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

CASES = (("joints", 64, 21, 11, False), ("mesh", 6, 778, 12, False), ("masked", 48, 21, 13, True))


def load_evalutil(reference):
    path = os.path.join(reference, "utils", "fh_utils.py")
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "EvalUtil"][0]
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    ns = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["EvalUtil"]


def case_inputs(n, K, seed, masked):
    """Hand-sized points in metres; errors of a centimetre or two, a few beyond the last threshold (0.05)."""
    rng = np.random.default_rng(seed)
    gt = (0.05 * rng.standard_normal((n, K, 3))).astype(np.float32)
    pred = (gt + 0.012 * rng.standard_normal((n, K, 3)) * rng.uniform(0.2, 2.5, (n, K, 1))).astype(np.float32)
    vis = np.ones((n, K), np.uint8)
    if masked:
        vis = (rng.uniform(size=(n, K)) > 0.3).astype(np.uint8)
        vis[:, 5] = 0
        vis[:, 0] = 1
    return pred, gt, vis


def main():
    import benchmark_ref as br
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HIFIHR_REFERENCE"), required="HIFIHR_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "benchmark_metrics.npz"))
    cli = ap.parse_args()
    EvalUtil = load_evalutil(cli.reference)
    out = {}
    for name, n, K, seed, masked in CASES:
        pred, gt, vis = case_inputs(n, K, seed, masked)
        ev = EvalUtil(num_kp=K)
        ev.feed(torch.from_numpy(gt.astype(np.float64)), torch.from_numpy(vis.astype(bool)), torch.from_numpy(pred.astype(np.float64)))
        mean, _median, auc, curve, thr = ev.get_measures(0.0, 0.05, 100)
        assert br.threshold_gap_ok(br.distances(pred, gt), thr), f"{name}: a distance sits on a threshold; take another seed"
        out.update({f"{name}_pred": pred, f"{name}_gt": gt, f"{name}_vis": vis, f"{name}_mean": np.float64(mean), f"{name}_auc": np.float64(auc),
                    f"{name}_curve": np.asarray(curve, np.float64), f"{name}_thresholds": np.asarray(thr, np.float64)})
        print(f"{name}: n {n} K {K} mean {mean:.6f} auc {auc:.6f}")
    np.savez_compressed(cli.out, **out)
    print("wrote", cli.out, os.path.getsize(cli.out), "bytes")


if __name__ == "__main__":
    main()
