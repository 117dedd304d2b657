#!/usr/bin/env python3
"""Generate tests/golden/mano_fit.npz by running the REFERENCE's own tilt-swing-azimuth pose prior, `tsa_pose_loss` of
utils/losses_util.py:139-215, the one term of the keypoint fit (hifihr_mano_fit) that no other fixture pins.

    python tools/make_mano_fit_golden.py --reference <checkout of the reference>      (or HIFIHR_REFERENCE)

Run it on a machine without a GPU; never part of a GPU test.  The module cannot be imported whole (pytorch3d at module level): the function
is compiled from its source unmodified, the way tools/make_open2d_golden.py takes loss_func.  Nothing of it is copied here.

Inputs are seeded, B = 6, float32 (the function builds float32 tables): every one of the 48 components lies above its upper bound in some
sample, below its lower bound in another, inside in the rest, and exactly ON a bound in sample 5 (the strict comparisons give 0 there).
The file holds arrays only:
  tsaposes [6,16,3]        the inputs
  loss [1]                 tsa_pose_loss of the whole batch
  sample_loss [6]          tsa_pose_loss of each sample alone
  max_nonloss, min_nonloss [16,3]   the two bound tables the function builds (the values of its list literals), float32"""
import argparse
import ast
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(reference):
    path = os.path.join(reference, "utils", "losses_util.py")
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "tsa_pose_loss"][0]
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    tables = {}
    for stmt in node.body:                                    # the list literals of the two live assignments, evaluated as the function does
        if isinstance(stmt, ast.Assign) and stmt.targets[0].id in ("max_nonloss", "min_nonloss"):
            lit = [n for n in ast.walk(stmt.value) if isinstance(n, ast.List)][0]
            tables[stmt.targets[0].id] = np.asarray(eval(compile(ast.Expression(lit), path, "eval"), {"pi": np.pi}), dtype=np.float32)
    return ns["tsa_pose_loss"], tables["max_nonloss"], tables["min_nonloss"]


def case_inputs(hi, lo, seed=47, B=6):
    rng = np.random.default_rng(seed)
    mid, half = (hi + lo) / 2, (hi - lo) / 2
    x = np.empty((B, 16, 3), np.float32)
    side = np.stack([rng.permutation(B - 1) for _ in range(48)], 1).reshape(B - 1, 16, 3)       # per component: which sample is above / below
    for b in range(B - 1):
        inside = mid + half * rng.uniform(-0.9, 0.9, (16, 3))
        above = hi + rng.uniform(0.01, 0.5, (16, 3))
        below = lo - rng.uniform(0.01, 0.5, (16, 3))
        x[b] = np.where(side[b] == 0, above, np.where(side[b] == 1, below, inside))
    x[B - 1] = np.where(rng.random((16, 3)) < 0.5, hi, lo)                                      # exactly on a bound
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HIFIHR_REFERENCE"), required="HIFIHR_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "mano_fit.npz"))
    cli = ap.parse_args()
    tsa_pose_loss, hi, lo = load_reference(cli.reference)
    x = case_inputs(hi, lo)
    loss = np.array([float(tsa_pose_loss(torch.from_numpy(x)))], np.float32)
    sample = np.array([float(tsa_pose_loss(torch.from_numpy(x[b:b + 1]))) for b in range(x.shape[0])], np.float32)
    assert sample[-1] == 0.0 and (sample[:-1] > 0).all()
    np.savez_compressed(cli.out, tsaposes=x, loss=loss, sample_loss=sample, max_nonloss=hi, min_nonloss=lo)
    print("loss", loss.tolist(), "per sample", sample.tolist())
    print("wrote", cli.out, os.path.getsize(cli.out), "bytes")


if __name__ == "__main__":
    main()
