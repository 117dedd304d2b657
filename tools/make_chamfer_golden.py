#!/usr/bin/env python3
"""Generate tests/golden/chamfer.npz by running the REFERENCE's own ChamferLoss (utils/losses_util.py:304-337).

    python tools/make_chamfer_golden.py --reference <checkout of the reference>      (or HIFIHR_REFERENCE)

Run it on a machine without a GPU (the class moves its index tensors to the GPU when one is visible); never part of a GPU test.
utils/losses_util.py imports pytorch3d at module level and cannot be imported whole: the ChamferLoss class is compiled from its source
unmodified, the way tools/make_benchmark_golden.py takes EvalUtil.  The class is defined in the reference and never wired (the import in
losses.py:7 is commented out).

One case: two seeded sets of fp32 values, x [3, 37, 3] (preds) and y [3, 53, 3] (gts), fed as float64 tensors.  The file holds arrays
only: the fp32 inputs and the reference's loss_1 [3] (mean over x of the squared distance to the nearest y) and loss_2 [3] (the same from
y to x)."""
import argparse
import ast
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_chamfer_loss(reference):
    path = os.path.join(reference, "utils", "losses_util.py")
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ChamferLoss"][0]
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["ChamferLoss"]


def case_inputs(seed=21):
    """Hand-sized point sets in metres, the second one shifted and of another size."""
    rng = np.random.default_rng(seed)
    x = (0.05 * rng.standard_normal((3, 37, 3))).astype(np.float32)
    y = (0.05 * rng.standard_normal((3, 53, 3)) + 0.01).astype(np.float32)
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HIFIHR_REFERENCE"), required="HIFIHR_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "chamfer.npz"))
    cli = ap.parse_args()
    x, y = case_inputs()
    loss_1, loss_2 = load_chamfer_loss(cli.reference)()(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(y.astype(np.float64)))
    assert loss_1.dtype == torch.float64 and loss_1.shape == (3,) and loss_2.shape == (3,)
    np.savez_compressed(cli.out, x=x, y=y, loss_1=loss_1.numpy(), loss_2=loss_2.numpy())
    print("loss_1", loss_1.tolist(), "loss_2", loss_2.tolist())
    print("wrote", cli.out, os.path.getsize(cli.out), "bytes")


if __name__ == "__main__":
    main()
