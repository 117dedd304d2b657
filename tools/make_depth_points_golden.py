#!/usr/bin/env python3
"""Generate tests/golden/depth_points.npz by running the REFERENCE's own back-projection: lines 686-698 of utils/fh_utils.py, the part of
`batch_depth2pc` in front of its sampling loop (the valid pixels of a depth batch and their x, y, z).

    python tools/make_depth_points_golden.py --reference <checkout of the reference>      (or HIFIHR_REFERENCE)

Run it on a machine without a GPU; never part of a GPU test.  The statements are taken from the function's syntax tree by their line
numbers and compiled unmodified, the way tools/make_open2d_golden.py takes its functions; nothing of them is copied here.  The sampling
loop behind them (randint(0, n - 1): it never draws the last valid pixel) is not run: hifihr_depth_points draws uniformly over all of them.

The function's comment gives its depth argument as [b, width, height]: its dim 1 is the column u, its dim 2 the row v.  The seeded maps
here are [b, H, W] as this project keeps them and go in TRANSPOSED, so that uv_index = (sample, u, v).  The maps are square (the function
repeats the intrinsics over shape[1] x shape[1]).  Everything runs in float32, as there.
The file holds arrays only:
  depths [3,24,24]   the maps as this project keeps them ([b, row, column]; 0 = no measurement), Ks [3,3,3] upper-triangular, fx, fy >= 100
  uv_index [N,3]     (sample, u, v) of every valid pixel, in the function's order
  x_gt, y_gt, z_gt [N]"""
import argparse
import ast
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, LAST = 686, 698


def load_reference(reference):
    path = os.path.join(reference, "utils", "fh_utils.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "batch_depth2pc"][0]
    body = [s for s in fn.body if FIRST <= s.lineno and s.end_lineno <= LAST]
    names = ", ".join(("x_gt", "y_gt", "z_gt", "uv_index"))
    assigned = {t.id for s in body for t in getattr(s, "targets", []) if isinstance(t, ast.Name)}
    assert {"x_gt", "y_gt", "z_gt", "uv_index"} <= assigned, f"{path}:{FIRST}-{LAST} no longer assigns {names}"
    fn.body = body + ast.parse(f"return {names}").body
    ast.fix_missing_locations(fn)
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["batch_depth2pc"]


def case_inputs(seed=41, B=3, S=24):
    rng = np.random.default_rng(seed)
    depths = (0.25 + 0.7 * rng.random((B, S, S))).astype(np.float32)
    depths[rng.random((B, S, S)) < 0.45] = 0.0
    depths[2, :, : S // 2] = 0.0                                          # a sample whose left half is empty
    Ks = np.zeros((B, 3, 3), np.float32)
    Ks[:, 0, 0], Ks[:, 1, 1] = 100 + 400 * rng.random(B), 100 + 400 * rng.random(B)
    Ks[:, 0, 2], Ks[:, 1, 2], Ks[:, 2, 2] = S / 2 + 3 * rng.standard_normal(B), S / 2 + 3 * rng.standard_normal(B), 1
    return depths, Ks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HIFIHR_REFERENCE"), required="HIFIHR_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "depth_points.npz"))
    cli = ap.parse_args()
    fn = load_reference(cli.reference)
    depths, Ks = case_inputs()
    x, y, z, uv = fn(torch.from_numpy(np.ascontiguousarray(depths.transpose(0, 2, 1))), torch.from_numpy(Ks))
    assert x.dtype == torch.float32 and uv.shape[0] == int((depths > 0).sum())
    np.savez_compressed(cli.out, depths=depths, Ks=Ks, uv_index=uv.numpy().astype(np.int32), x_gt=x.numpy(), y_gt=y.numpy(), z_gt=z.numpy())
    print(f"wrote {cli.out}: {uv.shape[0]} valid pixels of {depths.size}")


if __name__ == "__main__":
    main()
