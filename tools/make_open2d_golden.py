#!/usr/bin/env python3
"""Generate tests/golden/open2d.npz by running the REFERENCE's own code for the self-supervised keypoint terms: the deprecated `loss_func`
of losses.py (lines 45-63: open_2dj, open_2dj_de; 79-85: open_bone_direc) and `bone_direction_loss` of utils/losses_util.py:217-283.

    python tools/make_open2d_golden.py --reference <checkout of the reference>      (or HIFIHR_REFERENCE)

Run it on a machine without a GPU; never part of a GPU test.  Neither module can be imported whole (pytorch3d, the SSIM and perceptual
helpers at module level): the two functions are compiled from their source unmodified, the way tools/make_chamfer_golden.py takes
ChamferLoss.  Nothing of them is copied here.

Everything runs in float32: bone_direction_loss casts its matrices with .float() and cannot run in float64.  Inputs are seeded, B = 5.
The file holds arrays only:
  j2d, open_2dj [5,21,2], open_2dj_con [5,21,1]      the inputs
  terms [3]                                           open_2dj, open_bone_direc, open_2dj_de at unit weights, whole batch
  rho [5,21]                                          rho(d) per joint: loss_func on ONE sample with a one-hot confidence (its weight cancels)
  joint_addends [5,21]                                rho(d) (c w)^2, the addends of open_2dj before the batch-wide normalisation:
                                                      rho above times (c w)^2, the latter formed here in float32
  sample_open_2dj [5]                                 open_2dj of each sample alone
  bone_terms [5,20]                                   |vn - von|^2 per bone, before the confidence weighting: bone_direction_loss on ONE
                                                      sample with confidence 1 on the bone's two joints only, times 20
  sample_bone_direc [5]                               open_bone_direc of each sample alone, with its confidences"""
import argparse
import ast
import os
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYPOINT_WEIGHTS = np.array([2, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5], np.float32)
BONES = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12),
         (0, 13), (13, 14), (14, 15), (15, 16), (0, 17), (17, 18), (18, 19), (19, 20))


def _function(path, name, ns):
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name][0]
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def load_reference(reference):
    ns = {"torch": torch, "nn": torch.nn, "torch_f": torch.nn.functional}
    ns["bone_direction_loss"] = _function(os.path.join(reference, "utils", "losses_util.py"), "bone_direction_loss", dict(ns))
    return _function(os.path.join(reference, "losses.py"), "loss_func", ns)


def case_inputs(seed=31, B=5):
    """Detections around the image centre, predictions 0 .. 12 px away (both branches of rho), confidences in [0, 1] with a few zeros."""
    rng = np.random.default_rng(seed)
    det = (112 + 40 * rng.standard_normal((B, 21, 2))).astype(np.float32)
    j2d = (det + rng.uniform(0, 12, (B, 21, 1)) * rng.standard_normal((B, 21, 2)) / 1.5).astype(np.float32)
    con = rng.random((B, 21, 1)).astype(np.float32)
    con[rng.random((B, 21, 1)) < 0.1] = 0.0
    return j2d, det, con


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HIFIHR_REFERENCE"), required="HIFIHR_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "open2d.npz"))
    cli = ap.parse_args()
    loss_func = load_reference(cli.reference)
    args = types.SimpleNamespace(lambda_j2d=1.0, lambda_j2d_de=1.0, lambda_bone_direc=1.0)
    used = ["open_2dj", "open_2dj_de", "open_bone_direc"]
    j2d, det, con = case_inputs()
    t = torch.from_numpy

    def run(rows, c):
        ex = {"imgs": torch.zeros(1), "open_2dj": t(det[rows]), "open_2dj_con": t(np.ascontiguousarray(c))}
        d = loss_func(ex, {"j2d": t(j2d[rows])}, used, "FreiHand", args)
        assert all(d[k].dtype == torch.float32 for k in used)
        return [float(d[k]) for k in ("open_2dj", "open_bone_direc", "open_2dj_de")]

    B = j2d.shape[0]
    terms = np.array(run(slice(None), con), np.float32)
    rho = np.zeros((B, 21), np.float32)
    bone_terms = np.zeros((B, 20), np.float32)
    sample_open, sample_bone = np.zeros(B, np.float32), np.zeros(B, np.float32)
    for b in range(B):
        rows = slice(b, b + 1)
        sample_open[b], sample_bone[b], _ = run(rows, con[rows])
        for j in range(21):
            one = np.zeros((1, 21, 1), np.float32); one[0, j] = 1
            rho[b, j] = run(rows, one)[0]
        for k, (p, c) in enumerate(BONES):
            two = np.zeros((1, 21, 1), np.float32); two[0, p] = 1; two[0, c] = 1
            bone_terms[b, k] = np.float32(run(rows, two)[1]) * np.float32(20)
    cw2 = (con[..., 0] * KEYPOINT_WEIGHTS[None]) ** 2
    np.savez_compressed(cli.out, j2d=j2d, open_2dj=det, open_2dj_con=con, terms=terms, rho=rho, joint_addends=(rho * cw2).astype(np.float32),
                        sample_open_2dj=sample_open, bone_terms=bone_terms, sample_bone_direc=sample_bone)
    print("terms", terms.tolist())
    print("wrote", cli.out, os.path.getsize(cli.out), "bytes")


if __name__ == "__main__":
    main()
