"""Test-time refinement of a MANO prediction against 2-D (and optionally 3-D) keypoints: the reference's `mano_fitting`
(utils/traineval_util.py:505-595) on the live layer's parametrisation, run as ONE launch (ops.mano_fit; csrc/mano_fit.hip).

`fit_keypoints` is the entry the evaluation loops use (options `fit_keypoints`, `fit_iters`, `fit_target` and the six `fit_w_*` weights).
The tilt-swing-azimuth pose prior (`tsa_pose_loss`, utils/losses_util.py:139-215) exists only here: it is not a training term."""
from __future__ import annotations

import numpy as np
import torch

_D = np.pi / 180.0
# The live tables of tsa_pose_loss, [16][3]: the root, then index, middle, pinky, ring, thumb (three joints each), axis-angle components.
TSA_HI = np.array([[3.15, 0.01, 0.01],
                   [5 * _D, 10 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D],
                   [5 * _D, 10 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D],
                   [5 * _D, 20 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D],
                   [5 * _D, 10 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D], [5 * _D, 5 * _D, 100 * _D],
                   [90 * _D, 3 * np.pi / 16, np.pi / 8], [5 * _D, 5 * _D, np.pi / 8], [5 * _D, 5 * _D, 100 * _D]], dtype=np.float32)
TSA_LO = np.array([[3.13, -0.01, -0.01],
                   [-5 * _D, -10 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D],
                   [-5 * _D, -10 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D],
                   [-20 * _D, -10 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D],
                   [-5 * _D, -10 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D], [-5 * _D, -5 * _D, -10 * _D],
                   [0.0, -np.pi / 8, -np.pi / 8], [-5 * _D, -5 * _D, -np.pi / 8], [-5 * _D, -5 * _D, -20 * _D]], dtype=np.float32)
# the reference's [1, 1, 2] per axis; the root row's weight is 0: its bounds encode the legacy root convention (about pi around x),
# which is not the live model's
TSA_W = np.tile(np.array([1.0, 1.0, 2.0], dtype=np.float32), (16, 1))
TSA_W[0] = 0.0

FIT_WEIGHT_OPTIONS = ("fit_w_2d", "fit_w_bone", "fit_w_3d", "fit_w_prior", "fit_w_shape", "fit_w_pca")
FIT_WEIGHT_DEFAULTS = (1.0, 1.0, 0.0, 1.0, 0.1, 0.01)


_TSA_ON = {}


def tsa_tables(device):
    """(lo, hi, w) [48] float32 on `device`, built once per device."""
    key = str(device)
    if key not in _TSA_ON:
        _TSA_ON[key] = tuple(torch.as_tensor(t.reshape(48), device=device) for t in (TSA_LO, TSA_HI, TSA_W))
    return _TSA_ON[key]


def root_from_keypoints(joints_rel, kp2d, conf, K):
    """The translation t [B,3] that best reprojects a root-relative skeleton onto 2-D keypoints, confidence-weighted least squares.
    With X = J + t and K = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] the residuals of joint j are linear in t:
        (k0 - u_j k2) . (J_j + t) = 0,   (k1 - v_j k2) . (J_j + t) = 0        (k_i the rows of K),
    weighted by c_j^2.  The 3 x 3 normal equations are solved in closed form (adjugate / determinant) in plain torch ops.
    joints_rel [B,21,3], kp2d [B,21,2], conf [B,21] or [B,21,1], K [B,3,3]."""
    B = joints_rel.shape[0]
    c2 = conf.reshape(B, -1, 1).to(joints_rel.dtype) ** 2
    k0, k1, k2 = K[:, 0:1], K[:, 1:2], K[:, 2:3]                                    # [B,1,3]
    rows = torch.cat([k0 - kp2d[:, :, 0:1] * k2, k1 - kp2d[:, :, 1:2] * k2], 1)     # [B,42,3]
    w = torch.cat([c2, c2], 1)                                                      # [B,42,1]
    rhs = -(rows * torch.cat([joints_rel, joints_rel], 1)).sum(2, keepdim=True)     # [B,42,1]
    A = (rows.unsqueeze(3) * rows.unsqueeze(2) * w.unsqueeze(3)).sum(1)             # [B,3,3]
    b = (rows * w * rhs).sum(1)                                                     # [B,3]
    a00, a01, a02, a11, a12, a22 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    adj = torch.stack([torch.stack([c00, c01, c02], 1), torch.stack([c01, c11, c12], 1), torch.stack([c02, c12, c22], 1)], 1)
    return (adj * b.unsqueeze(1)).sum(2) / det.unsqueeze(1)


def fit_options(args):
    """-> dict(iters, target, weights) from the options (defaults where `args` does not carry them)."""
    weights = tuple(float(getattr(args, n, d)) for n, d in zip(FIT_WEIGHT_OPTIONS, FIT_WEIGHT_DEFAULTS))
    return dict(iters=int(getattr(args, "fit_iters", 151)), target=getattr(args, "fit_target", "open_2dj"), weights=weights)


def fit_target_of(examples, target):
    """-> (kp2d, conf) of the batch for `fit_target`, or None when the batch does not carry it."""
    if target == "open_2dj":
        if "open_2dj" in examples and "open_2dj_con" in examples:
            return examples["open_2dj"], examples["open_2dj_con"]
        return None
    if target == "j2d_gt":
        if "j2d_gt" in examples:
            return examples["j2d_gt"], torch.ones(examples["j2d_gt"].shape[:2], device=examples["j2d_gt"].device)
        return None
    raise ValueError(f"fit_target must be 'open_2dj' or 'j2d_gt', got {target!r}")


def fit_keypoints(model, outputs, kp2d, conf, Ks, root_xyz=None, kp3d=None, conf3d=None, *, iters=151, weights=FIT_WEIGHT_DEFAULTS, lr=None,
                  lr_mult=(1.0, 1.0, 1.0, 0.1), prior="tsa", root_id=None):
    """Refine the MANO prediction in `outputs` against kp2d [B,21,2] (pixels) with confidences conf [B,21] or [B,21,1] under the cameras
    Ks [B,3,3].  root_xyz [B,3] or [B,1,3] is the start of the root position; without it root_from_keypoints supplies one.
    -> dict(pose_params, shape_params, root_xyz, joints, mano_verts, j2d, fit_trace, fit_done); the mesh and joints are recomputed by one
    ops.mano_full call at the refined parameters."""
    from . import ops
    from .traineval import proj_func
    if getattr(model, "hand_model", "mano") != "mano":
        raise NotImplementedError("fit_keypoints fits the MANO layer's pose and shape; the NIMBLE-shaped layer has another pose space and "
                                  "another skin (csrc/lbs.hip), which the one-launch fit does not implement")
    handle = model.hand_layer.handle
    root_id = model.root_id if root_id is None else root_id
    pose, beta = outputs["pose_params"].detach().float(), outputs["shape_params"].detach().float()
    B = pose.shape[0]
    conf = conf.detach().reshape(B, 21).float()
    kp2d, Ks = kp2d.detach().float(), Ks.detach().float()
    if root_xyz is None:
        root = root_from_keypoints(outputs["joints"].detach().float(), kp2d, conf, Ks)
    else:
        root = root_xyz.detach().reshape(B, 3).float()
    pr = tsa_tables(pose.device) if isinstance(prior, str) and prior == "tsa" else None if prior is None else tuple(prior)
    pose, beta, root, trace, done = ops.mano_fit(handle, pose, beta, root, Ks, kp2d, conf, kp3d, conf3d, iters=iters, lr=lr, weights=weights,
                                                 lr_mult=lr_mult, prior=pr, root_id=root_id)
    joints, verts, _, _, _, _ = ops.mano_full(handle, pose, beta, root_id, None)
    return {"pose_params": pose, "shape_params": beta, "root_xyz": root, "joints": joints, "mano_verts": verts,
            "j2d": proj_func(joints + root.unsqueeze(1), Ks), "fit_trace": trace, "fit_done": done}


def refine_outputs(model, outputs, examples, args, root_xyz=None, root_id=None):
    """The evaluation loops' hook: with the option on and the target in the batch, the refined joints / vertices / j2d replace the
    network's in a shallow copy of `outputs` (rendered images and texture outputs stay the network's) -> (outputs, refined?).
    root_xyz: the start of the root position (None: root_from_keypoints); root_id: the root joint of this pass (None: the model's)."""
    if not getattr(args, "fit_keypoints", False):
        return outputs, False
    opt = fit_options(args)
    target = fit_target_of(examples, opt["target"])
    if target is None or "Ks" not in examples:
        return outputs, False
    with torch.no_grad():
        fitted = fit_keypoints(model, outputs, target[0], target[1], examples["Ks"], root_xyz, iters=opt["iters"], weights=opt["weights"],
                               root_id=root_id)
    refined = dict(outputs)
    refined.update(fitted)
    return refined, True
