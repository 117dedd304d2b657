"""Float64 / float32 torch restatement of the keypoint fit (include/hifihr.h: hifihr_mano_fit), test infrastructure only.

The chain is the oracle's (oracle/mano_oracle.py: mano_forward(center_idx=None) -> xyz_from_vertice -> root_relative), then X = J_rel + root,
uv = (K X)_xy / (K X)_z, the objective of the header, autograd for its gradient and torch's Adam formula with the moments kept.  The
prior's formula is pinned to the reference's own tsa_pose_loss by tests/test_mano_fit_host.py (tests/golden/mano_fit.npz).
The decided corners are written so that autograd yields the header's choice: rho below 5 px is d^2 / 10 (no square root: slope 0 at d = 0),
a bone of length 0 keeps only the direct part of its slope, a joint at or below MIN_Z is masked before the division."""
import numpy as np
import torch

from oracle import mano_oracle as mo

MIN_Z = 1e-4
BONE_PARENT = [0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
BONE_CHILD = list(range(1, 21))
DEFAULT_LR = [0.01] * 51 + [0.005] * 50 + [0.0025] * 50
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
GROUPS = ((0, 3), (3, 48), (48, 58), (58, 61))            # root rotation, pose coefficients, shape, root position in the 61-vector


def prior_per_hand(fp, lo, hi, w):
    """(1/48) sum_i w_i (max(fp_i - hi_i, 0) + max(lo_i - fp_i, 0)) with the reference's strict torch.where; fp [B,48] -> [B]."""
    z = torch.zeros_like(fp)
    err = torch.where(fp > hi, fp - hi, z) + torch.where(fp < lo, lo - fp, z)
    return (err * w).sum(1) / 48.0


def objective(tables, pose, beta, root, K, kp2d, conf, kp3d, conf3, prior, weights, root_id, dtype):
    """-> (E [B], terms [B,8] as the trace row, uv [B,21,2]); every input a tensor of `dtype` (kp3d / conf3 / prior may be None)."""
    B = pose.shape[0]
    verts, _, aux = mo.mano_forward(tables, pose, beta, dtype=dtype, center_idx=None)
    joints = mo.xyz_from_vertice(tables, verts, dtype=dtype)
    jrel, _, _ = mo.root_relative(joints, verts, root_id)
    X = jrel + root.unsqueeze(1)
    p = (X.unsqueeze(2) * K.unsqueeze(1)).sum(3)
    inside = X[:, :, 2] > MIN_Z
    pz = torch.where(inside, p[:, :, 2], torch.ones_like(p[:, :, 2]))
    uv = torch.where(inside.unsqueeze(-1), p[:, :, :2] / pz.unsqueeze(-1), torch.zeros_like(p[:, :, :2]))
    ceff = torch.where(inside, conf, torch.zeros_like(conf))
    diff = torch.where(inside.unsqueeze(-1), uv - kp2d, torch.zeros_like(uv))
    d2 = (diff * diff).sum(2)
    far = d2 >= 25.0
    d_far = torch.sqrt(torch.where(far, d2, torch.full_like(d2, 25.0)))
    rho = torch.where(far, d_far - 2.5, d2 / 10.0)
    w2 = ceff * ceff
    sw = w2.sum(1)
    e2d = torch.where(sw > 0, (w2 * rho).sum(1) / torch.where(sw > 0, sw, torch.ones_like(sw)), torch.zeros_like(sw))
    v = uv[:, BONE_CHILD] - uv[:, BONE_PARENT]
    vo = kp2d[:, BONE_CHILD] - kp2d[:, BONE_PARENT]
    s = (v * v).sum(2)
    n = torch.where(s > 0, torch.sqrt(torch.where(s > 0, s, torch.ones_like(s))), torch.zeros_like(s))
    dn = v / (n + 1e-4).unsqueeze(-1) - vo / (torch.sqrt((vo * vo).sum(2)) + 1e-4).unsqueeze(-1)
    bconf = ceff[:, BONE_PARENT] * ceff[:, BONE_CHILD]
    ebone = (torch.where(bconf != 0, (dn * dn).sum(2), torch.zeros_like(s)) * bconf).sum(1) / 20.0
    zero = torch.zeros(B, dtype=dtype)
    e3d = zero
    if kp3d is not None:
        s3 = conf3.sum(1)
        e3d = torch.where(s3 > 0, (conf3 * ((jrel - kp3d) ** 2).sum(2)).sum(1) / torch.where(s3 > 0, s3, torch.ones_like(s3)), zero)
    eprior = prior_per_hand(aux["full_pose"], *prior) if prior is not None else zero
    eshape = (beta * beta).mean(1)
    epca = (pose[:, 3:] ** 2).mean(1)
    E = weights[0] * e2d + weights[1] * ebone + weights[2] * e3d + weights[3] * eprior + weights[4] * eshape + weights[5] * epca
    seen = (inside & (conf > 0)).to(dtype)
    dist = torch.sqrt(torch.where(d2 > 0, d2, torch.ones_like(d2))) * (d2 > 0).to(dtype)
    pix = torch.where(seen.sum(1) > 0, (dist * seen).sum(1) / seen.sum(1).clamp_min(1.0), zero)
    return E, torch.stack([E, e2d, ebone, e3d, eprior, eshape, epca, pix], 1).detach(), uv.detach()


def _cast(x, dtype):
    return None if x is None else torch.as_tensor(x).to(dtype)


def fit(tables, pose, beta, root, K, kp2d, conf, kp3d=None, conf3=None, prior=None, weights=(1, 1, 0, 0, 0, 0), lr=DEFAULT_LR, iters=151,
        lr_mult=(1, 1, 1, 0.1), root_id=9, dtype=torch.float64, keep=()):
    """The fit in `dtype` -> dict(params {i: [B,61] before update i, for i in keep and i = iters}, trace [B,iters+1,8], grad0 [B,61]).
    Adam as torch.optim.Adam's single-tensor path: the bias corrections are Python floats, the state tensors are of `dtype`."""
    par = torch.cat([_cast(pose, dtype), _cast(beta, dtype), _cast(root, dtype)], 1).clone()
    K, kp2d, conf, kp3d, conf3 = (_cast(x, dtype) for x in (K, kp2d, conf.reshape(par.shape[0], 21), kp3d, conf3))
    prior = None if prior is None else tuple(_cast(x, dtype).view(1, 48) for x in prior)
    mult = torch.zeros(61, dtype=dtype)
    for (a, b), m in zip(GROUPS, lr_mult):
        mult[a:b] = m
    m1, m2 = torch.zeros_like(par), torch.zeros_like(par)
    out = {"params": {}, "trace": [], "grad0": None}
    for i in range(iters + 1):
        p = par.clone().requires_grad_(True)
        E, row, _ = objective(tables, p[:, :48], p[:, 48:58], p[:, 58:], K, kp2d, conf, kp3d, conf3, prior, weights, root_id, dtype)
        out["trace"].append(row)
        if i in keep or i == iters:
            out["params"][i] = par.clone()
        if i == iters and i > 0:
            break
        (g,) = torch.autograd.grad(E.sum(), p)
        if i == 0:
            out["grad0"] = g.clone()
        if i == iters:
            break
        t = i + 1
        m1 = m1 + (g - m1) * (1 - BETA1)
        m2 = m2 * BETA2 + g * g * (1 - BETA2)
        step = mult * (lr[i] / (1 - BETA1 ** t))
        denom = m2.sqrt() / np.sqrt(1 - BETA2 ** t) + EPS
        par = torch.where(mult != 0, par - step * (m1 / denom), par)
    out["trace"] = torch.stack(out["trace"], 1)
    return out
