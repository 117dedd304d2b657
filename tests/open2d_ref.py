"""Torch restatement of the self-supervised keypoint terms and of the data-side quantities that feed them, in the dtype of its inputs
(float64 as the yardstick; the same code in float32 gives the error a float32 evaluation makes, which the kernel bounds are built from).

  terms()              reference losses.py:45-63 (open_2dj, open_2dj_de) and :79-85 with utils/losses_util.py:217-283 (open_bone_direc) of the
                       deprecated loss_func, at the weights `lam`
  texture_con()        utils/traineval_util.py:60-64
  semi_mix()           utils/traineval_util.py:106-111
  warp()               utils/handutils.py:36-45 transform_coords WITHOUT its final astype(int) (include/hifihr.h: hifihr_freihand_keypoints)

Written out from those lines; tests/golden/open2d.npz holds what the reference's own code gives on seeded inputs
(tools/make_open2d_golden.py), and tests/test_open2d_host.py holds this file to it."""
import numpy as np
import torch

KEYPOINT_WEIGHTS = (2, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5, 1, 1, 1, 1.5)          # losses.py:49
# (parent, child) per row of mat_20_21 (utils/losses_util.py:226-245); the mask-and-gather of :257-280 walks the transposed 21 x 21 mask
# row by row, i.e. by CHILD 1 .. 20, and every child has one parent: it returns c_parent c_child in this order
BONES = ((0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12),
         (0, 13), (13, 14), (14, 15), (15, 16), (0, 17), (17, 18), (18, 19), (19, 20))
TRAIN_SIZE = 32560


def norm2(x):
    """sqrt(sum x^2) over the last axis; at x = 0 its gradient is taken as 0 (autograd's sqrt gives inf x 0 = NaN there), which is how the
    library states both corners (include/hifihr.h: d = 0, and a bone of length 0)."""
    s = torch.sum(x ** 2, -1)
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def rho(d):
    """losses.py:48."""
    return torch.where(d < 5, d ** 2 / 10, d - 2.5)


def joint_pieces(j2d, det, con):
    """-> (rho(d) (c w)^2 [B,21], (c w)^2 [B,21]): the addends of losses.py:52 before the batch-wide normalisation."""
    d = norm2(det - j2d)
    cw = con.reshape(con.shape[0], 21) * torch.tensor(KEYPOINT_WEIGHTS, dtype=j2d.dtype, device=j2d.device).view(1, 21)
    return rho(d) * cw ** 2, cw ** 2


def bone_pieces(j2d, det, con):
    """-> (|vn - von|^2 [B,20], c_parent c_child [B,20]) of utils/losses_util.py:248-282."""
    p, c = [b[0] for b in BONES], [b[1] for b in BONES]
    unit = lambda x: (x[:, c] - x[:, p]) / (norm2(x[:, c] - x[:, p]).unsqueeze(-1) + 1e-4)
    cc = con.reshape(con.shape[0], 21)
    return torch.sum((unit(j2d) - unit(det)) ** 2, 2), cc[:, p] * cc[:, c]


def terms(j2d, det, con, lam=(1.0, 1.0, 1.0), zero_weight_is_zero=True):
    """-> [3] = (open_2dj, open_bone_direc, open_2dj_de).  zero_weight_is_zero: a batch whose (c w)^2 sum to 0 gives open_2dj = 0, the
    library's documented departure from the reference's 0 / 0."""
    num, den = joint_pieces(j2d, det, con)
    if zero_weight_is_zero and float(den.sum()) == 0.0:
        t0 = (j2d * 0).sum()
    else:
        t0 = num.sum() / den.sum()
    t, cc = bone_pieces(j2d, det, con)
    return torch.stack([lam[0] * t0, lam[1] * torch.mean(t * cc), lam[2] * torch.mean((det - j2d) ** 2)])


def terms_and_grad(j2d, det, con, lam, gout, dtype=torch.float64):
    """-> (terms [3], d(sum_k gout[k] terms[k]) / d j2d [B,21,2]) in `dtype` (the gradient at d = 0 and at |v| = 0: see norm2)."""
    j = j2d.to(dtype).clone().requires_grad_(True)
    out = terms(j, det.to(dtype), con.to(dtype), lam)
    (out * torch.as_tensor(gout, dtype=dtype)).sum().backward()
    return out.detach(), j.grad


def texture_con(con, idxs):
    """utils/traineval_util.py:60-64 -> [B]; the gate compares with float32(0.1), as torch does for a float32 tensor."""
    c = con.reshape(con.shape[0], 21)
    gate = (c.min(1)[0] > float(np.float32(0.1))).to(c.dtype).unsqueeze(1)
    return torch.mean(gate * c, 1) * ((idxs < TRAIN_SIZE).to(c.dtype) + 0.1)


def semi_choice(idxs, semi_ratio):
    """utils/traineval_util.py:107-108 -> bool [B]: the samples that take the ground truth."""
    if semi_ratio is None:
        return torch.zeros(idxs.shape[0], dtype=torch.bool)
    return (idxs % TRAIN_SIZE) < TRAIN_SIZE * semi_ratio


def semi_mix(det, con, j2d_gt, idxs, semi_ratio):
    """utils/traineval_util.py:106-111 -> (open_2dj, open_2dj_con)."""
    pick = semi_choice(idxs, semi_ratio)
    return (torch.where(pick.view(-1, 1, 1), j2d_gt.to(det.dtype), det),
            torch.where(pick.view(-1, *([1] * (con.dim() - 1))), torch.ones_like(con), con))


def warp(det, total):
    """total [B,3,3] . (x, y, 1) -> [B,21,2] (handutils.transform_coords, rows 0-1, no truncation)."""
    hom = torch.cat([det, torch.ones_like(det[..., :1])], -1)
    return torch.einsum("bij,bnj->bni", total.to(det.dtype), hom)[..., :2]
