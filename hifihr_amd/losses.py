"""`LossFunction` with the reference's call signature, loss names and formulas
(reference losses.py:226-453; helpers utils/losses_util.py:217-301,366-378; utils/pytorch_ssim:17-37).

ONE path: GROUPS below lists every term, group by group, in the order they are evaluated; `LossFunction.__call__` walks it.  A group with
an `ops` entry runs as one fused HIP kernel pair on GPU tensors (csrc/losses.hip: two launches per group instead of ~250 ATen launches for
the photometric block and the geometry terms); a CPU tensor raises (no fallback).  The rarely used terms (mscale, scale, iou, mtex and the
self-supervised `*_self` terms) are a handful of torch ops on the same GPU tensors.  The torch restatement of the whole function that the
tests compare against is oracle/loss_oracle.py (pinned by the reference's own LossFunction.__call__, tests/golden/loss_dict.npz).
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import ops

# bones of the 21-joint FreiHAND skeleton, (parent, child) per row of mat_20_21 (utils/losses_util.py:226-245)
_BONES = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12),
          (0, 13), (13, 14), (14, 15), (15, 16), (0, 17), (17, 18), (18, 19), (19, 20)]

_BONE_IDX = {}


def bone_direction_loss(j, j_gt, conf=None):
    """utils/losses_util.py:217-283 with confidence 1 (as both call sites in losses.py:269-282 pass)."""
    if j.device not in _BONE_IDX:            # built once per device: a hipGraph capture of the step must not copy from the host
        _BONE_IDX[j.device] = (torch.tensor([b[0] for b in _BONES], device=j.device), torch.tensor([b[1] for b in _BONES], device=j.device))
    p, c = _BONE_IDX[j.device]
    v = j[:, c] - j[:, p]
    vg = j_gt[:, c] - j_gt[:, p]
    vn = v / (torch.sqrt((v ** 2).sum(-1, keepdim=True)) + 1e-4)
    vgn = vg / (torch.sqrt((vg ** 2).sum(-1, keepdim=True)) + 1e-4)
    return ((vn - vgn) ** 2).sum(-1).mean()


def edge_length_loss(pred, gt, face):
    """utils/losses_util.py:285-301."""
    f = face[0].long()
    def lens(x):
        a, b, c = x[:, f[:, 0]], x[:, f[:, 1]], x[:, f[:, 2]]
        return torch.cat([torch.sqrt(((a - b) ** 2).sum(2, keepdim=True)), torch.sqrt(((a - c) ** 2).sum(2, keepdim=True)),
                          torch.sqrt(((b - c) ** 2).sum(2, keepdim=True))], 1)
    return torch.abs(lens(pred) - lens(gt)).mean()


def iou(s_gt, s_est):
    """utils/losses_util.py:366-378."""
    b = s_gt.shape[0]
    mul = (s_gt * s_est).reshape(b, -1).sum(1)
    add = (s_gt + s_est).reshape(b, -1).sum(1)
    return 1 - torch.mean(mul / (add - mul))


# MEASURED (round 5, B = 32, gpurun_out/gb*.json): the geometry terms on a branch of their own make the captured step SLOWER, 5.31 -> 5.38
# ms/step -- a fork / join pair of the replayed graph costs more than the ~30 us of launches this branch hides (the light estimator's ~28
# launches are worth it: 5.38 -> 5.32).  Off by default; HIFIHR_GEOM_BRANCH=1 to re-measure.
_GEOM_BRANCH = os.environ.get("HIFIHR_GEOM_BRANCH", "0") != "0"


# ---- which mesh, which target: the four selections the mesh terms share ------------------------------------------------------------------
def _mano_faces(outputs):
    """The MANO faces [F, 3] int32: the model's own tensor, else (outputs that did not come from models.Model) the reference's key."""
    faces = outputs.get("_faces_i32")
    return faces if faces is not None else outputs["mano_faces"][0].int().contiguous()


def _callers_mesh(outputs):
    """(verts, faces [F, 3]) when the caller supplies outputs['verts'] AND outputs['faces'], else None.  They are the reference's keys: it
    asserts that both are present, and its own model never sets 'faces' (the loss-helpers row).  faces [B, F, 3]: one
    topology for the batch."""
    verts, faces = outputs.get("verts"), outputs.get("faces")
    if verts is None or faces is None:
        return None
    return verts, (faces[0] if faces.dim() == 3 else faces)


def _skin(outputs, args):
    """The dense skin of the NIMBLE-shaped layer, made root-relative like mano_verts, else None."""
    if getattr(args, "hand_model", "mano") == "nimble" and outputs.get("verts") is not None and outputs.get("_pred_root") is not None:
        return outputs["verts"] - outputs["_pred_root"]
    return None


def _target_points(examples):
    """The target of chamfer / point_mesh: a point cloud of any size (examples['chamfer_points'], in the root-relative frame of
    examples['verts']), else the ground-truth vertices."""
    points = examples.get("chamfer_points")
    return points if points is not None else examples["verts"]


# ---- the groups: fn(c, lam) picks the inputs and calls the one ops entry.  c: what __call__ was given (ex, out, used, dat_name, args, lf)
# plus `parts` (LossFunction._total_parts) and `join`; lam: the group's weights, 0.0 for a name that is not requested -------------------------
def _geometry(c, lam):
    """joint_3d / vert_3d / edge_length / mshape / mpose (reference losses.py:259-266, 283-284, 398-406) in one kernel pair (csrc/losses.hip)."""
    faces = _mano_faces(c.out) if "edge_length" in c.used else None
    # a term that is not requested has weight 0: any tensor of the right shape serves as its (absent) ground truth
    joints_gt = c.ex["joints"] if "joints" in c.ex else c.out["joints"].detach()
    verts_gt = c.ex["verts"] if "verts" in c.ex else c.out["mano_verts"].detach()
    # the geometry terms need nothing of the renderer: on a side stream they (and their backward) run beside the render / photometric
    # chain (ops.side_branch); __call__ joins the branch when every term is enqueued
    with ops.side_branch(c.out["joints"], "geom", enabled=_GEOM_BRANCH and "re_img" in c.out,
                         inputs=(joints_gt, c.out["mano_verts"], verts_gt, c.out["shape_params"], c.out["pose_params"])) as br:
        vec = ops.geom_losses(c.out["joints"], joints_gt, c.out["mano_verts"], verts_gt, c.out["shape_params"], c.out["pose_params"], faces,
                              c.args.base_loss_fn != "L1", lam)
    c.join = (br, vec)
    return vec


def _joints(c, lam):
    """The three supervised joint terms in one kernel pair (csrc/losses.hip joint_terms_*; 21-joint skeleton)."""
    two, three = "joint_2d" in c.used or "bone_direc" in c.used, "bone_direc_3d" in c.used
    return ops.joint_terms(c.out["j2d"] if two else None, c.ex["j2d_gt"] if two else None, c.out["joints"] if three else None,
                           c.ex["joints"] if three else None, c.args.base_loss_fn != "L1", lam)


def _open2d(c, lam):
    """The self-supervised keypoint terms (the reference's deprecated loss_func, losses.py:45-63, 79-85: its LossFunction class dropped
    them while its self_superv_* configs still name them): the projected joints against off-the-shelf 2-D detections weighted by the
    detector's confidences, one kernel pair (csrc/losses.hip open2d_terms_*).  include/hifihr.h states the two decided corners (d = 0; a
    batch whose confidences are all 0)."""
    assert "open_2dj" in c.ex and "open_2dj_con" in c.ex and "j2d" in c.out, (
        "the loss terms 'open_2dj' / 'open_bone_direc' / 'open_2dj_de' need examples['open_2dj'] and examples['open_2dj_con'] (2-D "
        "detections and their confidences: data_dic passes them through, FreiHandDeviceCache(open_2dj=..., open_2dj_con=...) "
        "produces them) and outputs['j2d'] (traineval's step projects it when one of the names is in args.losses)")
    return ops.open2d_terms(c.out["j2d"], c.ex["open_2dj"], c.ex["open_2dj_con"], lam)


def _bone_9_10(outputs):
    return torch.sqrt(torch.sum((outputs["joints"][:, 9] - outputs["joints"][:, 10]) ** 2, 1))


def _mscale(c, lam):
    bl = _bone_9_10(c.out)
    return lam[0] * F.l1_loss(bl, torch.ones_like(bl) * 0.0282)


def _scale(c, lam):
    bl = _bone_9_10(c.out)
    return lam[0] * F.mse_loss(bl, c.ex["scales"].to(bl.device))


def _rendered(c):
    return "re_img" in c.out and "re_sil" in c.out


def _photo_self(c, lam):
    """The self-supervised photometric terms (losses.py:317-340): confidence-weighted, against the image masked by the RENDERED
    silhouette (outputs['maskRGBs']) and with the unmasked render."""
    mask_rgbs, re_img, con = c.out["maskRGBs"], c.out["re_img"], c.ex["texture_con"]
    b = re_img.shape[0]
    c2 = con.view(-1) ** 2
    per = torch.abs(re_img - mask_rgbs).reshape(b, -1).sum(1)
    dm = torch.abs(torch.mean(re_img.reshape(b, -1), 1) - torch.mean(mask_rgbs.reshape(b, -1), 1))
    return (lam[0] * (torch.sum(per * c2) / (torch.sum(c2) * (re_img.numel() // b))), lam[1] * (torch.sum(dm * c2) / torch.sum(c2)),
            ops.ssim_loss(re_img, mask_rgbs, lam[2]))


def _photo(c, lam):
    """The photometric block (losses.py:355-378) + `sil` (:398-403) from the renderer's rgba in one kernel pair, then SSIM (csrc/ssim.hip)
    on the two images the kernel wrote: lambda * (1 - ssim), scalar glue folded in.  Two tensors, so the group registers its own parts.
    The kernel weights `sil` whether or not it is requested; an unrequested `sil` is left out of the count instead."""
    rgba = c.out.get("_rgba")
    if rgba is None:                         # outputs that did not come from models.Model: alpha = the binarised silhouette
        rgba = torch.cat([c.out["re_img"], (c.out["re_sil"] > 0).to(c.out["re_img"].dtype)], 1)
    out, re_img, mask_rgbs = ops.photo_losses(rgba, c.ex["imgs"], c.ex["segms_gt"], lam[0], lam[1], c.args.lambda_silhouette)
    tex, mrgb, sil, _ = out.unbind(0)
    ssim_tex = ops.ssim_loss(re_img, mask_rgbs, lam[2])
    c.parts.append((out, 3, ["texture", "mrgb", "sil"]) if "sil" in c.used else (out, 2, ["texture", "mrgb"]))
    c.parts.append((ssim_tex, 1, ["ssim_tex"]))
    return tex, mrgb, ssim_tex, sil


def _composite(c):
    seg = c.ex["segms_gt"].unsqueeze(1)
    return c.out["re_img"] * seg + c.ex["imgs"] * (1 - seg)


def _perceptual(c, lam):
    if c.lf.perceptual_loss is None:
        from .perceptual import PerceptualLoss
        c.lf.perceptual_loss = PerceptualLoss().to(c.out["re_img"].device)
    return lam[0] * c.lf.perceptual_loss(_composite(c), c.ex["imgs"])


def _lpips(c, lam):
    """Not in the reference (its LPIPS is an evaluation metric): the metric the evaluation pass reports, as a loss on the composite the
    `perceptual` term uses; images in [0, 1] (normalize=True), the target a constant (hifihr_amd/lpips.py, differentiable=True with its
    HIP backward, csrc/lpips.hip)."""
    fn = c.lf._lpips_module(c.args, c.out["re_img"].device)
    return lam[0] * fn(_composite(c), c.ex["imgs"], normalize=True).mean()


def _iou(c, lam):
    return lam[0] * iou(c.out["re_sil"], c.ex["segms_gt"].unsqueeze(1).float())


def _soft_sil(c, lam):
    """Not in the reference: `sil` and `iou` on the model's opt-in differentiable silhouette, one kernel pair (csrc/soft_sil.hip)."""
    assert "re_sil_soft" in c.out, ("the loss terms 'sil_soft' / 'iou_soft' need outputs['re_sil_soft']: build the model with "
                                    "Model(..., soft_silhouette=True) (options: soft_silhouette)")
    return ops.soft_sil_losses(c.out["re_sil_soft"], c.ex["segms_gt"], *lam)


def _mesh_reg(c, lam):
    """`triangle` (losses.py:421-429: lambda_laplacian * mesh_laplacian_smoothing(Meshes(verts, faces), method="uniform")) and its partner
    `normal_consistency` (not in the reference), one kernel pair (csrc/mesh_reg.hip).  The term cannot run in the reference (see
    _callers_mesh); here a caller that supplies both keys gets them, and without them the MANO-topology mesh of the model is regularised."""
    verts, faces = _callers_mesh(c.out) or (c.out["mano_verts"], None)
    topo = c.out.get("_mesh_topo") if faces is None else None          # the model's own table is the MANO mesh's
    if topo is None:                         # the caller's mesh, or outputs that did not come from models.Model: built once per faces tensor
        topo = ops.mesh_topology_of(faces if faces is not None else _mano_faces(c.out), verts.shape[1])
    return ops.mesh_regularizers(topo, verts, *lam)


def _chamfer(c, lam):
    """Not wired in the reference (utils/losses_util.py:304-337 ChamferLoss is defined, its import in losses.py:7 is commented out):
    lambda_chamfer * (mean squared distance to the nearest point, prediction -> target + target -> prediction), one kernel pair
    (csrc/chamfer.hip).  It needs no correspondence, so it reaches the dense skin of the NIMBLE-shaped layer, which no other geometry
    term does, and it takes a point cloud of any size as the target."""
    pred = c.out.get("chamfer_points")
    pred = pred if pred is not None else _skin(c.out, c.args)
    pred = pred if pred is not None else c.out["mano_verts"]
    return ops.chamfer_distance(pred, _target_points(c.ex), lam[0], lam[0])


def _point_mesh(c, lam):
    """Not in the reference: lambda_point_mesh * (mean squared distance of the target points to the closest TRIANGLE of the predicted
    mesh) + lambda_point_mesh_faces * (mean squared distance of the predicted faces to their closest target point; 0 by default: that
    direction is then not searched), one kernel pair (csrc/point_mesh.hip).  Zero exactly when the target points lie on the predicted
    surface, which `chamfer` on vertex sets of different density is not.  The target is the one of `chamfer`; the mesh is the caller's
    when given, else the dense skin with its faces, else the MANO-topology mesh."""
    mesh, skin_faces = _callers_mesh(c.out), c.out.get("_skin_faces_i32")
    if mesh is None and skin_faces is not None and (skin := _skin(c.out, c.args)) is not None:
        mesh = skin, skin_faces
    verts, faces = mesh or (c.out["mano_verts"], _mano_faces(c.out))
    return ops.point_mesh_distance(_target_points(c.ex), verts, faces, lam[0], c.args.lambda_point_mesh_faces)


def _depth(c, lam):
    """Declared, never wired in the reference (options lambda_depth, the dataset's depth_crop, a mention of outputs['re_depth'] in its
    loss code; its model renders no depth): lambda_depth * mean |re_depth - depths| over the pixels the mesh covers, the depth image
    measures (> 0), the hand mask keeps and -- with depth_trunc > 0 -- that lie within depth_trunc of the target, one kernel pair
    (csrc/depth.hip) on the model's opt-in depth map.  Dense, absolute in Z and free of correspondences.  examples['depths'] [B, H, W] is
    in the unit of the vertices."""
    assert "re_depth" in c.out and "_re_depth_hits" in c.out, (
        "the loss term 'depth' needs outputs['re_depth']: build the model with Model(..., render_depth=True) (options: render_depth)")
    return ops.depth_loss(c.out["re_depth"], c.out["_re_depth_hits"], c.ex["depths"], c.ex.get("segms_gt"), lam[0],
                          getattr(c.args, "depth_trunc", 0.0))


def _mtex(c, lam):
    return lam[0] * F.mse_loss(c.out["texture_params"], torch.zeros_like(c.out["texture_params"]))


class Group(NamedTuple):
    names: tuple        # in the order of the values fn returns
    lam: tuple          # per name, the attribute of `args` that carries its weight
    fn: object          # fn(c, lam) -> a vector whose leading entries are the names' values, a 0-d tensor, or a tuple of 0-d tensors
    cond: object = None     # cond(c): a further condition for the group to run
    always: tuple = ()      # names computed and reported whether or not they are requested: the group then runs on `cond` alone
    needs: dict = {}        # key of outputs that the step must provide -> the names that read it
    total: int = 0          # > 0: fn's result registers for total()'s one launch with this many leading entries (every entry of a vector
                            # is a term: the ones that were not asked for carry weight 0)


_GEOM_LAM = ("lambda_j3d", "lambda_vert_3d", "lambda_edge_len", "lambda_shape", "lambda_pose")
_PHOTO, _PHOTO_LAM = ("texture", "mrgb", "ssim_tex"), ("lambda_texture", "lambda_mrgb", "lambda_ssim_tex")
# in the order of evaluation, which is also the order of loss_dic's keys
GROUPS = (
    Group(ops.GEOM_TERMS, _GEOM_LAM, _geometry, total=5),
    # outside total()'s parts, as ever: the kernel pair (round 3) is older than total(), whose commit registered the geometry and photo
    # vectors of the default list only, and neither DESIGN.md, docs/HISTORY.md nor a commit message says that this vector was left out
    # on purpose.  No list the project ships would notice: those that name a joint term (configs[2] / [4]) also carry mtex and
    # perceptual, torch terms that send total() to stack + sum whatever is registered
    Group(("joint_2d", "bone_direc", "bone_direc_3d"), ("lambda_j2d_gt", "lambda_bone_direc", "lambda_bone_direc_3d"), _joints,
          needs={"j2d": ("joint_2d", "bone_direc")}),
    Group(ops.OPEN2D_TERMS, ("lambda_j2d", "lambda_bone_direc", "lambda_j2d_de"), _open2d, needs={"j2d": ops.OPEN2D_TERMS}, total=3),
    Group(("mscale",), ("lambda_mscale",), _mscale),
    Group(("scale",), ("lambda_scale",), _scale, cond=lambda c: c.dat_name in ("FreiHand", "RHD")),
    Group(tuple(k + "_self" for k in _PHOTO), _PHOTO_LAM, _photo_self, cond=lambda c: _rendered(c) and "texture_con" in c.ex,
          always=tuple(k + "_self" for k in _PHOTO)),
    Group(_PHOTO + ("sil",), _PHOTO_LAM + ("lambda_silhouette",), _photo, cond=_rendered, always=_PHOTO),
    Group(("perceptual",), ("lambda_percep",), _perceptual),
    Group(("lpips",), ("lambda_lpips",), _lpips),
    Group(("iou",), ("lambda_iou",), _iou),
    Group(("sil_soft", "iou_soft"), ("lambda_silhouette_soft", "lambda_iou_soft"), _soft_sil, total=2),
    Group(ops.MESH_REG_TERMS, ("lambda_laplacian", "lambda_normal_consistency"), _mesh_reg, total=2),
    Group(("chamfer",), ("lambda_chamfer",), _chamfer, total=1),
    Group(("point_mesh",), ("lambda_point_mesh",), _point_mesh, total=1),
    Group(("depth",), ("lambda_depth",), _depth, total=1),
    Group(("mtex",), ("lambda_tex_reg",), _mtex, cond=lambda c: c.out.get("texture_params") is not None),
)

# every name LossFunction.__call__ can produce (a name outside it in `losses` is ignored here and stops traineval's step with a KeyError)
TERMS = tuple(k for g in GROUPS for k in g.names)


def requested_needing(key, loss_used):
    """The names of loss_used that read outputs[key], which the step computes only for them (traineval: 'j2d', the projected joints)."""
    return [k for k in loss_used if any(k in g.needs.get(key, ()) for g in GROUPS)]


class LossFunction:
    def __init__(self, perceptual=None, lpips=None):
        # PerceptualLoss instance; None = built on first use (hifihr_amd/perceptual.py: seeded torchvision-style
        # initialisation unless the caller loads VGG19 weights -- they cannot be downloaded offline)
        self.perceptual_loss = perceptual
        # LPIPS(differentiable=True) instance of the opt-in term `lpips`; None = built on first use (args.lpips_weights when given, else the
        # seeded weights and one warning)
        self.lpips_loss = lpips
        # (vector, leading entries that are terms, their names) of the last __call__: the terms that live in the fused kernels' output
        # vectors; `total` sums them in one launch when they are exactly the requested list
        self._total_parts = []

    def _lpips_module(self, args, device):
        if self.lpips_loss is None:
            from .lpips import LPIPS, load_lpips_weights
            m = LPIPS(net="alex", differentiable=True)
            paths = getattr(args, "lpips_weights", None)
            if paths:
                load_lpips_weights(m, *([paths] if isinstance(paths, str) else paths))
            else:
                import warnings
                warnings.warn("loss term 'lpips': no lpips_weights given -- the AlexNet trunk and the lin layers carry SEEDED random weights, "
                              "not the calibrated metric's (hifihr_amd/lpips.py)", stacklevel=3)
            self.lpips_loss = m.to(device)
        return self.lpips_loss

    def __call__(self, examples, outputs, loss_used, dat_name, args) -> dict:
        loss_dic, self._total_parts = {}, []
        c = SimpleNamespace(ex=examples, out=outputs, used=loss_used, dat_name=dat_name, args=args, lf=self, parts=self._total_parts, join=None)
        try:
            for g in GROUPS:
                report = [k for k in g.names if k in loss_used or k in g.always]
                if not report or (g.cond is not None and not g.cond(c)):
                    continue
                res = g.fn(c, tuple(getattr(args, a) if k in report else 0.0 for k, a in zip(g.names, g.lam)))
                vals = res if isinstance(res, tuple) else res.unbind(0) if res.dim() else (res,)
                loss_dic.update((k, v) for k, v in zip(g.names, vals) if k in report)
                if g.total:
                    self._total_parts.append((res, g.total, report))
        finally:
            if c.join is not None:           # the geometry branch meets the main stream behind the last term
                c.join[0].join(c.join[1])
        return loss_dic

    def total(self, loss_dic, losses):
        """sum(loss_dic[k] for k in losses) (reference train_hrnet.py:98-104) -- in ONE launch when the requested terms are exactly the
        ones the fused kernels of the last __call__ hold in their output vectors, else as a stack + sum."""
        # (a vector none of whose terms is requested -- the photometric block of a rendering model under a keypoint-only list -- is left out)
        parts = [p for p in self._total_parts if any(k in losses for k in p[2])]
        covered = [k for _, _, names in parts for k in names]
        if (parts and len(parts) <= 4 and sorted(covered) == sorted(losses) and all(p.is_cuda for p, _, _ in parts)
                and all(loss_dic.get(k) is not None for k in losses)):
            return ops.loss_total([(p, n) for p, n, _ in parts])
        terms = [loss_dic[k] for k in losses]
        return terms[0] if len(terms) == 1 else torch.stack(terms).sum()      # 2 launches instead of a chain of adds
