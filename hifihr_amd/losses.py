"""`LossFunction` with the reference's call signature, loss names and formulas
(reference losses.py:226-453; helpers utils/losses_util.py:217-301,366-378; utils/pytorch_ssim:17-37).

ONE path: the step's terms run as fused HIP kernels -- SSIM (csrc/ssim.hip), the photometric block and the joint / vertex /
edge-length / shape / pose terms (csrc/losses.hip: two launches per group instead of ~250 ATen launches) -- on GPU tensors; a CPU
tensor raises (no fallback).  joint_2d / bone_direc / bone_direc_3d: one more kernel pair (round 3).  triangle / normal_consistency (the
reference's uniform-Laplacian term and, not in the reference, its usual partner): one kernel pair (csrc/mesh_reg.hip).  chamfer (the reference's
unwired ChamferLoss): one kernel pair (csrc/chamfer.hip).  point_mesh (not in the
reference: the distance of the target points to the SURFACE of the predicted mesh): one kernel pair (csrc/point_mesh.hip).  depth (declared and
never computed in the reference: the mean |rendered depth - depth image| on the model's opt-in depth map, outputs['re_depth']): one kernel pair
(csrc/depth.hip).  open_2dj / open_bone_direc / open_2dj_de (the self-supervised keypoint terms of the reference's deprecated loss_func, which
its configs still name): one kernel pair (csrc/losses.hip open2d_terms_*).  sil_soft / iou_soft (not in the
reference: `sil` and `iou` on the model's opt-in differentiable silhouette, outputs['re_sil_soft']): one kernel pair (csrc/soft_sil.hip).  lpips (not in the
reference: LPIPS(alex), the evaluation pass's texture metric, as an opt-in loss): hifihr_amd/lpips.py with its HIP backward (csrc/lpips.hip).  The rarely used terms (mscale, scale,
iou, mtex and the self-supervised `*_self` terms) are a handful of torch ops on the same GPU tensors.  The torch restatement of the whole function that the tests
compare against is oracle/loss_oracle.py (pinned by the reference's own LossFunction.__call__, tests/golden/loss_dict.npz).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

# bones of the 21-joint FreiHAND skeleton, (parent, child) per row of mat_20_21 (utils/losses_util.py:226-245)
_BONES = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 5), (5, 6), (6, 7), (7, 8), (0, 9), (9, 10), (10, 11), (11, 12),
          (0, 13), (13, 14), (14, 15), (15, 16), (0, 17), (17, 18), (18, 19), (19, 20)]


# every name LossFunction.__call__ can produce (a name outside it in `losses` is ignored here and stops traineval's step with a KeyError)
TERMS = ("joint_3d", "vert_3d", "edge_length", "mshape", "mpose", "joint_2d", "bone_direc", "bone_direc_3d", "mscale", "scale", "texture",
         "mrgb", "ssim_tex", "sil", "texture_self", "mrgb_self", "ssim_tex_self", "perceptual", "iou", "sil_soft", "iou_soft", "triangle",
         "normal_consistency", "lpips", "chamfer", "point_mesh", "depth", "mtex", "open_2dj", "open_bone_direc", "open_2dj_de")

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


class LossFunction:
    def __init__(self, perceptual=None, lpips=None):
        # PerceptualLoss instance; None = built on first use (hifihr_amd/perceptual.py: seeded torchvision-style
        # initialisation unless the caller loads VGG19 weights -- they cannot be downloaded offline)
        self.perceptual_loss = perceptual
        # LPIPS(differentiable=True) instance of the opt-in term `lpips`; None = built on first use (args.lpips_weights when given, else the
        # seeded weights and one warning)
        self.lpips_loss = lpips

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

    def _fused_geometry(self, examples, outputs, loss_used, args, loss_dic):
        """joint_3d / vert_3d / edge_length / mshape / mpose in one kernel pair (csrc/losses.hip)."""
        from . import ops
        lam = [args.lambda_j3d if "joint_3d" in loss_used else 0.0, args.lambda_vert_3d if "vert_3d" in loss_used else 0.0,
               args.lambda_edge_len if "edge_length" in loss_used else 0.0, args.lambda_shape if "mshape" in loss_used else 0.0,
               args.lambda_pose if "mpose" in loss_used else 0.0]
        faces = None
        if "edge_length" in loss_used:
            faces = outputs.get("_faces_i32")
            if faces is None:
                faces = outputs["mano_faces"][0].int().contiguous()
        # a term that is not requested has weight 0: any tensor of the right shape serves as its (absent) ground truth
        joints_gt = examples["joints"] if "joints" in examples else outputs["joints"].detach()
        verts_gt = examples["verts"] if "verts" in examples else outputs["mano_verts"].detach()
        # the geometry terms need nothing of the renderer: on a side stream they (and their backward) run beside the render / photometric
        # chain (ops.side_branch); __call__ joins the branch when every term is enqueued
        with ops.side_branch(outputs["joints"], "geom", enabled=_GEOM_BRANCH and "re_img" in outputs,
                             inputs=(joints_gt, outputs["mano_verts"], verts_gt, outputs["shape_params"], outputs["pose_params"])) as br:
            vec = ops.geom_losses(outputs["joints"], joints_gt, outputs["mano_verts"], verts_gt,
                                  outputs["shape_params"], outputs["pose_params"], faces, args.base_loss_fn != "L1", lam)
        self._pending_join = (br, vec)
        for k, v in zip(ops.GEOM_TERMS, vec.unbind(0)):
            if k in loss_used:
                loss_dic[k] = v
        # (every entry of the vector is a term: the ones that were not asked for carry weight 0)
        self._total_parts.append((vec, 5, [k for k in ops.GEOM_TERMS if k in loss_used]))

    def __call__(self, examples, outputs, loss_used, dat_name, args) -> dict:
        self._pending_join = None
        # (vector, leading entries that are terms, their names): the terms that live in the fused kernels' output vectors; `total` sums
        # them in one launch when they are exactly the requested list
        self._total_parts = []
        try:
            return self._terms(examples, outputs, loss_used, dat_name, args)
        finally:
            if self._pending_join is not None:          # the geometry branch meets the main stream behind the last term
                br, vec = self._pending_join
                br.join(vec)
                self._pending_join = None

    def total(self, loss_dic, losses):
        """sum(loss_dic[k] for k in losses) (reference train_hrnet.py:98-104) -- in ONE launch when the requested terms are exactly the
        ones the fused kernels of the last __call__ hold in their output vectors, else as a stack + sum."""
        from . import ops
        # (a vector none of whose terms is requested -- the photometric block of a rendering model under a keypoint-only list -- is left out)
        parts = [p for p in getattr(self, "_total_parts", []) if any(k in losses for k in p[2])]
        covered = [k for _, _, names in parts for k in names]
        if (parts and len(parts) <= 4 and sorted(covered) == sorted(losses) and all(p.is_cuda for p, _, _ in parts)
                and all(loss_dic.get(k) is not None for k in losses)):
            return ops.loss_total([(p, n) for p, n, _ in parts])
        terms = [loss_dic[k] for k in losses]
        return terms[0] if len(terms) == 1 else torch.stack(terms).sum()      # 2 launches instead of a chain of adds

    def _terms(self, examples, outputs, loss_used, dat_name, args) -> dict:
        from . import ops
        loss_dic = {}
        base = F.l1_loss if args.base_loss_fn == "L1" else F.mse_loss
        if any(k in loss_used for k in ("joint_3d", "vert_3d", "edge_length", "mshape", "mpose")):
            self._fused_geometry(examples, outputs, loss_used, args, loss_dic)
            loss_used = [k for k in loss_used if k not in loss_dic]
        want = [k in loss_used for k in ("joint_2d", "bone_direc", "bone_direc_3d")]
        if any(want):
            # one kernel pair for the three supervised joint terms (csrc/losses.hip joint_terms_*; 21-joint skeleton)
            two, three = want[0] or want[1], want[2]
            lam3 = (args.lambda_j2d_gt if want[0] else 0.0, args.lambda_bone_direc if want[1] else 0.0, args.lambda_bone_direc_3d if want[2] else 0.0)
            vals = ops.joint_terms(outputs["j2d"] if two else None, examples["j2d_gt"] if two else None,
                                   outputs["joints"] if three else None, examples["joints"] if three else None,
                                   args.base_loss_fn != "L1", lam3).unbind(0)
            for k, w, v in zip(("joint_2d", "bone_direc", "bone_direc_3d"), want, vals):
                if w:
                    loss_dic[k] = v
        if any(k in loss_used for k in ops.OPEN2D_TERMS):
            # the self-supervised keypoint terms (the reference's deprecated loss_func, losses.py:45-63, 79-85: its LossFunction class
            # dropped them while its self_superv_* configs still name them): the projected joints against off-the-shelf 2-D detections
            # weighted by the detector's confidences, one kernel pair (csrc/losses.hip open2d_terms_*); a term that is not requested has
            # weight 0.  include/hifihr.h states the two decided corners (d = 0; a batch whose confidences are all 0)
            assert "open_2dj" in examples and "open_2dj_con" in examples and "j2d" in outputs, (
                "the loss terms 'open_2dj' / 'open_bone_direc' / 'open_2dj_de' need examples['open_2dj'] and examples['open_2dj_con'] (2-D "
                "detections and their confidences: data_dic passes them through, FreiHandDeviceCache(open_2dj=..., open_2dj_con=...) "
                "produces them) and outputs['j2d'] (traineval's step projects it when one of the names is in args.losses)")
            names = [k for k in ops.OPEN2D_TERMS if k in loss_used]
            vec = ops.open2d_terms(outputs["j2d"], examples["open_2dj"], examples["open_2dj_con"],
                                   (args.lambda_j2d if "open_2dj" in loss_used else 0.0,
                                    args.lambda_bone_direc if "open_bone_direc" in loss_used else 0.0,
                                    args.lambda_j2d_de if "open_2dj_de" in loss_used else 0.0))
            for k, v in zip(ops.OPEN2D_TERMS, vec.unbind(0)):
                if k in loss_used:
                    loss_dic[k] = v
            self._total_parts.append((vec, 3, names))
        if "mscale" in loss_used:
            bl = torch.sqrt(torch.sum((outputs["joints"][:, 9] - outputs["joints"][:, 10]) ** 2, 1))
            loss_dic["mscale"] = args.lambda_mscale * F.l1_loss(bl, torch.ones_like(bl) * 0.0282)
        if "scale" in loss_used and dat_name in ("FreiHand", "RHD"):
            bl = torch.sqrt(torch.sum((outputs["joints"][:, 9] - outputs["joints"][:, 10]) ** 2, 1))
            loss_dic["scale"] = args.lambda_scale * F.mse_loss(bl, examples["scales"].to(bl.device))
        if "re_img" in outputs and "re_sil" in outputs and "texture_con" in examples:
            # self-supervised photometric terms (losses.py:317-340): confidence-weighted, against the image masked by the RENDERED
            # silhouette (outputs['maskRGBs']) and with the unmasked render
            mask_rgbs, re_img, con = outputs["maskRGBs"], outputs["re_img"], examples["texture_con"]
            b = re_img.shape[0]
            c2 = con.view(-1) ** 2
            per = torch.abs(re_img - mask_rgbs).reshape(b, -1).sum(1)
            loss_dic["texture_self"] = args.lambda_texture * (torch.sum(per * c2) / (torch.sum(c2) * (re_img.numel() // b)))
            dm = torch.abs(torch.mean(re_img.reshape(b, -1), 1) - torch.mean(mask_rgbs.reshape(b, -1), 1))
            loss_dic["mrgb_self"] = args.lambda_mrgb * (torch.sum(dm * c2) / torch.sum(c2))
            loss_dic["ssim_tex_self"] = ops.ssim_loss(re_img, mask_rgbs, args.lambda_ssim_tex)
        if "re_img" in outputs and "re_sil" in outputs:
            # photometric block (losses.py:355-378) + `sil` (:398-403) from the renderer's rgba in one kernel pair
            rgba = outputs.get("_rgba")
            if rgba is None:                     # outputs that did not come from models.Model: alpha = the binarised silhouette
                rgba = torch.cat([outputs["re_img"], (outputs["re_sil"] > 0).to(outputs["re_img"].dtype)], 1)
            out, re_img, mask_rgbs = ops.photo_losses(rgba, examples["imgs"], examples["segms_gt"], args.lambda_texture,
                                                      args.lambda_mrgb, args.lambda_silhouette)
            tex, mrgb, sil, _ = out.unbind(0)
            loss_dic["texture"], loss_dic["mrgb"] = tex, mrgb
            loss_dic["ssim_tex"] = ops.ssim_loss(re_img, mask_rgbs, args.lambda_ssim_tex)   # lambda * (1 - ssim), scalar glue folded in
            if "sil" in loss_used:
                loss_dic["sil"] = sil
                self._total_parts.append((out, 3, ["texture", "mrgb", "sil"]))
            else:
                self._total_parts.append((out, 2, ["texture", "mrgb"]))
            self._total_parts.append((loss_dic["ssim_tex"], 1, ["ssim_tex"]))
        if "perceptual" in loss_used:
            if self.perceptual_loss is None:
                from .perceptual import PerceptualLoss
                self.perceptual_loss = PerceptualLoss().to(outputs["re_img"].device)
            seg = examples["segms_gt"].unsqueeze(1)
            loss_dic["perceptual"] = args.lambda_percep * self.perceptual_loss(
                outputs["re_img"] * seg + examples["imgs"] * (1 - seg), examples["imgs"])
        if "lpips" in loss_used:
            # not in the reference (its LPIPS is an evaluation metric): the metric the evaluation pass reports, as a loss on the composite the
            # `perceptual` term uses; images in [0, 1] (normalize=True), the target a constant (hifihr_amd/lpips.py, differentiable=True)
            seg = examples["segms_gt"].unsqueeze(1)
            fn = self._lpips_module(args, outputs["re_img"].device)
            loss_dic["lpips"] = args.lambda_lpips * fn(outputs["re_img"] * seg + examples["imgs"] * (1 - seg), examples["imgs"],
                                                       normalize=True).mean()
        if "iou" in loss_used:
            loss_dic["iou"] = args.lambda_iou * iou(outputs["re_sil"], examples["segms_gt"].unsqueeze(1).float())
        if "sil_soft" in loss_used or "iou_soft" in loss_used:
            # the two terms of the differentiable silhouette, one kernel pair (csrc/soft_sil.hip); a term that is not requested has weight 0
            assert "re_sil_soft" in outputs, ("the loss terms 'sil_soft' / 'iou_soft' need outputs['re_sil_soft']: build the model with "
                                              "Model(..., soft_silhouette=True) (options: soft_silhouette)")
            names = [k for k in ("sil_soft", "iou_soft") if k in loss_used]
            vec = ops.soft_sil_losses(outputs["re_sil_soft"], examples["segms_gt"],
                                      args.lambda_silhouette_soft if "sil_soft" in loss_used else 0.0,
                                      args.lambda_iou_soft if "iou_soft" in loss_used else 0.0)
            for k, v in zip(("sil_soft", "iou_soft"), vec.unbind(0)):
                if k in loss_used:
                    loss_dic[k] = v
            self._total_parts.append((vec, 2, names))
        if "triangle" in loss_used or "normal_consistency" in loss_used:
            # `triangle` (losses.py:421-429: lambda_laplacian * mesh_laplacian_smoothing(Meshes(verts, faces), method="uniform")) and its
            # partner `normal_consistency` (not in the reference), one kernel pair (csrc/mesh_reg.hip); a term that is not requested has
            # weight 0.  outputs['verts'] / outputs['faces'] are the reference's keys: it asserts that both are present, and its own model
            # never sets 'faces', so the term cannot run there (the loss-helpers row).  A caller that supplies both
            # gets them; without them the MANO-topology mesh of the model is regularised
            if outputs.get("verts") is not None and outputs.get("faces") is not None:
                verts, faces = outputs["verts"], outputs["faces"]              # faces [F, 3], or [B, F, 3] with one topology for the batch
                topo = ops.mesh_topology_of(faces[0] if faces.dim() == 3 else faces, verts.shape[1])
            else:
                verts, topo = outputs["mano_verts"], outputs.get("_mesh_topo")
                if topo is None:                 # outputs that did not come from models.Model: built once per faces tensor
                    faces = outputs.get("_faces_i32")
                    if faces is None:
                        faces = outputs["mano_faces"][0].int().contiguous()
                    topo = ops.mesh_topology_of(faces, verts.shape[1])
            names = [k for k in ops.MESH_REG_TERMS if k in loss_used]
            vec = ops.mesh_regularizers(topo, verts, args.lambda_laplacian if "triangle" in loss_used else 0.0,
                                        args.lambda_normal_consistency if "normal_consistency" in loss_used else 0.0)
            for k, v in zip(ops.MESH_REG_TERMS, vec.unbind(0)):
                if k in loss_used:
                    loss_dic[k] = v
            self._total_parts.append((vec, 2, names))
        if "chamfer" in loss_used:
            # not wired in the reference (utils/losses_util.py:304-337 ChamferLoss is defined, its import in losses.py:7 is commented out):
            # lambda_chamfer * (mean squared distance to the nearest point, prediction -> target + target -> prediction), one kernel pair
            # (csrc/chamfer.hip).  It needs no correspondence, so it reaches the dense skin of the NIMBLE-shaped layer, which no other geometry
            # term does, and it takes a point cloud of any size as the target (examples['chamfer_points'], in the root-relative frame of
            # examples['verts'])
            target = examples["chamfer_points"] if examples.get("chamfer_points") is not None else examples["verts"]
            if outputs.get("chamfer_points") is not None:
                pred = outputs["chamfer_points"]
            elif getattr(args, "hand_model", "mano") == "nimble" and outputs.get("verts") is not None and outputs.get("_pred_root") is not None:
                pred = outputs["verts"] - outputs["_pred_root"]             # the dense skin, root-relative like mano_verts
            else:
                pred = outputs["mano_verts"]
            loss_dic["chamfer"] = ops.chamfer_distance(pred, target, args.lambda_chamfer, args.lambda_chamfer)
            self._total_parts.append((loss_dic["chamfer"], 1, ["chamfer"]))
        if "point_mesh" in loss_used:
            # not in the reference: lambda_point_mesh * (mean squared distance of the target points to the closest TRIANGLE of the predicted
            # mesh) + lambda_point_mesh_faces * (mean squared distance of the predicted faces to their closest target point; 0 by default: that
            # direction is then not searched), one kernel pair (csrc/point_mesh.hip).  Zero exactly when the target points lie on the predicted
            # surface, which `chamfer` on vertex sets of different density is not.  The target is the one of `chamfer`; the mesh is the
            # caller's outputs['verts'] / outputs['faces'] when both are given, else the dense skin of the NIMBLE-shaped layer made
            # root-relative, else the MANO-topology mesh
            target = examples["chamfer_points"] if examples.get("chamfer_points") is not None else examples["verts"]
            if outputs.get("verts") is not None and outputs.get("faces") is not None:
                verts, faces = outputs["verts"], outputs["faces"]              # faces [F, 3], or [B, F, 3] with one topology for the batch
                faces = faces[0] if faces.dim() == 3 else faces
            elif (getattr(args, "hand_model", "mano") == "nimble" and outputs.get("verts") is not None and outputs.get("_pred_root") is not None
                  and outputs.get("_skin_faces_i32") is not None):
                verts, faces = outputs["verts"] - outputs["_pred_root"], outputs["_skin_faces_i32"]
            else:
                verts, faces = outputs["mano_verts"], outputs.get("_faces_i32")
                if faces is None:
                    faces = outputs["mano_faces"][0].int().contiguous()
            loss_dic["point_mesh"] = ops.point_mesh_distance(target, verts, faces, args.lambda_point_mesh, args.lambda_point_mesh_faces)
            self._total_parts.append((loss_dic["point_mesh"], 1, ["point_mesh"]))
        if "depth" in loss_used:
            # declared, never wired in the reference (options lambda_depth, the dataset's depth_crop, a mention of outputs['re_depth'] in its
            # loss code; its model renders no depth): lambda_depth * mean |re_depth - depths| over the pixels the mesh covers, the depth image
            # measures (> 0), the hand mask keeps and -- with depth_trunc > 0 -- that lie within depth_trunc of the target, one kernel pair
            # (csrc/depth.hip).  Dense, absolute in Z and free of correspondences.  examples['depths'] [B, H, W] is in the unit of the vertices
            assert "re_depth" in outputs and "_re_depth_hits" in outputs, (
                "the loss term 'depth' needs outputs['re_depth']: build the model with Model(..., render_depth=True) (options: render_depth)")
            loss_dic["depth"] = ops.depth_loss(outputs["re_depth"], outputs["_re_depth_hits"], examples["depths"], examples.get("segms_gt"),
                                               args.lambda_depth, getattr(args, "depth_trunc", 0.0))
            self._total_parts.append((loss_dic["depth"], 1, ["depth"]))
        if "mtex" in loss_used and outputs.get("texture_params") is not None:
            loss_dic["mtex"] = args.lambda_tex_reg * F.mse_loss(outputs["texture_params"], torch.zeros_like(outputs["texture_params"]))
        return loss_dic
