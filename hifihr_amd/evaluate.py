"""Evaluation pass of the reference's loop (reference train_hrnet.py:119-161 collection + texture metrics, :216-272
MPJPE / MPVPE after Procrustes alignment; utils/train_utils.py:267-290 align_w_scale) with the alignment batched on the
device (csrc/eval.hip) instead of a per-sample numpy / scipy loop.  SURVEY.md section 8(f) N2.

LPIPS (train_hrnet.py:156-158) is opt-in: `Evaluator(lpips_fn=hifihr_amd.lpips.LPIPS(...))` -- the AlexNet metric on this package's
kernels, with weights loaded by `load_state_dict_lpips` (train_hrnet.py --lpips_weights) or, without any, seeded ones.  With no
`lpips_fn` it is reported as None.  Parity with the `lpips` package and with the real weights is unpinned: neither is available here.

The FreiHAND benchmark's other `scores.txt` keys -- PCK / AUC of joints and mesh, aligned and not (reference utils/fh_utils.py:719-815
EvalUtil, instantiated at train_hrnet.py:25,43) and F@5 mm / F@15 mm -- come from `pck_auc`, `fscore` and `Evaluator(benchmark=True)`:
the device counts (csrc/eval.hip: one launch per metric), the host turns the integer counts into curves in float64.  PCK / AUC are pinned
to the reference's EvalUtil (tests/golden/benchmark_metrics.npz); the F-score has no counterpart in the reference tree and neither the
benchmark's eval.py nor open3d is available here: its parity with the benchmark's script is unpinned (tests/benchmark_ref.py restates it).

The Chamfer distance, the number mesh papers report beside the F-score, is opt-in: `chamfer` and `Evaluator(chamfer=True)` (csrc/chamfer.hip,
the kernels of the loss term of the same name; pinned to the reference's unwired ChamferLoss by tests/golden/chamfer.npz).  So is the mean
squared distance from the ground-truth vertices to the predicted SURFACE: `point_to_surface` and `Evaluator(point_mesh=True)`
(csrc/point_mesh.hip, the kernels of the loss term `point_mesh`; parity with PyTorch3D's point_mesh_face_distance is unpinned).  The
error of the rendered depth map against a depth image, `depth_mae`, is opt-in too: `depth_error` and `Evaluator(depth=True)`
(csrc/depth.hip, the kernel of the loss term `depth`)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ._lib import get_lib, require_cuda
from .traineval import Frei2HO3D


def align_w_scale(mtx1, mtx2, return_error=False):
    """utils/train_utils.py:267-290 for batches: aligns mtx2 [B,N,3] (prediction) to mtx1 [B,N,3] (ground truth) with
    translation, isotropic scale and an orthogonal map (reflections allowed, like scipy's orthogonal_procrustes).
    Returns the aligned mtx2 (and, with return_error, the per-sample mean point distance to mtx1)."""
    require_cuda(mtx1, mtx2)
    gt, pred = mtx1.float().contiguous(), mtx2.float().contiguous()
    assert gt.shape == pred.shape and gt.dim() == 3 and gt.shape[2] == 3, (gt.shape, pred.shape)
    aligned = torch.empty_like(pred)
    err = torch.empty(pred.shape[0], device=pred.device)
    get_lib().procrustes_error(pred, gt, aligned, err)
    return (aligned, err / pred.shape[1]) if return_error else aligned


def aligned_error(pred, gt):
    """Mean per-point distance after alignment, one value per sample (no aligned copy is written)."""
    require_cuda(pred, gt)
    pred, gt = pred.float().contiguous(), gt.float().contiguous()
    err = torch.empty(pred.shape[0], device=pred.device)
    get_lib().procrustes_error(pred, gt, None, err)
    return err / pred.shape[1]


BENCHMARK_KEYS = ("xyz_mean3d", "xyz_auc3d", "xyz_al_mean3d", "xyz_al_auc3d", "mesh_mean3d", "mesh_auc3d", "mesh_al_mean3d", "mesh_al_auc3d",
                  "f_score_5", "f_score_15", "f_al_score_5", "f_al_score_15")
CHAMFER_KEYS = ("mesh_chamfer", "mesh_al_chamfer")
POINT_MESH_KEYS = ("mesh_p2s", "mesh_al_p2s")
_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def point_error_counts(pred, gt, vis, thresholds):
    """hifihr_point_error_hist: (hist int32 [K, T+1], sum float64 [K]) on the device, no host sync.  pred / gt [n,K,3]; vis [n,K] or None."""
    require_cuda(pred, gt)
    pred, gt = pred.float().contiguous(), gt.float().contiguous()
    assert pred.shape == gt.shape and pred.dim() == 3 and pred.shape[2] == 3, (pred.shape, gt.shape)
    if vis is not None:
        require_cuda(vis)
        vis = (vis != 0).to(torch.uint8).contiguous()
    hist = torch.empty(pred.shape[1], len(thresholds) + 1, dtype=torch.int32, device=pred.device)
    sums = torch.empty(pred.shape[1], dtype=torch.float64, device=pred.device)
    get_lib().point_error_hist(pred, gt, vis, thresholds, hist, sums)
    return hist, sums


def pck_measures(hist, sums, thresholds):
    """EvalUtil.get_measures (utils/fh_utils.py:774-815) from the per-keypoint counts, float64 numpy on the host: hist [K, T+1] (the last
    column = beyond the last threshold), sums [K] the distance sums.  Keypoints without a visible sample are skipped, as the reference
    `continue`s; mean / auc / pck_curve are averages over the others."""
    hist, sums, thr = np.asarray(hist, np.int64), np.asarray(sums, np.float64), np.asarray(thresholds, np.float64)
    visible = hist.sum(1)
    keep = visible > 0
    if not keep.any():
        nan = float("nan")
        return {"mean": nan, "auc": nan, "pck_curve": np.full(len(thr), nan), "thresholds": thr}
    pck = np.cumsum(hist[keep, :-1], 1).astype(np.float64) / visible[keep, None].astype(np.float64)
    norm = _trapezoid(np.ones_like(thr), thr)
    auc = np.array([_trapezoid(row, thr) / norm for row in pck])
    return {"mean": float(np.mean(sums[keep] / visible[keep])), "auc": float(np.mean(auc)), "pck_curve": np.mean(pck, 0), "thresholds": thr}


def pck_auc(pred, gt, vis=None, val_min=0.0, val_max=0.05, steps=100):
    """EvalUtil.feed + get_measures(val_min, val_max, steps) for pred / gt [n,K,3] (vis [n,K]: which keypoints count): a dict with the
    mean end-point error, the area under the PCK curve, the curve and its thresholds.  The median is not computed."""
    thr = np.linspace(val_min, val_max, steps)
    hist, sums = point_error_counts(pred, gt, vis, thr)
    return pck_measures(hist.cpu().numpy(), sums.cpu().numpy(), thr)


def fscore(pred, gt, thresholds=(0.005, 0.015)):
    """The benchmark's calculate_fscore for every sample and threshold: pred [B,Np,3], gt [B,Ng,3] -> (F, precision, recall), float64
    [B,T] on the device.  precision = share of predicted points whose nearest ground-truth point is closer than the threshold (strictly),
    recall = the same from ground truth to prediction, F = 2 P R / (P + R), 0 where P + R = 0."""
    require_cuda(pred, gt)
    pred, gt = pred.float().contiguous(), gt.float().contiguous()
    assert pred.dim() == 3 and gt.dim() == 3 and pred.shape[0] == gt.shape[0] and pred.shape[2] == 3 and gt.shape[2] == 3, (pred.shape, gt.shape)
    counts = torch.empty(pred.shape[0], 2, len(thresholds), dtype=torch.int32, device=pred.device)
    get_lib().fscore_counts(pred, gt, thresholds, counts)
    return fscore_from_counts(counts, pred.shape[1], gt.shape[1])


def fscore_from_counts(counts, Np, Ng):
    P, R = counts[:, 0].double() / Np, counts[:, 1].double() / Ng
    S = P + R
    return torch.where(S > 0, 2 * P * R / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S)), P, R


def chamfer(pred, gt):
    """float64 [B, 2] on the device: per sample the MEAN squared distance to the nearest point of the other set, (pred -> gt, gt -> pred), in
    the inputs' unit squared.  pred [B, Np, 3], gt [B, Ng, 3], any Np, Ng.  Their sum is the Chamfer distance of the loss term `chamfer`
    at unit weights (ops.chamfer_distance), sample by sample."""
    from . import ops
    require_cuda(pred, gt)
    assert pred.dim() == 3 and gt.dim() == 3 and pred.shape[0] == gt.shape[0] and pred.shape[2] == 3 and gt.shape[2] == 3, (pred.shape, gt.shape)
    return ops.chamfer_sums(pred, gt) / torch.tensor([pred.shape[1], gt.shape[1]], dtype=torch.float64, device=pred.device)


def point_to_surface(pred_verts, faces, gt_points):
    """float64 [B] on the device: per sample the MEAN squared distance from the ground-truth points gt_points [B, N, 3] to the closest
    triangle of the predicted mesh (pred_verts [B, V, 3], faces [F, 3] int tensor on the device), in the inputs' unit squared.  Only that
    direction is searched.  It is the points -> faces half of the loss term `point_mesh` (ops.point_mesh_distance), sample by sample, and
    exactly 0 where the points lie on the surface."""
    from . import ops
    require_cuda(pred_verts, gt_points, faces)
    assert pred_verts.dim() == 3 and gt_points.dim() == 3 and pred_verts.shape[0] == gt_points.shape[0], (pred_verts.shape, gt_points.shape)
    return ops.point_mesh_sums(gt_points, pred_verts, faces, 1.0, 0.0)[:, 0] / float(gt_points.shape[1])


def depth_error(pred_depth, hits, gt_depth, mask=None):
    """A float64 scalar on the device: the mean |pred_depth - gt_depth| over the valid pixels of the batch, in the inputs' unit -- a pixel is
    valid where the mesh covers it (hits > 0), the depth image measures (gt_depth > 0) and the mask (None: everywhere) is not 0.
    pred_depth [B, 1, H, W] and hits [B, H, W] from ops.render_depth, gt_depth [B, H, W].  It is the loss term `depth` at lambda = 1 and
    trunc = 0 (ops.depth_loss, the same kernel); 0 when no pixel is valid."""
    from . import ops
    s = ops.depth_loss_sums(pred_depth, hits, gt_depth, mask).sum(0)
    return s[0] / s[1].clamp(min=1.0)


class Evaluator:
    """Accumulates what the evaluation loop keeps (train_hrnet.py:119-161) and reduces it as :216-272 does."""

    def __init__(self, ssim_fn=None, lpips_fn=None, benchmark=False, chamfer=False, point_mesh=False, faces=None, depth=False):
        self.xyz_pred, self.verts_pred, self.texture = [], [], []
        self.depth, self.depth_sums = bool(depth), []      # summary() adds 'depth_mae' when the batches carried 're_depth' and 'depths'
        self.benchmark = bool(benchmark)          # summary() adds BENCHMARK_KEYS when ground truth is given
        self.chamfer = bool(chamfer)              # summary() adds CHAMFER_KEYS when verts_gt is given
        self.point_mesh = bool(point_mesh)        # summary() adds POINT_MESH_KEYS when verts_gt is given
        self.faces = faces                        # the predicted mesh's faces [F, 3] on the device; else outputs['_faces_i32'] of `collect`
        if ssim_fn is None:
            from . import ops
            ssim_fn = ops.ssim
        self.ssim_fn, self.lpips_fn = ssim_fn, lpips_fn

    def collect(self, outputs, examples, dat_name, render=True):
        joints = outputs["joints"].detach()
        if dat_name == "HO3D":           # back to the HO-3D joint order and OpenGL axes for the challenge dump (:128-132)
            joints = Frei2HO3D(joints) * torch.tensor([1.0, -1.0, -1.0], device=joints.device).view(1, 1, 3)
        self.xyz_pred.append(joints)
        self.verts_pred.append(outputs["mano_verts"].detach())
        if self.point_mesh and self.faces is None:
            self.faces = outputs.get("_faces_i32")
        if self.depth and render:
            if "re_depth" not in outputs or examples.get("depths") is None:
                raise ValueError("Evaluator(depth=True) needs outputs['re_depth'] (Model(..., render_depth=True)) and examples['depths']")
            from . import ops
            self.depth_sums.append(ops.depth_loss_sums(outputs["re_depth"], outputs["_re_depth_hits"], examples["depths"],
                                                       examples.get("segms_gt")))          # [B, 2] on the device
        if render and "re_img" in outputs:
            if dat_name == "HO3D":
                m = (outputs["re_sil"] > 0).float()
                mask_rgbs, mask_re = examples["imgs"] * m, outputs["re_img"] * m
            else:
                m = examples["segms_gt"].unsqueeze(1).float()
                mask_rgbs, mask_re = m * examples["imgs"], outputs["re_img"] * m
            mse = F.mse_loss(mask_re, mask_rgbs)
            rec = {"psnr": -10 * mse.log10(), "ssim": self.ssim_fn(mask_re.contiguous(), mask_rgbs.contiguous()),
                   "l1": F.l1_loss(mask_re, mask_rgbs), "l2": mse}
            if self.lpips_fn is not None:
                rec["lpips"] = self.lpips_fn(mask_re * 2 - 1, mask_rgbs * 2 - 1).mean()
            self.texture.append(rec)              # device scalars: one host sync at `summary`, not one per batch

    def dump(self, pred_out_path):
        """utils/train_utils.py:242-254: `[xyz_pred_list, verts_pred_list]` as JSON -- the file the HO-3D challenge server takes
        (train_hrnet.py:277-293; HO-3D joints were already put back into the HO-3D order / OpenGL axes by `collect`) and the
        reference's `pred.json` for FreiHAND."""
        import json
        import os
        xyz = torch.cat(self.xyz_pred).cpu().tolist() if self.xyz_pred else []
        verts = torch.cat(self.verts_pred).cpu().tolist() if self.verts_pred else []
        os.makedirs(os.path.dirname(os.path.abspath(pred_out_path)), exist_ok=True)
        with open(pred_out_path, "w") as fo:
            json.dump([xyz, verts], fo)
        return len(xyz), len(verts)

    def summary(self, xyz_gt=None, verts_gt=None, root_id=None):
        """xyz_gt [n,21,3] / verts_gt [n,778,3]: evaluation_xyz.json / evaluation_verts.json.  Returns a dict with
        'pose_3d' / 'vert_3d' (MPJPE / MPVPE in the inputs' unit, metres in FreiHAND; the reference prints x100 = cm) and
        the batch-averaged texture metrics.  An Evaluator(benchmark=True) adds BENCHMARK_KEYS for the ground truth it is given (the
        FreiHAND benchmark's scores.txt names: *_mean3d in the inputs' unit, *_auc3d over 0..0.05 in 100 steps, F at 0.005 / 0.015); the
        `_al_` forms are taken on the fp32 output of align_w_scale.  root_id: the ground truth is made relative to its joint `root_id`
        before the un-aligned forms (the predictions are root-relative already); None takes it as given.  An Evaluator(chamfer=True)
        adds CHAMFER_KEYS when verts_gt is given: the two directions of `chamfer` summed, averaged over the samples, in the inputs' unit
        SQUARED; taken on the same two pairs of point sets as the F-scores.  An Evaluator(point_mesh=True) adds POINT_MESH_KEYS the same
        way: the mean squared distance from the ground-truth vertices to the predicted SURFACE (point_to_surface), averaged over the
        samples, un-aligned and aligned.  An Evaluator(depth=True) adds 'depth_mae': the mean |re_depth - depths| over the valid pixels
        of every collected batch (depth_error's definition with the mask segms_gt), in the inputs' unit."""
        out, bench = {}, []
        mesh_extra = self.chamfer or self.point_mesh
        if self.point_mesh and verts_gt is not None and self.faces is None:
            raise ValueError("Evaluator(point_mesh=True) needs the predicted mesh's faces: faces=, or outputs['_faces_i32'] at collect")
        dev = lambda a, like: torch.as_tensor(a, dtype=torch.float32).to(like.device)
        root = None
        if (self.benchmark or mesh_extra) and root_id is not None and (xyz_gt is not None or verts_gt is not None):
            if xyz_gt is None:
                raise ValueError("root_id needs xyz_gt: the root is a ground-truth joint")
            root = dev(xyz_gt, (self.xyz_pred or self.verts_pred)[0])[:, int(root_id):int(root_id) + 1]
        for name, gt, preds in (("xyz", xyz_gt, self.xyz_pred), ("mesh", verts_gt, self.verts_pred)):
            if gt is None:
                continue
            pred = torch.cat(preds)
            gt = dev(gt, pred)
            if self.benchmark or (mesh_extra and name == "mesh"):
                aligned, err = align_w_scale(gt, pred, return_error=True)           # the same err bits as aligned_error
                bench.append((name, pred, gt if root is None else gt - root, aligned, gt))
            else:
                err = aligned_error(pred, gt)
            out["pose_3d" if name == "xyz" else "vert_3d"] = float(err.mean())
        if bench:
            out.update(self._benchmark_summary(bench, benchmark=self.benchmark, with_chamfer=self.chamfer,
                                               p2s_faces=self.faces if self.point_mesh else None))
        if self.texture:
            for k in self.texture[0]:
                out[k] = float(torch.stack([r[k] for r in self.texture]).mean())
            out.setdefault("lpips", None)
        if self.depth and self.depth_sums:
            s = torch.cat(self.depth_sums).sum(0).tolist()
            out["depth_mae"] = s[0] / max(s[1], 1.0)
        return out

    @staticmethod
    def _benchmark_summary(bench, benchmark=True, with_chamfer=False, p2s_faces=None):
        """bench: (name, pred, gt for the un-aligned forms, aligned pred, gt) per point set.  Everything is counted on the device and
        comes to the host in ONE copy; the curves are host float64.  benchmark: BENCHMARK_KEYS; with_chamfer: CHAMFER_KEYS; p2s_faces
        (the predicted mesh's faces): POINT_MESH_KEYS."""
        thr = np.linspace(0.0, 0.05, 100)
        parts, plan = [], []
        for name, pred, gt_rel, aligned, gt in bench:
            for tag, p, g in ((name, pred, gt_rel), (name + "_al", aligned, gt)):
                if benchmark:
                    hist, sums = point_error_counts(p, g, None, thr)
                    parts += [hist.double().reshape(-1), sums]
                    plan.append(("pck", tag, hist.shape))
                if benchmark and name == "mesh":
                    parts.append(fscore(p, g, (0.005, 0.015))[0].mean(0))
                    plan.append(("f", "f_al_score_" if tag.endswith("_al") else "f_score_", None))
                if with_chamfer and name == "mesh":
                    parts.append(chamfer(p, g).sum(1).mean(0, keepdim=True))
                    plan.append(("chamfer", tag + "_chamfer", None))
                if p2s_faces is not None and name == "mesh":
                    parts.append(point_to_surface(p, p2s_faces, g).mean(0, keepdim=True))
                    plan.append(("chamfer", tag + "_p2s", None))
        flat, at, out = torch.cat(parts).cpu().numpy(), 0, {}
        for kind, tag, shape in plan:
            if kind == "pck":
                K, W = shape
                m = pck_measures(np.rint(flat[at:at + K * W]).astype(np.int64).reshape(K, W), flat[at + K * W:at + K * W + K], thr)
                out[tag + "_mean3d"], out[tag + "_auc3d"] = m["mean"], m["auc"]
                at += K * W + K
            elif kind == "chamfer":
                out[tag] = float(flat[at])
                at += 1
            else:
                out[tag + "5"], out[tag + "15"] = float(flat[at]), float(flat[at + 1])
                at += 2
        return {k: out[k] for k in BENCHMARK_KEYS + CHAMFER_KEYS + POINT_MESH_KEYS if k in out}
