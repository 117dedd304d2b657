"""Config surface of the hot path: the argparse defaults the reference's step reads
(reference options/train_options.py:4-201) plus the JSON overlay and lambda-list handling of
reference train_hrnet.py:503-519.  Only keys that select or weight the hot path are kept."""
from __future__ import annotations

import argparse
import json

_DEFAULTS = dict(
    new_model=True, render=True, light_estimation=True, four_channel=False, hand_model="mano", pretrain="res18",
    use_mean_shape=False, base_loss_fn="L1", losses=["joint_3d", "vert_3d", "mpose", "mshape", "edge_length", "sil",
                                                      "texture", "mrgb", "ssim_tex"],
    train_batch=32, val_batch=16, num_workers=8, init_lr=0.001, force_init_lr=-1, lr_steps=[50], lr_gamma=0.001,
    optimizer="Adam", total_epochs=100, semi_ratio=None,
    lambda_texture=0.003, lambda_silhouette=0.005, lambda_j2d_gt_list=[0.00001], lambda_j2d_gt_steps=[],
    lambda_j3d=100.0, lambda_vert_3d=100.0, lambda_shape_list=[0.00001], lambda_shape_steps=[],
    lambda_pose_list=[0.0001], lambda_pose_steps=[], lambda_tex_reg_list=[0.00001], lambda_tex_reg_steps=[],
    lambda_mrgb=1e-3, lambda_iou=1e-3, lambda_bone_direc=0.1, lambda_bone_direc_3d=0.1, lambda_edge_len=0.1,
    lambda_percep=1e-5, lambda_ssim_tex=0.001, lambda_scale=100.0, lambda_mscale=0.1, lambda_laplacian=0.1,
    ROOT=9, ROOT_NIMBLE=11,
    lpips_weights=None,    # [path, ...]: AlexNet + lin weights for the evaluation pass's LPIPS and the loss term "lpips" (hifihr_amd/lpips.py); None = LPIPS not reported (the loss term: seeded weights)
    benchmark_metrics=True,    # the evaluation pass also reports the FreiHAND benchmark's PCK / AUC and F-score keys (hifihr_amd/evaluate.py)
    # opt-in differentiable silhouette (hifihr_amd/ops.py soft_silhouette; the loss names "sil_soft" / "iou_soft" switch it on as well).
    # The two weights are the defaults of their hard counterparts lambda_silhouette / lambda_iou: starting points, not tuned values
    soft_silhouette=False, soft_sil_sigma=1e-4, lambda_silhouette_soft=0.005, lambda_iou_soft=1e-3,
    # opt-in gradient guard of the fused Adam step (hifihr_amd/optim.py FusedAdam(max_grad_norm=...)): the global L2 norm the gradient is
    # clipped to, and a step whose gradient holds a NaN / inf is skipped.  0 = off; inf = the skip alone
    max_grad_norm=0.0,
    # weight of the opt-in term "normal_consistency" (hifihr_amd/ops.py mesh_regularizers; "triangle" reads the reference's
    # lambda_laplacian above): the weight of PyTorch3D's mesh-fitting tutorial [recalled] -- a starting point, not a tuned value
    lambda_normal_consistency=0.01,
    # weight of the opt-in term "lpips" (hifihr_amd/losses.py: LPIPS(alex) of the composite against the image, hifihr_amd/lpips.py with
    # differentiable=True; it reads lpips_weights above): the order of lambda_texture -- a starting point, not a tuned value
    lambda_lpips=0.01,
    # weight of the opt-in term "chamfer" (hifihr_amd/ops.py chamfer_distance): the weight of PyTorch3D's mesh-fitting tutorial [recalled]
    # -- a starting point, not a tuned value.  The term is in SQUARED metres (1 cm off is 1e-4), so a real run will need it much larger
    lambda_chamfer=1.0,
    # weights of the opt-in term "point_mesh" (hifihr_amd/ops.py point_mesh_distance): target points -> the predicted surface, and predicted
    # faces -> the target points.  Starting points, not tuned values; the term is in SQUARED metres like "chamfer".  The second is 0, which
    # also skips its search: against a sparse target that direction's minimum is not zero, the very problem the term exists to avoid
    lambda_point_mesh=1.0,
    lambda_point_mesh_faces=0.0,
    # opt-in depth map of the hard render and its loss term "depth" (hifihr_amd/ops.py render_depth / depth_loss; the loss name switches the
    # option on as well).  lambda_depth is the reference option's own default (it declares the weight and never computes the term): a starting
    # point, not a tuned value; the term is in metres.  depth_trunc (metres; 0 = off): pixels further than this from the depth image are left
    # out -- a few centimetres for HO-3D, where the object occludes the hand
    render_depth=False, lambda_depth=1.0, depth_trunc=0.0,
    depth_metric=False,   # the evaluation pass also reports depth_mae (hifihr_amd/evaluate.py Evaluator(depth=True)); needs render_depth and batches with 'depths'
    point_mesh_metric=False,   # the evaluation pass also reports mesh_p2s / mesh_al_p2s (hifihr_amd/evaluate.py Evaluator(point_mesh=True))
    # weights of the self-supervised keypoint terms "open_2dj" and "open_2dj_de" (hifihr_amd/ops.py open2d_terms; "open_bone_direc" reads
    # lambda_bone_direc above): the reference's argparse defaults (options/train_options.py:108, 112), untuned here.  semi_ratio above: the share
    # of the training set whose detections data_dic / FreiHandDeviceCache replace with the ground-truth projection
    lambda_j2d=1e-3, lambda_j2d_de=1e-4,
    # test-time refinement of the evaluation pass (hifihr_amd/fit.py; one launch per batch, csrc/mano_fit.hip): off by default.  fit_target names
    # the batch's keypoints to fit to ('open_2dj' with its confidences, or 'j2d_gt' at confidence 1); the six weights multiply the 2-D, bone
    # direction, 3-D, pose-prior, shape and pose-coefficient terms of include/hifihr.h: starting points, not tuned values
    fit_keypoints=False, fit_iters=151, fit_target="open_2dj",
    fit_w_2d=1.0, fit_w_bone=1.0, fit_w_3d=0.0, fit_w_prior=1.0, fit_w_shape=0.1, fit_w_pca=0.01,
    chamfer_metric=False,    # the evaluation pass also reports mesh_chamfer / mesh_al_chamfer (hifihr_amd/evaluate.py Evaluator(chamfer=True))
    # P > 0: traineval.data_dic builds examples['chamfer_points'] [B,P,3], the target of "chamfer" / "point_mesh", from examples['depths']
    # (hifihr_amd/ops.py depth_points: P draws with replacement among the depth pixels under the hand mask, back-projected, root-relative).
    # The reference's batch_depth2pc draws 1000.  0: off; a caller's own chamfer_points always wins
    depth_points=0,
)

# lambda values of reference config/FreiHAND/full_rhd_freihand.json, used by the
# BASELINE config-2 composition (res18 + MANO + render) defined in SURVEY.md section 8(d)
FREIHAND_FULL_LAMBDAS = dict(
    lambda_j3d=200, lambda_vert_3d=150, lambda_edge_len=100, lambda_silhouette=0.0008,
    lambda_tex_reg_steps=[260, 270], lambda_tex_reg_list=[5e-3, 5e-5, 5e-7], lambda_pose_steps=[10, 20],
    lambda_pose_list=[0.01, 0.001, 0.00001], lambda_shape_steps=[270, 300], lambda_shape_list=[0.1, 0.001, 0.00001],
    lambda_percep=1e-8, lambda_mrgb=2e-3, lambda_ssim_tex=0.01, lambda_texture=0.02, lambda_bone_direc_3d=6,
    init_lr=0.001, force_init_lr=0.000001, lr_steps=[80, 160, 200, 300, 350, 400, 450], lr_gamma=0.5,
)


def finalize(args):
    """train_hrnet.py:516-519: lambda_* <- first element of *_list."""
    args.lambda_pose = args.lambda_pose_list[0]
    args.lambda_j2d_gt = args.lambda_j2d_gt_list[0]
    args.lambda_shape = args.lambda_shape_list[0]
    args.lambda_tex_reg = args.lambda_tex_reg_list[0]
    return args


def update_lambdas_for_epoch(args, epoch):
    """train_hrnet.py:454-465: step schedules of lambda_pose / _j2d_gt / _shape / _tex_reg."""
    for name in ("pose", "j2d_gt", "shape", "tex_reg"):
        steps, vals = getattr(args, f"lambda_{name}_steps"), getattr(args, f"lambda_{name}_list")
        idx = sum(1 for s in steps if epoch >= s)
        setattr(args, f"lambda_{name}", vals[min(idx, len(vals) - 1)])
    return args


def make_args(config_json: str | None = None, **overrides) -> argparse.Namespace:
    args = argparse.Namespace(**{k: (list(v) if isinstance(v, list) else v) for k, v in _DEFAULTS.items()})
    if config_json:
        with open(config_json) as fh:
            for k, v in json.load(fh).items():          # unknown keys accepted silently, like train_hrnet.py:505-510
                setattr(args, k, v)
    for k, v in overrides.items():
        setattr(args, k, v)
    return finalize(args)


def baseline_config2_args(**overrides):
    """BASELINE.json configs[1]: FreiHAND batch=32, ResNet-18 + MANO LBS + silhouette/texture losses."""
    kw = dict(FREIHAND_FULL_LAMBDAS)
    kw.update(overrides)
    return make_args(None, **kw)


# reference config/FreiHAND/full_rhd_freihand.json ("losses", "train_batch", "pretrain"; hand_model is "nimble" there)
FREIHAND_FULL_LOSSES = ["joint_3d", "vert_3d", "mpose", "mshape", "mtex", "bone_direc_3d", "edge_length",
                        "texture", "mrgb", "sil", "ssim_tex", "perceptual"]


def baseline_config3_args(**overrides):
    """BASELINE.json configs[2]: full_rhd_freihand.json -- EfficientNet-b3, batch 48, texture + perceptual losses.  The
    NIMBLE layer is not available: the composition runs with MANO + the texture stand-in of models.Model
    and a VGG19 carrying seeded random weights."""
    kw = dict(FREIHAND_FULL_LAMBDAS)
    kw.update(pretrain="effb3", train_batch=48, losses=list(FREIHAND_FULL_LOSSES), hand_model="mano")
    kw.update(overrides)
    return make_args(None, **kw)


# reference config/HO3D/weak_rhd_ho3d.json
HO3D_WEAK_LAMBDAS = dict(
    lambda_j3d=200, lambda_vert_3d=200, lambda_edge_len=100, lambda_silhouette=0.00001, lambda_iou=0.0008,
    lambda_tex_reg_steps=[260, 270], lambda_tex_reg_list=[5e-3, 5e-5, 5e-7], lambda_pose_steps=[260, 270, 280],
    lambda_pose_list=[0.01, 0.001, 0.0001, 0.00001], lambda_shape_steps=[270, 300], lambda_shape_list=[0.1, 0.001, 0.00001],
    lambda_j2d_gt_list=[0.01], lambda_bone_direc=0.1, lambda_percep=1e-8, lambda_ssim_tex=0.002, lambda_texture=0.01,
    init_lr=0.001, lr_steps=[80, 160, 200, 300, 350, 400, 450], lr_gamma=0.5,
)
HO3D_WEAK_LOSSES = ["joint_2d", "bone_direc", "mpose", "mshape", "mtex", "texture", "mrgb", "sil", "ssim_tex", "perceptual"]


def baseline_config5_args(**overrides):
    """BASELINE.json configs[4]: HO-3D weak supervision (2-D joints + photometric terms), 16 images per GPU.  Same
    stand-ins as `baseline_config3_args`; dat_name is "HO3D" (no scale term, absolute ground truth, OpenGL-convention
    intrinsics flipped by data_dic)."""
    kw = dict(HO3D_WEAK_LAMBDAS)
    kw.update(pretrain="effb3", train_batch=16, losses=list(HO3D_WEAK_LOSSES), hand_model="mano")
    kw.update(overrides)
    return make_args(None, **kw)
