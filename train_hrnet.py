#!/usr/bin/env python3
"""Training / evaluation front-end with the reference's command line:  python train_hrnet.py --config_json <file>.json

Mirrors the flow of the reference's train_hrnet.py (argument overlay :503-519, model / optimizer / scheduler / checkpoint
set-up :537-566, epoch driver :449-485 with the lambda schedules, periodic test + save, evaluation mode :487-496) on this
package's device-resident pieces:

  data        hifihr_amd.data.FreiHandDeviceCache -- the decoded set lives in HBM, a batch is one gather-and-warp launch.
              Source: --freihand_cache <npz with images u8 [n,224,224,3], masks u8, Ks, joints, verts> (pre-decoded by the user;
              JPEG decoding is outside the hot path) or, by default, a seeded synthetic FreiHAND-shaped set (--synthetic_size).
              --dataset HO3D: hifihr_amd.data.HO3DDeviceCache -- 480 x 640 frames in HBM, the reference's hand crop (window from the
              projected joints, Pillow-exact crop + resize to 224) on the device; --ho3d_cache <npz> or seeded synthetic frames.  The epoch
              driver's periodic test and the evaluation mode write the challenge dump `<base_out_path>/json/test/<epoch>/pred.json` from the
              evaluation split (--ho3d_eval_cache <npz>: hand boxes + root joints; reference train_hrnet.py:124-136, 286-293).
              Either npz may also carry open_2dj / open_2dj_con (2-D detections) and depth_u16 (16-bit depth frames): the cache then feeds
              the self-supervised keypoint terms, fit_keypoints, the term `depth` / depth_mae and, with the option depth_points, the
              `chamfer_points` of `chamfer` / `point_mesh`; the synthetic frames carry them when something asks for them.
  step        hifihr_amd.traineval.GraphedTrainStep (hipGraph replay) or the eager step (--graph 0)
  multi-GPU   one process per GPU under torch.distributed.run; rank r takes every world-th batch slice; RCCL all-reduce of the
              flat gradient buffer (hifihr_amd/dist.py).  Replaces nn.DataParallel (:560).
  checkpoints the reference's .t7 layout (hifihr_amd/checkpoint.py); --pretrain_model resumes a reference file.

hand_model "nimble" configs run with MANO + the texture stand-in (hifihr_amd/models.py) and say so: the NIMBLE submodule
and its assets are not part of the reference tree.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config_json", default=None)
    ap.add_argument("--freihand_cache", default=None, help="npz: images, masks, Ks, joints, verts [, eval_* counterparts]")
    ap.add_argument("--dataset", default="FreiHand", choices=["FreiHand", "HO3D"],
                    help="HO3D: train on 480 x 640 frames through hifihr_amd.data.HO3DDeviceCache (the reference's hand crop on the device)")
    ap.add_argument("--ho3d_eval_cache", default=None, help="npz of the HO-3D EVALUATION split: images u8 [n,480,640,3], Ks [n,3,3], bboxes "
                    "[n,2,2] ((x0, y0), (x1, y1)), root_xyz [n,3] (the split has a hand box and the root joint, no 21 joints: dataset.py:1071-1080); "
                    "without it the evaluation pass runs on the training frames with boxes / roots derived from their joints")
    ap.add_argument("--ho3d_cache", default=None, help="npz: images u8 [n,480,640,3], hand_masks u8 [n,480,640], Ks [n,3,3] (camMat . cam_extr), "
                                                       "xyz21 [n,21,3]; optional: open_2dj [n,21,2] + open_2dj_con (2-D detections) and depth_u16 "
                                                       "[n,480,640] (hifihr_amd.data.ho3d_depth_to_u16); default: seeded synthetic frames, "
                                                       "which carry both when a requested loss, metric or fit_keypoints needs them")
    ap.add_argument("--openpose_keypoints", default=None, metavar="JSON",
                    help="2-D detections for the self-supervised terms 'open_2dj' / 'open_bone_direc' / 'open_2dj_de' and the `*_self` photometric "
                         "terms, in the reference's layout (data/dataset.py:1430-1432): [keypoints [n][21][2], confidences [n][21] or [n][21][1]], "
                         "in pixels of the cached images, one row per training sample.  The --freihand_cache npz may carry them itself as "
                         "open_2dj / open_2dj_con; the synthetic set makes seeded ones when a requested loss needs them")
    ap.add_argument("--synthetic_size", type=int, default=512)
    ap.add_argument("--mano_pkl", default=None, help="MANO_RIGHT.pkl (licensed, user supplied); default: synthetic MANO-shaped tables")
    ap.add_argument("--nimble_layer", choices=["mano-stand-in", "synthetic", "synthetic-uv"], default="mano-stand-in",
                    help="what hand_model 'nimble' runs on: MANO + the vertex-colour texture stand-in, or the NIMBLE-shaped layer "
                         "(csrc/lbs.hip: 25 joints, 5990 skin vertices, texture PCA) on seeded synthetic tables; synthetic-uv: the same "
                         "layer with a texture IMAGE sampled through per-face uvs (TexturesUV, hifihr_render_fwd_uv)")
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--max_iters", type=int, default=0, help="stop after this many iterations (0 = run the epochs)")
    ap.add_argument("--print_freq", type=int, default=50)
    ap.add_argument("--dist_timeout_min", type=float, default=60.0, help="collective timeout of the process group: has to cover rank 0's "
                    "evaluation pass, during which the other ranks wait in a barrier")
    ap.add_argument("--lpips_weights", nargs="+", default=None, metavar="PATH",
                    help="report LPIPS(net='alex') beside PSNR / SSIM in the evaluation pass (reference train_hrnet.py:158,563): one or two torch "
                         "files -- torchvision's alexnet state dict and the lpips package's alex.pth, or the package's full LPIPS state dict "
                         "(hifihr_amd/lpips.py: load_state_dict_lpips).  Without it LPIPS is not reported.  The opt-in loss term 'lpips' "
                         "(options: lambda_lpips) reads the same files; without them it trains on seeded weights and warns.")
    ap.add_argument("--soft_silhouette", action="store_true",
                    help="the model also emits outputs['re_sil_soft'], a differentiable silhouette (options: soft_silhouette, soft_sil_sigma); "
                         "the loss names 'sil_soft' / 'iou_soft' switch it on by themselves")
    ap.add_argument("--render_depth", action="store_true",
                    help="the model also emits outputs['re_depth'], the depth map of its hard render with a backward pass to the vertices "
                         "(options: render_depth, lambda_depth, depth_trunc); the loss name 'depth' switches it on by itself, and the "
                         "FreiHAND batches then carry the ground-truth mesh's depth map as 'depths'")
    ap.add_argument("--fit_keypoints", action="store_true",
                    help="the evaluation pass refines every MANO prediction against the batch's 2-D keypoints before it is scored (options: "
                         "fit_keypoints, fit_iters, fit_target 'open_2dj' | 'j2d_gt', fit_w_*): the whole fit is one launch per batch "
                         "(hifihr_amd/fit.py); rendered images and texture metrics stay the network's")
    ap.add_argument("--max_grad_norm", type=float, default=None, metavar="X",
                    help="gradient guard of the optimizer step (options: max_grad_norm): clip the global L2 norm of the gradient to X and skip a "
                         "step whose gradient holds a NaN / inf, all on the device; 'inf' = the skip alone, 0 = off (the default)")
    ap.add_argument("--override", default=None, help='JSON object of option overrides, e.g. \'{"total_epochs": 2}\'')
    return ap.parse_args(argv)


def soft_silhouette_kwargs(args):
    """Model(...)'s soft-silhouette options: on when asked for, or when a loss term that reads outputs['re_sil_soft'] is requested."""
    on = bool(getattr(args, "soft_silhouette", False)) or any(k in args.losses for k in ("sil_soft", "iou_soft"))
    return dict(soft_silhouette=on, soft_sil_sigma=float(getattr(args, "soft_sil_sigma", 1e-4)))


def render_depth_kwargs(args):
    """Model(...)'s depth-map option: on when asked for, or when the loss term or the metric that reads outputs['re_depth'] is requested."""
    return dict(render_depth=bool(getattr(args, "render_depth", False)) or "depth" in args.losses or bool(getattr(args, "depth_metric", False)))


def wants_depths(args):
    """The batches need examples['depths']: the loss term 'depth' or the metric depth_mae is requested."""
    return "depth" in args.losses or bool(getattr(args, "depth_metric", False))


def wants_depth_points(args):
    """The batches need examples['chamfer_points'] made from examples['depths'] (the option depth_points > 0 with a term that reads them)."""
    return int(getattr(args, "depth_points", 0) or 0) > 0 and any(k in args.losses for k in ("chamfer", "point_mesh"))


def attach_mesh_depths(ex, model, static=None):
    """examples['depths'] for a FreiHAND batch: that data path carries no depth image, so the depth map of the batch's ground-truth mesh
    (hifihr_amd/synth.py mesh_depths: its augmented vertices through its own camera) stands in for one.  static: the captured step's
    inputs -- the map is written into the tensor the graph reads."""
    from hifihr_amd import synth
    cam = ex["cam_ndc"] if "cam_ndc" in ex else model.camera_from_K(ex["Ks"])
    out = static["depths"] if static is not None and "depths" in static else None
    ex["depths"] = synth.mesh_depths(depth_renderer(model), ex["verts"], cam, out=out)
    return ex


KEYPOINT_LOSSES = ("open_2dj", "open_bone_direc", "open_2dj_de", "texture_self", "mrgb_self", "ssim_tex_self")


def wants_keypoints(args):
    """A requested loss reads the 2-D detections or the texture_con made from their confidences."""
    return any(k in args.losses for k in KEYPOINT_LOSSES)


def fit_wants_detections(args):
    """The evaluation pass refines its predictions against the 2-D detections (fit_keypoints with fit_target 'open_2dj'): the arrays the
    pass runs on have to carry them."""
    return bool(getattr(args, "fit_keypoints", False)) and getattr(args, "fit_target", "open_2dj") == "open_2dj"


def load_openpose_keypoints(path, n):
    """The reference's detection file (data/dataset.py:1430-1432: json [keypoints, confidences]) -> (open_2dj f32 [n,21,2], open_2dj_con f32
    [n,21,1]) for the first n samples."""
    with open(path) as fh:
        both = json.load(fh)
    if not (isinstance(both, list) and len(both) == 2):
        raise ValueError(f"{path}: expected the list [keypoints, confidences]")
    det, con = np.asarray(both[0], dtype=np.float32), np.asarray(both[1], dtype=np.float32)
    if det.ndim != 3 or det.shape[1:] != (21, 2) or det.shape[0] < n or con.shape[0] != det.shape[0] or con.size != det.shape[0] * 21:
        raise ValueError(f"{path}: keypoints {det.shape} / confidences {con.shape} do not cover {n} samples of 21 joints")
    return det[:n], con.reshape(-1, 21, 1)[:n]


def optimizer_max_grad_norm(args):
    """FusedAdam's max_grad_norm from the options: 0 (or a missing key) is off."""
    x = float(getattr(args, "max_grad_norm", 0.0) or 0.0)
    return x if x != 0.0 else None


def grad_guard_log(stats):
    """What the training loops append to their log line: FusedAdam.grad_stats() (None: the guard is off)."""
    if stats is None:
        return ""
    return f" gnorm={stats['norm']:.3e} clipped={stats['clipped']}/{stats['steps']} skipped={stats['skipped']}"


def build_args(cli):
    from hifihr_amd import options
    over = json.loads(cli.override) if cli.override else {}
    defaults = dict(mode=["training"], save_interval=10, if_test=True, save_mode="only_latest", pretrain_model=None,
                    base_out_path="outputs/run", val_batch=16)
    defaults.update(over)
    args = options.make_args(cli.config_json, **{k: v for k, v in defaults.items() if cli.config_json is None or k in over})
    for k, v in defaults.items():                      # keys a JSON may leave out
        if not hasattr(args, k):
            setattr(args, k, v)
    args.state_output = os.path.join(args.base_out_path, "model")       # options/train_options.py:208-220
    args.pred_output = os.path.join(args.base_out_path, "json")         # :214 (the pred.json dumps)
    args.texture_stand_in = 0
    if getattr(cli, "soft_silhouette", False):
        args.soft_silhouette = True
    if getattr(cli, "render_depth", False):
        args.render_depth = True
    if getattr(cli, "max_grad_norm", None) is not None:
        args.max_grad_norm = float(cli.max_grad_norm)
    if getattr(cli, "fit_keypoints", False):
        args.fit_keypoints = True
    if cli.lpips_weights:
        args.lpips_weights = list(cli.lpips_weights)
    elif isinstance(getattr(args, "lpips_weights", None), str):        # a JSON may name one file
        args.lpips_weights = [args.lpips_weights]
    if args.hand_model == "nimble" and cli.nimble_layer in ("synthetic", "synthetic-uv"):
        print("[train_hrnet] hand_model 'nimble': NIMBLE-shaped layer on seeded synthetic tables (hifihr_amd/nimble_tables.py); the real "
              "NIMBLE assets are not available (SURVEY.md section 8 A9)")
    elif args.hand_model == "nimble":
        print("[train_hrnet] hand_model 'nimble': the NIMBLE layer is not available; running MANO + the 10-component "
              "vertex-colour texture stand-in (SURVEY.md section 8 A9)")
        args.hand_model, args.texture_stand_in = "mano", 10
    if isinstance(args.mode, str):
        args.mode = [args.mode]
    return args


def load_or_make_dataset(cli, model, device, keypoints=False, eval_keypoints=False):
    """-> (train arrays, eval arrays) as dicts of numpy arrays: images u8 [n,H,W,3], masks u8 [n,H,W], Ks, joints, verts.  The training
    arrays also hold open_2dj [n,21,2] / open_2dj_con when the npz or --openpose_keypoints carries them, or -- synthetic set, keypoints=True --
    seeded ones (synth.make_batch(open_2dj=True)).  eval_keypoints (the evaluation pass fits to detections): the eval arrays keep theirs too,
    the npz's eval_open_2dj / eval_open_2dj_con or the synthetic set's rows behind the cut; without it they are as before."""
    if cli.freihand_cache:
        z = np.load(cli.freihand_cache)
        tr = {k: z[k] for k in ("images", "masks", "Ks", "joints", "verts")}
        ev = {k: z["eval_" + k] for k in tr} if "eval_images" in z else None
        if ev is not None and eval_keypoints and "eval_open_2dj" in z and "eval_open_2dj_con" in z:
            ev["open_2dj"], ev["open_2dj_con"] = z["eval_open_2dj"], z["eval_open_2dj_con"]
        if "open_2dj" in z and "open_2dj_con" in z:
            tr["open_2dj"], tr["open_2dj_con"] = z["open_2dj"], z["open_2dj_con"]
        if getattr(cli, "openpose_keypoints", None):
            tr["open_2dj"], tr["open_2dj_con"] = load_openpose_keypoints(cli.openpose_keypoints, len(tr["images"]))
        return tr, ev
    from hifihr_amd import synth
    parts, n = [], cli.synthetic_size + 64
    if model.hand_model == "nimble":                  # the data side is MANO either way (FreiHAND's ground truth)
        from hifihr_amd import ops
        from hifihr_amd.mano_tables import synthetic_mano_tables
        mt = synthetic_mano_tables(0)
        mano, rend = ops.ManoLayerHandle(mt), ops.RendererHandle(mt.faces, 778, image_size=224, aa=3)
    else:
        mano, rend = model.hand_layer.handle, model.renderer_p3d
    for first in range(0, n, 64):
        s = synth.make_batch(mano, rend, min(64, n - first), first_index=first, device=device, images="render", open_2dj=keypoints)
        parts.append({"images": (s["trans_images"].permute(0, 2, 3, 1) * 255).round().to(torch.uint8).numpy(),
                      "masks": (s["trans_masks"][:, 0] * 255).to(torch.uint8).numpy(), "Ks": s["trans_Ks"].numpy(),
                      "joints": s["trans_joints"].numpy(), "verts": s["trans_verts"].numpy()})
        if keypoints:
            parts[-1].update(open_2dj=s["trans_open_2dj"].numpy(), open_2dj_con=s["open_2dj_con"].numpy())
    full = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    cut = cli.synthetic_size
    if getattr(cli, "openpose_keypoints", None):
        full["open_2dj"], full["open_2dj_con"] = load_openpose_keypoints(cli.openpose_keypoints, len(full["images"]))
    return {k: v[:cut] for k, v in full.items()}, {k: v[cut:] for k, v in full.items() if eval_keypoints or not k.startswith("open_2dj")}


def train_ho3d(cli, args, model, loss_func, opt, sched, reducer, current_epoch, rank, world, device, say):
    """The epoch driver on HO-3D frames (reference train_hrnet.py:449-485 with dat_name 'HO3D'): batches from HO3DDeviceCache through the
    HO3D branch of data_dic, copied into the captured step's static inputs."""
    from hifihr_amd import options, synth
    from hifihr_amd.checkpoint import save_model
    from hifihr_amd.data import HO3DDeviceCache
    from hifihr_amd.traineval import GraphedTrainStep, data_dic, train_step
    need_depth, need_det = wants_depths(args) or wants_depth_points(args), wants_keypoints(args) or fit_wants_detections(args)
    if cli.ho3d_cache:
        z = np.load(cli.ho3d_cache)
        frames = {"images_u8": z["images"], "hand_masks_u8": z["hand_masks"], "Ks": z["Ks"], "xyz21": z["xyz21"]}
        frames.update(ho3d_optional_arrays(z))
    else:
        from hifihr_amd import ops
        from hifihr_amd.mano_tables import synthetic_mano_tables
        mt = synthetic_mano_tables(0)
        frames = synth.make_ho3d_frames(ops.ManoLayerHandle(mt), ops.RendererHandle(mt.faces, 778, image_size=224, aa=3), cli.synthetic_size,
                                        device=device, images="render", depth=need_depth, open_2dj=need_det)
        frames.pop("depths", None)                        # (the float map the 16-bit frames were made from)
    training = "training" in args.mode
    if training and (wants_depths(args) or wants_depth_points(args)) and "depth_u16" not in frames:
        raise SystemExit("[train_hrnet] the loss term 'depth' / depth_metric / depth_points need HO-3D depth frames: give depth_u16 "
                         "(uint16 [n,480,640], hifihr_amd.data.ho3d_depth_to_u16 of the depth PNGs) in the --ho3d_cache npz")
    if training and wants_keypoints(args) and "open_2dj" not in frames:
        raise SystemExit(f"[train_hrnet] the losses {[k for k in args.losses if k in KEYPOINT_LOSSES]} need 2-D detections: give open_2dj / "
                         "open_2dj_con in the --ho3d_cache npz")
    cache = HO3DDeviceCache(**frames, device=device)
    say(f"[train_hrnet] HO3D: {cache.n} frames resident on {device}; world {world}; encoder {args.pretrain}; losses {args.losses}")
    eval_cache = ho3d_eval_cache(cli, frames, device) if rank == 0 else None
    if eval_cache is not None and fit_wants_detections(args) and eval_cache.open_2dj is None:
        raise SystemExit("[train_hrnet] fit_keypoints with fit_target 'open_2dj' needs 2-D detections for the HO-3D evaluation split: give "
                         "open_2dj / open_2dj_con in the --ho3d_eval_cache npz (or in --ho3d_cache when the split is derived from it), or "
                         "set fit_target to 'j2d_gt'")
    if "training" not in args.mode:                       # evaluation only (reference train_hrnet.py:487-496)
        if rank == 0:
            say("[train_hrnet] HO3D evaluation:", run_evaluation_ho3d(model, eval_cache, args, device, current_epoch))
        if world > 1:                                      # the other ranks leave together with rank 0, not while it still evaluates
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return 0
    B = args.train_batch
    gen = torch.Generator().manual_seed(1000 + current_epoch)
    noise_gen = torch.Generator().manual_seed(77 + rank)
    points_gen = torch.Generator().manual_seed(177 + rank)             # the draws of depth_points
    stepper, stepper_key, it, t_last = None, None, 0, time.perf_counter()
    for epoch in range(1, args.total_epochs + 1 - current_epoch):
        options.update_lambdas_for_epoch(args, epoch + current_epoch)
        lam_key = (args.lambda_pose, args.lambda_j2d_gt, args.lambda_shape, args.lambda_tex_reg)
        if stepper is not None and lam_key != stepper_key:
            stepper.release()
            stepper = None
        perm = torch.randperm(cache.n, generator=gen)
        per_step = B * world
        for lo in range(0, cache.n - per_step + 1, per_step):
            idx = perm[lo + rank * B: lo + (rank + 1) * B]
            ex = data_dic(cache.batch(idx, generator=noise_gen), "HO3D", "training", args, device=device, generator=points_gen)
            if cli.graph and stepper is None:
                ok = 1
                try:
                    stepper = GraphedTrainStep(model, loss_func, opt, ex, args, dat_name="HO3D", reducer=reducer if world > 1 else None)
                    stepper_key = lam_key
                except Exception as e:            # noqa: BLE001
                    # GraphedTrainStep's warm-up and capture are collective-free (round 3; the round-2 advisor found the bucket all-reduces
                    # of the old warm-up left the other ranks inside collectives a failing rank never joined), so a one-sided failure
                    # meets the other ranks in the flag all-reduce below and every rank falls back to the eager step together
                    print(f"[train_hrnet] rank {rank}: hipGraph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr, flush=True)
                    ok = 0
                if world > 1:
                    flag = torch.tensor([ok], device=device, dtype=torch.int32)
                    torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
                    ok = int(flag.item())
                if not ok:
                    if stepper is not None:
                        stepper.release()
                    stepper, cli.graph = None, 0
            if stepper is not None:
                stepper.load_batch(ex)
                loss, dic = stepper()
            else:
                loss, dic = train_step(model, loss_func, opt, ex, args, dat_name="HO3D", backward_hook=reducer.finish)
            it += 1
            if it % cli.print_freq == 0 or it == cli.max_iters:
                torch.cuda.synchronize()
                dt, t_last = time.perf_counter() - t_last, time.perf_counter()
                n_it = cli.print_freq if it % cli.print_freq == 0 else it % cli.print_freq
                terms = " ".join(f"{k}={float(dic[k].detach()):.4g}" for k in args.losses)
                say(f"[train_hrnet] epoch {epoch + current_epoch} it {it} loss {float(loss.detach()):.5f} ({terms}) {n_it * per_step / dt:.0f} img/s"
                    + grad_guard_log(opt.grad_stats()))
            if cli.max_iters and it >= cli.max_iters:
                break
        if (epoch + current_epoch) % args.save_interval == 0 or (cli.max_iters and it >= cli.max_iters):
            if rank == 0:
                say("[train_hrnet] saved", save_model(model, opt, sched, epoch, current_epoch, args))
                # the periodic test of the reference's epoch driver (:470-480): on HO-3D it is the challenge dump
                say("[train_hrnet] HO3D test:", run_evaluation_ho3d(model, eval_cache, args, device, epoch + current_epoch))
            if world > 1:
                # rank 0 alone walks the evaluation split: the others wait HERE, so that the evaluation is not booked as step time of the
                # next epoch.  This barrier is a collective like any other: it runs under the process group's timeout (`--dist_timeout_min`,
                # set at init_process_group), which therefore has to cover the longest evaluation pass.
                torch.distributed.barrier()
        sched.step()
        if cli.max_iters and it >= cli.max_iters:
            break
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    say("Done!")
    return 0


def ho3d_optional_arrays(z):
    """The optional keys of an HO-3D npz -> HO3DDeviceCache keywords: open_2dj [n,21,2] + open_2dj_con [n,21] or [n,21,1] (2-D detections,
    FreiHAND joint order, pixels of the stored frame) and depth_u16 [n,480,640] uint16 (hifihr_amd.data.ho3d_depth_to_u16 of the depth PNGs)."""
    extra = {}
    if "open_2dj" in z and "open_2dj_con" in z:
        extra.update(open_2dj=z["open_2dj"], open_2dj_con=z["open_2dj_con"])
    if "depth_u16" in z:
        extra.update(depth_u16=z["depth_u16"])
    return extra


def ho3d_eval_cache(cli, frames, device):
    """The HO-3D evaluation split as an HO3DDeviceCache (crop window from the hand box, root joint instead of 21 joints: reference
    data/dataset.py:1071-1080).  From --ho3d_eval_cache, else derived from the training frames: box = the projected joints' bounds,
    root = joint 0 of the HO-3D order.  Detections and depth frames travel with either (ho3d_optional_arrays)."""
    from hifihr_amd.data import HO3DDeviceCache
    if cli.ho3d_eval_cache:
        z = np.load(cli.ho3d_eval_cache)
        n = z["images"].shape[0]
        masks = z["hand_masks"] if "hand_masks" in z else np.zeros((n,) + z["images"].shape[1:3], np.uint8)
        return HO3DDeviceCache(z["images"], masks, z["Ks"], np.zeros((n, 21, 3), np.float32) + z["root_xyz"][:, None], device=device,
                               bboxes=z["bboxes"], root_xyz=z["root_xyz"], **ho3d_optional_arrays(z))
    Ks, xyz = np.asarray(frames["Ks"], np.float32), np.asarray(frames["xyz21"], np.float32)
    uvw = np.einsum("nij,nkj->nki", Ks, xyz)
    uv = uvw[..., :2] / uvw[..., 2:3]
    boxes = np.stack([uv.min(1), uv.max(1)], 1)
    extra = {k: frames[k] for k in ("open_2dj", "open_2dj_con", "depth_u16") if k in frames}
    return HO3DDeviceCache(frames["images_u8"], frames["hand_masks_u8"], Ks, xyz, device=device, bboxes=boxes, root_xyz=xyz[:, 0], **extra)


_LPIPS = {}


_DEPTH_RENDERER = {}


def depth_renderer(model):
    """The renderer the stand-in depth images are drawn with: the model's own for the MANO topology, a MANO one beside a NIMBLE-shaped
    model (the ground truth is MANO either way); built once per model."""
    if model.hand_model != "nimble":
        return model.renderer_p3d
    if id(model) not in _DEPTH_RENDERER:
        from hifihr_amd import ops
        _DEPTH_RENDERER[id(model)] = ops.RendererHandle(model.mano_face[0].cpu().numpy(), 778, image_size=224, aa=3)
    return _DEPTH_RENDERER[id(model)]


def make_evaluator(args, device, depth=None):
    """Evaluator of the evaluation pass; with --lpips_weights it also reports LPIPS (the module is built and loaded once per device).
    depth: overrides the option depth_metric (a pass whose batches carry no depth image cannot report depth_mae)."""
    from hifihr_amd.evaluate import Evaluator
    paths = getattr(args, "lpips_weights", None)
    bench = bool(getattr(args, "benchmark_metrics", True))          # the FreiHAND benchmark's PCK / AUC and F-score keys
    cham = bool(getattr(args, "chamfer_metric", False))             # mesh_chamfer / mesh_al_chamfer beside the F-scores
    p2s = bool(getattr(args, "point_mesh_metric", False))           # mesh_p2s / mesh_al_p2s: ground-truth vertices -> the predicted surface
    dep = bool(getattr(args, "depth_metric", False)) if depth is None else bool(depth)      # depth_mae: the rendered depth map against examples['depths']
    if not paths:
        return Evaluator(benchmark=bench, chamfer=cham, point_mesh=p2s, depth=dep)
    key = (str(device), tuple(paths))
    if key not in _LPIPS:
        from hifihr_amd.lpips import LPIPS, load_lpips_weights
        _LPIPS[key] = load_lpips_weights(LPIPS(net="alex"), *paths).to(device)
    return Evaluator(lpips_fn=_LPIPS[key], benchmark=bench, chamfer=cham, point_mesh=p2s, depth=dep)


def fit_keypoints_log(args, refined):
    """With the option fit_keypoints on: say whether the summary that follows describes refined predictions."""
    if not getattr(args, "fit_keypoints", False):
        return
    from hifihr_amd.fit import fit_options
    opt = fit_options(args)
    if refined:
        print(f"[train_hrnet] fit_keypoints: the summary describes predictions REFINED by {opt['iters']} fit iterations against "
              f"'{opt['target']}' in {refined} batches (joints, vertices and j2d; rendered images and texture metrics are the network's)")
    else:
        print(f"[train_hrnet] fit_keypoints: no batch carried '{opt['target']}'; the summary describes the network's own predictions")


def run_evaluation_ho3d(model, cache, args, device, epoch):
    """The reference's HO-3D evaluation pass (train_hrnet.py:55-64 the evaluation queries, :124-136 joints back in the HO-3D order and
    OpenGL axes, :286-293 `pred.json` for the challenge server; texture metrics when rendering): no ground truth exists for this split,
    the product is the dump.  -> (path, n, texture metrics)."""
    from hifihr_amd.fit import refine_outputs
    from hifihr_amd.traineval import data_dic
    # depth_mae is reported when the split carries depth frames (HO3DDeviceCache(depth_u16=...)) and the model renders its depth map
    if getattr(args, "depth_metric", False) and getattr(cache, "depth_u16", None) is None:
        print("[train_hrnet] depth_metric: the HO-3D evaluation split carries no depth_u16; depth_mae is not reported")
        ev = make_evaluator(args, device, depth=False)
    else:
        ev = make_evaluator(args, device)
    refined = 0
    model.eval()
    with torch.no_grad():
        for lo in range(0, cache.n, args.val_batch):
            idx = torch.arange(lo, min(cache.n, lo + args.val_batch))
            zeros = np.zeros((len(idx), 2), np.float32)
            ex = data_dic(cache.batch(idx, center_noise=zeros, scale_noise=np.ones(len(idx), np.float32)), "HO3D", "evaluation", args, device=device)
            out = model("HO3D", False, ex["imgs"], Ks=ex["Ps"], root_xyz=ex["root_xyz"].unsqueeze(1))
            if getattr(args, "fit_keypoints", False):
                out, did = refine_outputs(model, out, ex, args, root_xyz=ex["root_xyz"], root_id=0)
                refined += did
            ev.collect(out, ex, "HO3D", render=args.render)
    model.train()
    fit_keypoints_log(args, refined)
    path = os.path.join(args.pred_output, "test", str(epoch), "pred.json")                     # train_hrnet.py:286-290
    n, _ = ev.dump(path)
    return path, n, ev.summary()


def evaluation_examples(cache, idx, args, device):
    """The `examples` of one FreiHAND evaluation batch (no rotation).  When the pass fits to detections and the cache holds them, the
    batch comes from cache.batch_examples, the one-call form of the same dict that also carries open_2dj / open_2dj_con (cache.batch does
    not); otherwise exactly the two calls made before."""
    from hifihr_amd.traineval import data_dic
    rots = np.zeros(len(idx))
    if fit_wants_detections(args) and getattr(cache, "open_2dj", None) is not None:
        return cache.batch_examples(idx, rots=rots)
    return data_dic(cache.batch(idx, rots=rots), "FreiHand", "training", args, device=device)


def run_evaluation(model, cache, arrays, args, device):
    from hifihr_amd.fit import refine_outputs
    ev = make_evaluator(args, device)
    refined = 0
    model.eval()
    n = cache.n
    with torch.no_grad():
        for lo in range(0, n, args.val_batch):
            idx = torch.arange(lo, min(n, lo + args.val_batch))
            ex = evaluation_examples(cache, idx, args, device)
            if wants_depths(args) and args.render:
                attach_mesh_depths(ex, model)
            root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
            out = model("FreiHand", False, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
            if getattr(args, "fit_keypoints", False):
                out, did = refine_outputs(model, out, ex, args, root_xyz=root)
                refined += did
            ev.collect(out, ex, "FreiHand", render=args.render)
    model.train()
    fit_keypoints_log(args, refined)
    return ev.summary(arrays["joints"], arrays["verts"], root_id=args.ROOT)


def benchmark_report(summary):
    """The twelve values of the FreiHAND benchmark's scores.txt, under its names (those the summary holds); with the option
    chamfer_metric the two Chamfer distances (inputs' unit squared) follow the F-scores, with point_mesh_metric the two point-to-surface
    distances after them."""
    from hifihr_amd.evaluate import BENCHMARK_KEYS, CHAMFER_KEYS, POINT_MESH_KEYS
    lines = [f"{k}: {summary[k]:.6f}" for k in BENCHMARK_KEYS if k in summary]
    return "\n".join(lines + [f"{k}: {summary[k]:.6e}" for k in CHAMFER_KEYS + POINT_MESH_KEYS if k in summary])


def main(argv=None):
    cli = parse(argv)
    args = build_args(cli)
    from hifihr_amd import dist as hdist
    from hifihr_amd import options
    from hifihr_amd.checkpoint import freeze_model_modules, load_model, save_model
    from hifihr_amd.data import FreiHandDeviceCache
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.mano_tables import load_mano_pkl, synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, attach_depth_points, data_dic, train_step

    rank, local_rank, world = hdist.init_process_group_from_env(timeout_min=cli.dist_timeout_min)
    assert torch.cuda.is_available(), "the hot path has no CPU fallback"
    device = torch.device("cuda", local_rank % torch.cuda.device_count())
    torch.cuda.set_device(device)
    torch.cuda.set_stream(torch.cuda.Stream(device=device))            # see GraphedTrainStep: never step on the legacy default stream
    args.device = device
    say = print if rank == 0 else (lambda *a, **k: None)

    tables = load_mano_pkl(cli.mano_pkl) if cli.mano_pkl else synthetic_mano_tables(0)
    torch.manual_seed(0)
    nimble_tables = None
    if args.hand_model == "nimble" and cli.nimble_layer == "synthetic-uv":
        from hifihr_amd.nimble_tables import add_synthetic_uv, synthetic_nimble_tables
        nimble_tables = add_synthetic_uv(synthetic_nimble_tables(0))
    model = Model(ifRender=args.render, device=device, if_4c=args.four_channel, hand_model=args.hand_model,
                  use_mean_shape=args.use_mean_shape, pretrain=args.pretrain, root_id=args.ROOT, root_id_nimble=args.ROOT_NIMBLE,
                  ifLight=args.light_estimation, mano_tables=tables, texture_stand_in=args.texture_stand_in,
                  nimble_tables=nimble_tables, **soft_silhouette_kwargs(args), **render_depth_kwargs(args)).to(device).train()
    frozen = freeze_model_modules(model, args)          # only_train_regressor / only_train_texture (train_hrnet.py:566)
    if frozen:
        say("[train_hrnet] frozen:", ", ".join(frozen))
    flat = FlatParams(model)
    hdist.broadcast_params(flat)
    reducer = hdist.GradReducer(flat, num_buckets=4)
    wd = 0.01 if args.optimizer == "AdamW" else 0.0                   # train_hrnet.py:549-550: "AdamW" is Adam with L2 0.01
    opt = FusedAdam(flat, lr=args.init_lr, betas=(0.9, 0.999), weight_decay=wd, grad_scale=reducer.grad_scale,
                    max_grad_norm=optimizer_max_grad_norm(args))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=args.lr_steps, gamma=args.lr_gamma)
    model, current_epoch, opt, sched = load_model(model, opt, sched, args)
    if args.force_init_lr > 0:
        opt.param_groups[0]["lr"] = args.force_init_lr
    loss_func = LossFunction()

    dat_name = cli.dataset
    if dat_name == "HO3D":
        return train_ho3d(cli, args, model, loss_func, opt, sched, reducer, current_epoch, rank, world, device, say)
    fit_det = fit_wants_detections(args)
    train_arrays, eval_arrays = load_or_make_dataset(cli, model, device, keypoints=wants_keypoints(args) or fit_det, eval_keypoints=fit_det)
    if wants_keypoints(args) and "open_2dj" not in train_arrays:
        raise SystemExit(f"[train_hrnet] the losses {[k for k in args.losses if k in KEYPOINT_LOSSES]} need 2-D detections: give "
                         "--openpose_keypoints <json>, or open_2dj / open_2dj_con in the --freihand_cache npz")
    has_eval = eval_arrays is not None and len(eval_arrays["images"]) > 0
    if fit_det and "open_2dj" not in (eval_arrays if has_eval else train_arrays):
        raise SystemExit("[train_hrnet] fit_keypoints with fit_target 'open_2dj' needs 2-D detections for the samples the evaluation pass runs "
                         "on: give " + ("eval_open_2dj / eval_open_2dj_con" if has_eval else "open_2dj / open_2dj_con (or --openpose_keypoints)") +
                         " in the --freihand_cache npz, or set fit_target to 'j2d_gt'")
    cache = FreiHandDeviceCache(train_arrays["images"], train_arrays["masks"], train_arrays["Ks"], train_arrays["joints"],
                                train_arrays["verts"], device=device, open_2dj=train_arrays.get("open_2dj"),
                                open_2dj_con=train_arrays.get("open_2dj_con"), semi_ratio=getattr(args, "semi_ratio", None))
    eval_cache = None
    if eval_arrays is not None and len(eval_arrays["images"]):
        eval_cache = FreiHandDeviceCache(eval_arrays["images"], eval_arrays["masks"], eval_arrays["Ks"], eval_arrays["joints"],
                                         eval_arrays["verts"], device=device, open_2dj=eval_arrays.get("open_2dj"),
                                         open_2dj_con=eval_arrays.get("open_2dj_con"))       # (detections only when the pass fits to them)
    say(f"[train_hrnet] {cache.n} training samples resident on {device}; world {world}; encoder {args.pretrain}; losses {args.losses}")

    if "evaluation" in args.mode:
        summary = run_evaluation(model, eval_cache or cache, eval_arrays or train_arrays, args, device)
        say("[train_hrnet] evaluation:", summary)
        if getattr(args, "benchmark_metrics", True) or getattr(args, "chamfer_metric", False) or getattr(args, "point_mesh_metric", False):
            say("[train_hrnet] benchmark scores:\n" + benchmark_report(summary))
        return 0

    B = args.train_batch
    gen = torch.Generator().manual_seed(1000 + current_epoch)         # same permutation on every rank
    rot_gen = torch.Generator().manual_seed(77 + rank)                # ... different rotations
    points_gen = torch.Generator().manual_seed(177 + rank)            # ... and draws of depth_points
    stepper, stepper_key, it, t_last = None, None, 0, time.perf_counter()
    for epoch in range(1, args.total_epochs + 1 - current_epoch):
        options.update_lambdas_for_epoch(args, epoch + current_epoch)
        lam_key = (args.lambda_pose, args.lambda_j2d_gt, args.lambda_shape, args.lambda_tex_reg)
        if stepper is not None and lam_key != stepper_key:
            stepper.release()
            stepper = None                        # the loss weights are kernel arguments baked into the captured graph: re-capture
        perm = torch.randperm(cache.n, generator=gen)
        per_step = B * world
        for lo in range(0, cache.n - per_step + 1, per_step):
            idx = perm[lo + rank * B: lo + (rank + 1) * B]
            # the batch is written straight into the captured step's static inputs (one staged copy + two launches)
            ex = cache.batch_examples(idx, generator=rot_gen, out=stepper.static if stepper is not None else None, root_id=args.ROOT)
            if "depth" in args.losses or wants_depth_points(args):
                static = stepper.static if stepper is not None else None
                attach_mesh_depths(ex, model, static=static)
                if wants_depth_points(args):                  # the target points of chamfer / point_mesh from that depth map
                    attach_depth_points(ex, args, generator=points_gen, out=static.get("chamfer_points") if static is not None else None)
            if cli.graph and stepper is None:
                ok = 1
                try:
                    stepper = GraphedTrainStep(model, loss_func, opt, ex, args, reducer=reducer if world > 1 else None)
                    stepper_key = lam_key
                except Exception as e:            # noqa: BLE001  -- report and continue eagerly (GraphedTrainStep restored the state)
                    # (collective-free constructor: the ranks meet in the flag all-reduce below -- see the HO-3D loop above)
                    print(f"[train_hrnet] rank {rank}: hipGraph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr, flush=True)
                    ok = 0
                if world > 1:                     # the two step forms issue their bucket all-reduces in different orders: all ranks
                    flag = torch.tensor([ok], device=device, dtype=torch.int32)       # must take the same one
                    torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
                    ok = int(flag.item())
                if not ok:
                    if stepper is not None:
                        stepper.release()
                    stepper, cli.graph = None, 0
            if stepper is not None:
                if ex["imgs"].data_ptr() != stepper.static["imgs"].data_ptr():      # the batch the step was captured on
                    stepper.load_batch(ex)
                loss, dic = stepper()
            else:
                loss, dic = train_step(model, loss_func, opt, ex, args, backward_hook=reducer.finish)
            it += 1
            if it % cli.print_freq == 0 or it == cli.max_iters:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t_last
                t_last = time.perf_counter()
                n_it = cli.print_freq if it % cli.print_freq == 0 else it % cli.print_freq
                terms = " ".join(f"{k}={float(dic[k].detach()):.4g}" for k in args.losses)
                say(f"[train_hrnet] epoch {epoch + current_epoch} it {it} loss {float(loss.detach()):.5f} ({terms}) {n_it * per_step / dt:.0f} img/s"
                    + grad_guard_log(opt.grad_stats()))
            if cli.max_iters and it >= cli.max_iters:
                break
        if (epoch + current_epoch) % args.save_interval == 0 or (cli.max_iters and it >= cli.max_iters):
            if args.if_test and eval_cache is not None:
                say("[train_hrnet] test:", run_evaluation(model, eval_cache, eval_arrays, args, device))
            if rank == 0:
                say("[train_hrnet] saved", save_model(model, opt, sched, epoch, current_epoch, args))
        sched.step()
        if cli.max_iters and it >= cli.max_iters:
            break
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    say("Done!")
    return 0


if __name__ == "__main__":
    sys.exit(main())
