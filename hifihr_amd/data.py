"""FreiHAND training samples assembled on the device.

The reference decodes a JPEG, rotates image and mask in the plane with PIL and rotates the 3-D annotations, per sample,
in CPU DataLoader workers (reference data/dataset.py:153-289 `get_sample`, utils/handutils.py:48-101), then copies the
batch to the GPU.  At several thousand images per second per GPU that pipeline is the bottleneck, so here the decoded
dataset is kept in HBM as uint8 (32 560 training images x 224 x 224 x RGBX = 6.5 GB + masks 1.6 GB, out of 288 GB) and
a batch is one gather-and-warp launch (csrc/augment.hip) plus two small batched products for K / joints / verts:
no host pixels, no H2D copy in the step.  JPEG decoding itself (done once, offline or at start-up) is not part of this.

`affine_for_rotation` restates utils/handutils.py:63-101 get_affine_transform for the call the dataset makes
(centre = image centre, scale = res); the warp coefficients go through the same float32 -> numpy inverse -> PIL 16.16
fixed-point chain as the reference, which makes the device warp bit-exact with PIL (tests/golden/data_path.npz).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ._lib import get_lib, require_cuda

# 1: the batch kernels read their per-sample parameters straight from the pinned staging slot (no staged H2D copy in front of them).  Measured
# 10 us/step faster on a fresh box and 0.2 ms/step SLOWER in a process that follows a long host-side job (the -m gpu suite) on the same box:
# device reads of host memory depend on the state of the host's memory.  Off: one staged copy (profiles/r05_batch_params_ab.txt).
_DIRECT_PARAMS = os.environ.get("HIFIHR_BATCH_DIRECT_PARAMS", "0") != "0"


def _no_rot(center, scale, res):
    """utils/handutils.py:104-111: crop of `scale` pixels around `center` resized to `res` (rows, cols)."""
    t = np.zeros((3, 3))
    t[0, 0] = float(res[1]) / scale
    t[1, 1] = float(res[0]) / scale
    t[0, 2] = res[1] * (-float(center[0]) / scale + 0.5)
    t[1, 2] = res[0] * (-float(center[1]) / scale + 0.5)
    t[2, 2] = 1
    return t


def affine_for_rotation(center, scale, res, rot):
    """utils/handutils.py:63-101.  Returns (total_trans, post_rot_trans) as float32 3x3: the image warp (rotation about the
    origin followed by the crop around the rotated centre) and the crop that stays to be applied to K once the 3-D points
    have been rotated about the optical axis."""
    sn, cs = np.sin(rot), np.cos(rot)
    rot_mat = np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]])
    c = np.array([center[0], center[1], 1.0])
    origin_rot_center = rot_mat.dot(c)[:2]
    shift = np.eye(3); shift[0, 2] = -res[1] / 2; shift[1, 2] = -res[0] / 2
    back = np.eye(3); back[0, 2] = res[1] / 2; back[1, 2] = res[0] / 2
    centre_after = back.dot(rot_mat).dot(shift).dot(c)
    total = _no_rot(origin_rot_center, scale, res).dot(rot_mat)
    post = _no_rot(centre_after[:2], scale, res)
    return total.astype(np.float32), post.astype(np.float32)


def pil_affine_fixed_terms(affine_trans):
    """The six 16.16 fixed-point integers PIL's nearest-neighbour AFFINE transform derives from transform_img's coefficients
    (utils/handutils.py:55-59: rows 0-1 of the float32 inverse of `affine_trans`)."""
    inv = np.linalg.inv(affine_trans)
    a, b, c, d, e, f = (float(inv[0, 0]), float(inv[0, 1]), float(inv[0, 2]), float(inv[1, 0]), float(inv[1, 1]), float(inv[1, 2]))
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(a), fix(b), fix(c + a * 0.5 + b * 0.5), fix(d), fix(e), fix(f + d * 0.5 + e * 0.5)]


def batch_affine_terms(center, scale, res, rots, with_total=False):
    """`affine_for_rotation` + `pil_affine_fixed_terms` for a whole batch in stacked numpy calls (the per-sample Python loop
    costs ~1 ms per 32 samples, a tenth of a training step).  Returns (fixed int32 [B,6], post_rot_trans f32 [B,3,3],
    rot_mat f32 [B,3,3]).  Same operations in the same order on stacked arrays; tests compare it with the per-sample path.
    with_total: also the float32 `total` [B,3,3] itself, the forward affine that carries a pixel of the stored image to the warped one
    (`affinetrans` of data/dataset.py:245-257: what handutils.transform_coords applies to the 2-D detections)."""
    rots = np.asarray(rots, dtype=np.float64)
    B = rots.shape[0]
    sn, cs = np.sin(rots), np.cos(rots)
    rot_mat = np.zeros((B, 3, 3))
    rot_mat[:, 0, 0] = cs; rot_mat[:, 0, 1] = -sn; rot_mat[:, 1, 0] = sn; rot_mat[:, 1, 1] = cs; rot_mat[:, 2, 2] = 1.0
    c = np.array([center[0], center[1], 1.0])
    origin = np.matmul(rot_mat, c)[:, :2]
    shift = np.eye(3); shift[0, 2] = -res[1] / 2; shift[1, 2] = -res[0] / 2
    back = np.eye(3); back[0, 2] = res[1] / 2; back[1, 2] = res[0] / 2
    centre_after = np.matmul(np.matmul(np.matmul(back, rot_mat), shift), c)

    def no_rot(cen):
        t = np.zeros((B, 3, 3))
        t[:, 0, 0] = float(res[1]) / scale
        t[:, 1, 1] = float(res[0]) / scale
        t[:, 0, 2] = res[1] * (-cen[:, 0] / scale + 0.5)
        t[:, 1, 2] = res[0] * (-cen[:, 1] / scale + 0.5)
        t[:, 2, 2] = 1
        return t
    total = np.matmul(no_rot(origin), rot_mat).astype(np.float32)
    post = no_rot(centre_after[:, :2]).astype(np.float32)
    inv = np.linalg.inv(total).astype(np.float64)
    a, b, cc, d, e, f = inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2], inv[:, 1, 0], inv[:, 1, 1], inv[:, 1, 2]
    fix = lambda v: np.floor(v * 65536.0 + 0.5).astype(np.int64)
    fixed = np.stack([fix(a), fix(b), fix(cc + a * 0.5 + b * 0.5), fix(d), fix(e), fix(f + d * 0.5 + e * 0.5)], axis=1).astype(np.int32)
    if with_total:
        return fixed, post, rot_mat.astype(np.float32), total
    return fixed, post, rot_mat.astype(np.float32)


class FreiHandDeviceCache:
    """The decoded training set resident in device memory + per-batch augmentation on the device.

    images_u8 [n,H,W,3] uint8, masks_u8 [n,H,W] (or [n,H,W,3]) uint8 in {0,255}, Ks [n,3,3], joints [n,21,3], verts [n,778,3]
    (host tensors / arrays; moved once).  `batch(idxs, rots)` returns the reference's training sample dict
    {trans_images, trans_Ks, trans_joints, trans_verts, trans_masks, scales, idxs} with every tensor on the device.
    open_2dj [n,21,2] + open_2dj_con [n,21] or [n,21,1]: off-the-shelf 2-D detections in pixels of the stored images and their
    confidences, for the self-supervised terms; `batch_examples` then also returns KEYPOINT_KEYS (one more launch).  semi_ratio
    (args.semi_ratio): the share of the training set whose detections are replaced by the projected ground truth."""

    def __init__(self, images_u8, masks_u8, Ks, joints, verts, scales=None, device="cuda", max_rot=math.pi, open_2dj=None,
                 open_2dj_con=None, semi_ratio=None):
        images_u8 = torch.as_tensor(images_u8)
        n, H, W, _ = images_u8.shape
        rgbx = torch.zeros(n, H, W, 4, dtype=torch.uint8)
        rgbx[..., :3] = images_u8
        self.images = rgbx.to(device).view(torch.int32).reshape(n, H, W)
        masks_u8 = torch.as_tensor(masks_u8)
        if masks_u8.dim() == 4:
            masks_u8 = masks_u8[..., 0]
        self.masks = masks_u8.contiguous().to(device)
        require_cuda(self.images, self.masks)
        f32 = lambda t: torch.as_tensor(t, dtype=torch.float32).to(device)
        self.Ks, self.joints, self.verts = f32(Ks), f32(joints), f32(verts)
        self.scales = f32(scales) if scales is not None else (self.joints[:, 9] - self.joints[:, 10]).norm(dim=-1)
        self.n, self.H, self.W, self.device, self.max_rot = n, H, W, torch.device(device), max_rot
        self.lib = get_lib()
        if (open_2dj is None) != (open_2dj_con is None):
            raise ValueError("FreiHandDeviceCache: open_2dj and open_2dj_con come together")
        self.open_2dj = self.open_2dj_con = None
        if open_2dj is not None:
            self.open_2dj, self.open_2dj_con = f32(open_2dj).contiguous(), f32(open_2dj_con).contiguous()
            if tuple(self.open_2dj.shape) != (n, 21, 2) or tuple(self.open_2dj_con.shape) not in ((n, 21), (n, 21, 1)):
                raise ValueError(f"FreiHandDeviceCache: open_2dj must be [{n},21,2] and open_2dj_con [{n},21] or [{n},21,1], got "
                                 f"{tuple(self.open_2dj.shape)} and {tuple(self.open_2dj_con.shape)}")
        self.semi_ratio = semi_ratio

    _RING = 32         # pinned staging slots (the device reads a slot when it gets to it, possibly many host steps later)
    _GROUP = 8         # ... released in groups: ONE event per _GROUP steps (an event record is a barrier packet between the batch kernels and the step)

    def _stage(self, nwords):
        if not hasattr(self, "_slots"):
            # every slot of the ring now: a pinned allocation is a driver call of a millisecond or more, and the first trip round the ring
            # would otherwise pay one per step (bench.py's default warm-up is shorter than the ring: the last allocations landed in the timed
            # region, +0.1 ms/step over 30 steps every time it happened)
            self._slots = [self._pinned(nwords) for _ in range(self._RING)]
            self._events, self._turn = [None] * (self._RING // self._GROUP), 0
        i = self._turn = (self._turn + 1) % self._RING
        if i % self._GROUP == 0 and self._events[i // self._GROUP] is not None:
            self._events[i // self._GROUP].synchronize()        # every launch that read a slot of this group has completed
        if self._slots[i] is None or self._slots[i].numel() < nwords:
            self._slots[i] = self._pinned(nwords)                # (a larger batch than the ring was made for)
        return i, self._slots[i][:nwords]

    def _pinned(self, nwords):
        t = torch.empty(nwords, dtype=torch.int32)
        return t.pin_memory() if self.device.type == "cuda" else t

    def _packed_terms(self, idxs, rots, generator, direct=False, keypoints=False):
        """Host side of one batch: affine coefficients (numpy, stacked) packed with the indices and the two 3x3 matrices per sample
        into ONE pinned staging buffer that goes over in ONE asynchronous copy.  -> (B, packed int32 [25 B] on the device, slot);
        direct=True: the pinned buffer itself (see below).  keypoints=True: the float32 forward affines of the warp, [B,3,3], go over as
        well, in a staging buffer of their own that shares the slot's turn (self._total_d; the 25-word layout is unchanged)."""
        idxs = torch.as_tensor(idxs, dtype=torch.int64)
        B = idxs.shape[0]
        if rots is None:                       # np.random.uniform(-max_rot, max_rot) per sample (data/dataset.py:237)
            rots = (2 * torch.rand(B, generator=generator, dtype=torch.float64) - 1) * self.max_rot
        rots = np.asarray(rots, dtype=np.float64)
        fixed, post, rmat, total = batch_affine_terms(np.asarray([self.W // 2, self.H // 2]), self.H, [self.H, self.W], rots, with_total=True)
        slot, host = self._stage(25 * B)
        if keypoints:
            if not hasattr(self, "_total_slots"):
                self._total_slots = [None] * self._RING
            if self._total_slots[slot] is None or self._total_slots[slot].numel() < 9 * B:
                t = torch.empty(9 * B, dtype=torch.float32)
                self._total_slots[slot] = t.pin_memory() if self.device.type == "cuda" else t
            th = self._total_slots[slot][:9 * B]
            th.numpy()[:] = total.reshape(-1)
            self._total_d = torch.empty(B, 3, 3, dtype=torch.float32, device=self.device)
            self._total_d.view(-1).copy_(th, non_blocking=True)          # (before the slot's release below: one event covers both buffers)
        hv = host.numpy()
        hv[:B] = idxs.numpy().astype(np.int32)
        hv[B:7 * B] = fixed.reshape(-1)
        hv[7 * B:16 * B] = post.reshape(-1).view(np.int32)
        hv[16 * B:25 * B] = rmat.reshape(-1).view(np.int32)
        if direct:
            # the kernels read the pinned slot THEMSELVES (hipHostMalloc memory is mapped into the device's address space: 100 B per sample
            # over the host link, once, by the workgroups that need them): no staging copy -- a blit kernel of its own on this runtime, with a
            # hand-over on either side, in front of every step.  The caller releases the slot behind its launches (_release).
            return B, host, slot
        packed = torch.empty(25 * B, dtype=torch.int32, device=self.device)
        packed.copy_(host, non_blocking=True)
        self._release(slot)
        return B, packed, slot

    def _release(self, slot):
        """The stream is done with the slot once it gets here; recorded behind the LAST slot of a group (the slots are used in order)."""
        if self.device.type == "cuda" and slot % self._GROUP == self._GROUP - 1:
            g = slot // self._GROUP
            ev = self._events[g] or torch.cuda.Event()
            ev.record()
            self._events[g] = ev

    EXAMPLE_KEYS = ("imgs", "masks", "segms_gt", "Ks", "Ps", "joints", "verts", "j2d_gt", "scales", "idxs")

    KEYPOINT_KEYS = ("open_2dj", "open_2dj_con", "texture_con")           # only from a cache that was given detections

    STEP_KEYS = ("root_xyz", "joints_rel", "verts_rel", "cam_ndc")      # what a training iteration derives from the batch (root_id given)

    def batch_examples(self, idxs, rots=None, generator=None, out=None, root_id=None):
        """`data_dic(self.batch(...), "FreiHand", "training", ...)` -- the `examples` dict of a training step (reference
        utils/traineval_util.py:21-111 over data/dataset.py:223-275) -- from ONE staged copy and TWO launches
        (hifihr_freihand_batch: warp + segmentation plane; camera / joint / vertex / projection terms).  The two-step form costs
        ~30 small ATen launches and, in front of a captured step, one device copy per entry of the dict (0.3 ms of a 6.4 ms step).
        out: a dict holding tensors for EXAMPLE_KEYS (the static inputs of traineval.GraphedTrainStep) to be written in place.
        root_id (= args.ROOT): the same two launches also emit STEP_KEYS -- root_xyz [B,1,3] = joints[:, root_id], joints_rel / verts_rel
        (train_hrnet.py:62-68) and cam_ndc [B,4] (models_res_nimble.py:184-186,228-235) -- which traineval.forward_backward and
        Model.forward pick up instead of four elementwise launches per step.
        A cache that holds detections also returns KEYPOINT_KEYS -- open_2dj [B,21,2] warped like the image, open_2dj_con (the cache's
        shape per sample), texture_con [B], with the semi-supervised mix when semi_ratio was given -- from ONE more launch
        (hifihr_freihand_keypoints) and one more staged copy of 36 bytes per sample."""
        kp = self.open_2dj is not None
        B, packed, slot = self._packed_terms(idxs, rots, generator, direct=_DIRECT_PARAMS and self.device.type == "cuda", keypoints=kp)
        kp_shapes = {"open_2dj": (B, 21, 2), "open_2dj_con": (B,) + tuple(self.open_2dj_con.shape[1:]), "texture_con": (B,)} if kp else {}
        dev, J, V = self.device, self.joints.shape[1], self.verts.shape[1]
        if out is None:
            f = lambda *shape: torch.empty(*shape, device=dev)
            out = {"imgs": f(B, 3, self.H, self.W), "masks": f(B, 3, self.H, self.W),
                   "segms_gt": torch.empty(B, self.H, self.W, dtype=torch.int64, device=dev), "Ks": f(B, 3, 3), "Ps": f(B, 3, 4),
                   "joints": f(B, J, 3), "verts": f(B, V, 3), "j2d_gt": f(B, J, 2), "scales": f(B),
                   "idxs": torch.empty(B, dtype=torch.int64, device=dev)}
            if root_id is not None:
                out.update({"root_xyz": f(B, 1, 3), "joints_rel": f(B, J, 3), "verts_rel": f(B, V, 3), "cam_ndc": f(B, 4)})
            out.update({k: f(*shape) for k, shape in kp_shapes.items()})
        else:
            expect = {"imgs": (B, 3, self.H, self.W), "masks": (B, 3, self.H, self.W), "segms_gt": (B, self.H, self.W), "Ks": (B, 3, 3),
                      "Ps": (B, 3, 4), "joints": (B, J, 3), "verts": (B, V, 3), "j2d_gt": (B, J, 2), "scales": (B,), "idxs": (B,)}
            if root_id is not None or all(k in out for k in self.STEP_KEYS):
                expect.update({"root_xyz": (B, 1, 3), "joints_rel": (B, J, 3), "verts_rel": (B, V, 3), "cam_ndc": (B, 4)})
                if root_id is None:
                    root_id = getattr(self, "_root_id", None)
                    if root_id is None:
                        raise ValueError("batch_examples(out=...): `out` holds the step terms (root_xyz, joints_rel, ...) but no root_id was "
                                         "given here or in an earlier call")
            expect.update(kp_shapes)
            for k, shape in expect.items():
                if k not in out or tuple(out[k].shape) != shape:
                    raise ValueError(f"batch_examples(out=...): '{k}' must be a tensor of shape {shape}")
            out = {k: out[k] for k in expect}
        if root_id is not None:
            self._root_id = root_id                              # (a later in-place call on the same dict keeps the step terms current)
        self.lib.freihand_batch(self.images, self.masks, self.Ks, self.joints, self.verts, self.scales, packed, B, out,
                                root_id=root_id, image_size=self.H)
        if kp:
            from .traineval import semi_below
            below = semi_below(self.semi_ratio)
            self.lib.freihand_keypoints(self.open_2dj, self.open_2dj_con, packed[:B], self._total_d, out["j2d_gt"] if below else None, below,
                                        out["open_2dj"], out["open_2dj_con"], out["texture_con"])
        self._release(slot)
        return out

    def batch(self, idxs, rots=None, generator=None, out_images=None, out_masks=None):
        """One training batch assembled on the device.  Host work: the affine coefficients (numpy, stacked) and ONE pinned
        staging buffer (indices + 16.16 warp terms + the two 3x3 matrices per sample) that goes over in ONE asynchronous copy.
        out_images / out_masks: write the warped planes straight into caller-owned tensors (the static inputs of a captured step)."""
        B, packed, _ = self._packed_terms(idxs, rots, generator)
        dev = self.device
        idx_d, coef_d = packed[:B], packed[B:7 * B].view(B, 6)
        post_d = packed[7 * B:16 * B].view(torch.float32).view(B, 3, 3)
        rmat_d = packed[16 * B:25 * B].view(torch.float32).view(B, 3, 3)
        imgs = out_images if out_images is not None else torch.empty(B, 3, self.H, self.W, device=dev)
        masks = out_masks if out_masks is not None else torch.empty(B, 3, self.H, self.W, device=dev)
        self.lib.freihand_augment(self.images, self.masks, idx_d, coef_d, imgs, masks)
        idx_l = idx_d.long()
        # 3x3 products as broadcast multiply-adds (a batched-GEMM call would put a vendor-library kernel on the step's path)
        Ks = (post_d.unsqueeze(3) * self.Ks[idx_l].unsqueeze(1)).sum(2)                            # post_rot_trans . K  (:258-260)
        rot = lambda pts: (pts.unsqueeze(2) * rmat_d.unsqueeze(1)).sum(3)                          # (R p^T)^T          (:271-275)
        return {
            "trans_images": imgs, "trans_masks": masks, "trans_Ks": Ks,
            "trans_joints": rot(self.joints[idx_l]), "trans_verts": rot(self.verts[idx_l]),
            "scales": self.scales[idx_l], "idxs": idx_l,
        }


# ------------------------------------------------------------------------------------------------
# HO-3D (reference data/dataset.py:1023-1215): hand crop + resize on the device
# ------------------------------------------------------------------------------------------------
def ho3d_crop_windows(uv21, center_noise, scale_noise, inp_res=224, img_wh=(640.0, 480.0)):
    """The crop window of every sample of a batch, the reference's float32 arithmetic (dataset.py:1106-1161, `ho_scope = 0`), stacked.
    uv21 [B,P,2] the points the window is formed from: the 21 projected joints (u, v), or the 2 corners of the evaluation split's hand box; center_noise [B,2] = 5 * randn(2) per sample (:1120); scale_noise [B] =
    (1 - 1.1) * rand(1) + 1 - 0.1 (:1126).  `int / tensor` is tensor.reciprocal() * int in torch, hence the two-step divisions.
    -> crop_center [B,2], scale [B], size [B] (= crop_size_scales), box int32 [B,4] = the (x0, y0, x1, y1) Pillow's Image.crop makes of
    (x1, y1, x1 + size, y1 + size): Python round(), half to even."""
    f = np.float32
    uv = np.asarray(uv21, dtype=f)
    lo, hi = uv.min(1), uv.max(1)
    center = (hi + lo) / f(2)
    center = np.asarray(center_noise, dtype=f) + center
    min_uv = np.maximum(lo, f(0)) - f(10.0)
    max_uv = np.minimum(hi, np.asarray(img_wh, dtype=f)[None]) + f(10.0)
    best = (f(4) * np.maximum(max_uv - center, center - min_uv)).max(1)
    best = np.minimum(np.maximum(best, f(50.0)), f(640.0))
    scale = f(inp_res) * (f(1) / best)
    scale = np.minimum(scale, f(10.0))
    scale = (scale * np.asarray(scale_noise, dtype=f)).astype(f)
    size = (f(inp_res) * (f(1) / scale)).astype(f)
    half = np.floor(size / f(2))
    y1 = (center[:, 1] - half).astype(f)
    x1 = (center[:, 0] - half).astype(f)
    # Image.crop((left, top, left + width, top + height)) on Python floats (the reference passes .item() values)
    x1d, y1d, sd = x1.astype(np.float64), y1.astype(np.float64), size.astype(np.float64)
    box = np.stack([np.rint(x1d), np.rint(y1d), np.rint(x1d + sd), np.rint(y1d + sd)], 1).astype(np.int32)      # rint: half to even
    return center.astype(f), scale, size, box


HO3D_MAX_WINDOW = 800          # HIFIHR_HO3D_MAX_WINDOW (include/hifihr.h): the longest box edge hifihr_ho3d_batch resamples
HO3D_DEPTH_SCALE = 0.00012498664727900177      # metres per unit of an HO-3D depth image (reference data/dataset.py:1040)


def ho3d_depth_to_u16(rgb_u8):
    """An HO-3D depth PNG as decoded to [..., 3] uint8 (R, G, B) -> the 16-bit depth it encodes, `rgb[..., 2] + 256 * rgb[..., 1]`
    (reference data/dataset.py:1041), as uint16: what `HO3DDeviceCache(depth_u16=...)` keeps on the device.  Host helper (numpy)."""
    rgb = np.asarray(rgb_u8)
    if rgb.dtype != np.uint8 or rgb.shape[-1] < 3:
        raise ValueError(f"ho3d_depth_to_u16: expected uint8 [..., 3], got {rgb.dtype} {rgb.shape}")
    return rgb[..., 2].astype(np.uint16) + np.uint16(256) * rgb[..., 1].astype(np.uint16)


class HO3DDeviceCache:
    """The decoded HO-3D training frames resident in device memory + the per-batch hand crop on the device (reference
    data/dataset.py:1023-1215).  images_u8 [n,480,640,3], hand_masks_u8 [n,480,640] (channel 0 of the reference's mask image, 0 / 255),
    Ks [n,3,3] (camMat . cam_extr as the dataset forms it), xyz21 [n,21,3].  `batch(idxs)` returns the sample dict the HO3D branch of
    `traineval.data_dic` reads -- img_crop, hand_mask_crop, K_crop, uv21_crop, xyz21 -- with every tensor on the device: one staged
    copy of 32 bytes per sample and three launches (hifihr_ho3d_batch); pixels bit-exact with the reference's PIL path.
    Opt-in, each ONE more launch on the same staged copy: detections (`open_2dj_crop`, `open_2dj_con`: hifihr_ho3d_keypoints) and the
    metric depth (`depth_crop`: hifihr_ho3d_depth_crop).  A cache built without them returns the dict above from the launches above."""

    KEYPOINT_KEYS = ("open_2dj_crop", "open_2dj_con")      # only from a cache that was given detections
    DEPTH_KEYS = ("depth_crop",)                           # only from a cache that was given depth frames

    def __init__(self, images_u8, hand_masks_u8, Ks, xyz21, device="cuda", inp_res=224, bboxes=None, root_xyz=None, open_2dj=None,
                 open_2dj_con=None, depth_u16=None, depth_scale=HO3D_DEPTH_SCALE):
        """bboxes [n,2,2] ((x0, y0), (x1, y1)) + root_xyz [n,3]: the EVALUATION split, which carries a hand bounding box and the root joint
        instead of 21 joints (dataset.py:1071-1080): the crop window is then formed from the box corners, and `batch` also returns
        `root_xyz` with y / z negated as those lines do.
        open_2dj [n,21,2] (pixels of the stored frame, FreiHAND joint order as data_dic assumes) + open_2dj_con [n,21] or [n,21,1]: 2-D
        detections; `batch` then also returns open_2dj_crop [B,21,2] = (open_2dj - centre) * scale + inp_res // 2 (dataset.py:1199-1203) and
        open_2dj_con (the cache's shape per sample), bit for bit.
        depth_u16 [n,H,W] uint16 (`ho3d_depth_to_u16` of the depth PNGs) with depth_scale metres per unit: `batch` then also returns
        depth_crop [B,S,S] float32 in metres, the frame through the crop box with NEAREST resampling (include/hifihr.h)."""
        images_u8 = torch.as_tensor(images_u8)
        n, H, W, _ = images_u8.shape
        rgbx = torch.zeros(n, H, W, 4, dtype=torch.uint8)
        rgbx[..., :3] = images_u8
        self.images = rgbx.to(device).view(torch.int32).reshape(n, H, W)
        self.masks = torch.as_tensor(hand_masks_u8).contiguous().to(device)
        require_cuda(self.images, self.masks)
        Ks = torch.as_tensor(Ks, dtype=torch.float32)
        xyz21 = torch.as_tensor(xyz21, dtype=torch.float32)
        uvw = (xyz21.unsqueeze(2) * Ks.unsqueeze(1)).sum(3)                    # proj_func (fh_utils.py:30-39), dataset.py:1093
        self.uv21_host = (uvw[:, :, :2] / uvw[:, :, 2:3]).numpy()
        self.window_pts = np.asarray(bboxes, dtype=np.float32) if bboxes is not None else self.uv21_host     # what the crop window is formed from
        self.root_xyz = None
        if root_xyz is not None:                                                   # dataset.py:1078-1080
            self.root_xyz = (torch.as_tensor(root_xyz, dtype=torch.float32) * torch.tensor([1.0, -1.0, -1.0])).to(device)
        self.Ks, self.xyz21, self.uv21 = Ks.to(device), xyz21.to(device), torch.from_numpy(self.uv21_host).to(device)
        self.n, self.H, self.W, self.device, self.inp_res = n, H, W, torch.device(device), inp_res
        self.lib = get_lib()
        self._ws = None
        if (open_2dj is None) != (open_2dj_con is None):
            raise ValueError("HO3DDeviceCache: open_2dj and open_2dj_con come together (the detections and their confidences)")
        self.open_2dj = self.open_2dj_con = self.depth_u16 = None
        if open_2dj is not None:
            det, con = torch.as_tensor(open_2dj, dtype=torch.float32), torch.as_tensor(open_2dj_con, dtype=torch.float32)
            if tuple(det.shape) != (n, 21, 2) or tuple(con.shape) not in ((n, 21), (n, 21, 1)):
                raise ValueError(f"HO3DDeviceCache: open_2dj {tuple(det.shape)} / open_2dj_con {tuple(con.shape)} for {n} frames: expected "
                                 f"[{n},21,2] and [{n},21] or [{n},21,1]")
            self.open_2dj, self.open_2dj_con = det.contiguous().to(device), con.contiguous().to(device)
        if depth_u16 is not None:
            d = depth_u16 if torch.is_tensor(depth_u16) else torch.from_numpy(np.ascontiguousarray(depth_u16))
            if d.dtype != torch.uint16 or tuple(d.shape) != (n, H, W):
                raise ValueError(f"HO3DDeviceCache: depth_u16 {d.dtype} {tuple(d.shape)}: expected uint16 [{n},{H},{W}] (ho3d_depth_to_u16)")
            self.depth_u16, self.depth_scale = d.contiguous().to(device), float(depth_scale)
            require_cuda(self.depth_u16)

    _RING, _GROUP = FreiHandDeviceCache._RING, FreiHandDeviceCache._GROUP
    _stage = FreiHandDeviceCache._stage
    _pinned = FreiHandDeviceCache._pinned
    _release = FreiHandDeviceCache._release

    def batch(self, idxs, center_noise=None, scale_noise=None, generator=None):
        idxs = torch.as_tensor(idxs, dtype=torch.int64)
        B = idxs.shape[0]
        if center_noise is None:               # dataset.py:1120 and :1126, per sample in that order
            draws = [(5 * torch.randn(2, generator=generator), (1 - 1.1) * torch.rand(1, generator=generator) + 1 - 0.1) for _ in range(B)]
            center_noise = torch.stack([d[0] for d in draws]).numpy()
            scale_noise = torch.cat([d[1] for d in draws]).numpy()
        center, scale, _, box = ho3d_crop_windows(self.window_pts[idxs.numpy()], center_noise, scale_noise, self.inp_res, (float(self.W), float(self.H)))
        edges = np.concatenate([box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]])
        if B and (int(edges.max()) > HO3D_MAX_WINDOW or int(edges.min()) <= 0):       # the device cannot refuse a box: it would write zeros
            raise ValueError(f"HO-3D crop window of {int(edges.min())} .. {int(edges.max())} pixels: hifihr_ho3d_batch resamples boxes of "
                             f"1 .. {HO3D_MAX_WINDOW} pixels on an edge (include/hifihr.h)")
        slot, host = self._stage(8 * B)
        hv = host.numpy()
        hv[:B] = idxs.numpy().astype(np.int32)
        hv[B:5 * B] = box.reshape(-1)
        hv[5 * B:8 * B] = np.concatenate([center, scale[:, None]], 1).astype(np.float32).reshape(-1).view(np.int32)
        if _DIRECT_PARAMS:
            packed = host                          # read by the kernels straight from the pinned slot (FreiHandDeviceCache._packed_terms)
        else:
            packed = torch.empty(8 * B, dtype=torch.int32, device=self.device)
            packed.copy_(host, non_blocking=True)
        nws = self.lib.ho3d_workspace_bytes(B, self.inp_res)
        if self._ws is None or self._ws.numel() * 4 < nws:
            self._ws = torch.empty(nws // 4 + 1, dtype=torch.int32, device=self.device)
        S, dev = self.inp_res, self.device
        out = {"img_crop": torch.empty(B, 3, S, S, device=dev), "hand_mask_crop": torch.empty(B, 1, S, S, device=dev),
               "K_crop": torch.empty(B, 3, 3, device=dev), "uv21_crop": torch.empty(B, 21, 2, device=dev),
               "xyz21": torch.empty(B, 21, 3, device=dev)}
        self.lib.ho3d_batch(self.images, self.masks, self.Ks, self.uv21, self.xyz21, packed, B, S, self._ws, out)
        if self.open_2dj is not None:
            out["open_2dj_crop"] = torch.empty(B, 21, 2, device=dev)
            out["open_2dj_con"] = torch.empty((B,) + tuple(self.open_2dj_con.shape[1:]), device=dev)
            self.lib.ho3d_keypoints(self.open_2dj, self.open_2dj_con, packed, B, S, out["open_2dj_crop"], out["open_2dj_con"])
        if self.depth_u16 is not None:
            out["depth_crop"] = torch.empty(B, S, S, device=dev)
            self.lib.ho3d_depth_crop(self.depth_u16, packed, B, S, self.depth_scale, out["depth_crop"])
        self._release(slot)
        if self.root_xyz is not None:
            out["root_xyz"] = self.root_xyz[idxs.to(self.device)]
        return out
