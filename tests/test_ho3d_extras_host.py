"""Host-side checks of the HO-3D device-path extras (no GPU): the depth encoding helper, the float64 back-projection restatement against
the reference's own routine (tests/golden/depth_points.npz, made by tools/make_depth_points_golden.py from the reference's source), the
options key, and the wiring of traineval.data_dic -- there ops.depth_points runs the real kernel on the host emulator."""
import os

import numpy as np
import pytest
import torch

import ho3d_extras_cases as hc
import kernel_cases as kc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_points.npz")


def test_ho3d_depth_to_u16_round_trips_a_seeded_map():
    from hifihr_amd.data import HO3D_DEPTH_SCALE, ho3d_depth_to_u16
    rng = np.random.default_rng(2)
    want = rng.integers(0, 65536, (3, 17, 23)).astype(np.uint16)
    want[0, 0, :4] = [0, 255, 256, 65535]
    rgb = np.stack([rng.integers(0, 256, want.shape).astype(np.uint8), (want >> 8).astype(np.uint8), (want & 255).astype(np.uint8)], -1)
    got = ho3d_depth_to_u16(rgb)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert np.array_equal(ho3d_depth_to_u16(rgb[0]), want[0])
    assert HO3D_DEPTH_SCALE == 0.00012498664727900177
    with pytest.raises(ValueError):
        ho3d_depth_to_u16(rgb.astype(np.int32))


def test_restatement_agrees_with_the_references_back_projection():
    """Per pixel, for EVERY valid pixel of the golden file: z exactly, |x - x_ref| <= |x| (1e-5 / fx + 4 x 2^-24) and likewise y -- the
    reference's `fx + 1e-5` and its four float32 roundings (u - cx, (.) z, fx + 1e-5 with its reciprocal, the last product).  The
    restatement runs at c = 0, the reference's pixel convention."""
    g = np.load(GOLDEN)
    depths, Ks, uv = g["depths"], g["Ks"], g["uv_index"]
    assert (Ks[:, 0, 0] >= 100).all() and (Ks[:, 1, 1] >= 100).all() and depths.shape[1] == depths.shape[2]
    assert uv.shape[0] == int((depths > 0).sum()) and uv.shape[0] > 500, "no pixel is left out"
    seen = np.zeros(depths.shape, bool)
    seen[uv[:, 0], uv[:, 2], uv[:, 1]] = True                          # (sample, u, v): the map went in transposed
    assert np.array_equal(seen, depths > 0)
    worst = 0.0
    for b in range(depths.shape[0]):
        rows = uv[:, 0] == b
        u, v = uv[rows, 1], uv[rows, 2]
        d = depths[b, v, u]
        want = hc.backproject_ref(d, Ks[b], v, u, c=0.0)
        # z: the reference's is the depth itself; the restatement's (fx fy d) / (fx fy) in float64 is the depth once rounded to float32
        assert np.array_equal(g["z_gt"][rows], d) and np.array_equal(want[:, 2].astype(np.float32), d)
        for axis, ref, f in ((0, g["x_gt"][rows], Ks[b, 0, 0]), (1, g["y_gt"][rows], Ks[b, 1, 1])):
            bound = np.abs(want[:, axis]) * (1e-5 / float(f) + 4 * 2.0 ** -24)
            err = np.abs(ref.astype(np.float64) - want[:, axis])
            assert (err <= bound).all(), (b, axis, float((err - bound).max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"reference back-projection against the float64 restatement at c = 0: worst error / bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0


def test_depth_points_is_an_option_that_defaults_to_off():
    from hifihr_amd import losses, options
    assert options.make_args().depth_points == 0 and options.make_args(depth_points=1000).depth_points == 1000
    assert len(losses.TERMS) == 31


# ---- traineval.data_dic ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def emulated_ops(monkeypatch):
    """hifihr_amd.ops bound to the emulator library: ops.depth_points then runs csrc/depth_points.hip on host tensors."""
    from hifihr_amd import ops
    lib = kc.build_hostsim()
    monkeypatch.setattr(ops, "get_lib", lambda: lib)
    monkeypatch.setattr(ops, "require_cuda", lambda *t: None)
    return ops


def _ho3d_sample(B=2, S=16):
    rng = np.random.default_rng(8)
    K = np.asarray([[30.0, 0, 8.2], [0, 28.0, 7.6], [0, 0, 1.0]], np.float32) * np.asarray([1, -1, -1], np.float32)      # HO-3D's raw K
    depth = (0.4 + 0.3 * rng.random((B, S, S))).astype(np.float32)
    depth[rng.random((B, S, S)) < 0.3] = 0
    mask = (rng.random((B, 1, S, S)) < 0.6).astype(np.float32)
    xyz = np.concatenate([0.1 * rng.random((B, 21, 2)) - 0.05, -0.5 - 0.2 * rng.random((B, 21, 1))], -1).astype(np.float32)
    t = torch.from_numpy
    return {"img_crop": torch.rand(B, 3, S, S), "K_crop": t(np.tile(K, (B, 1, 1))), "xyz21": t(xyz), "hand_mask_crop": t(mask), "depth_crop": t(depth)}


@pytest.mark.parametrize("image_size", [16, 32])
def test_data_dic_builds_chamfer_points_from_the_depth_crop(emulated_ops, image_size):
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic
    s = _ho3d_sample()
    B, P = 2, 32
    off = data_dic(s, "HO3D", "training", options.make_args(), device="cpu", image_size=image_size)
    assert "chamfer_points" not in off and "depths" in off                                # the default 0: none
    args = options.make_args(depth_points=P)
    ex = data_dic(s, "HO3D", "training", args, device="cpu", image_size=image_size, generator=torch.Generator().manual_seed(1))
    assert set(ex) == set(off) | {"chamfer_points"} and all(torch.equal(ex[k], off[k]) for k in off)
    pts = ex["chamfer_points"]
    assert pts.shape == (B, P, 3) and pts.dtype == torch.float32 and bool(torch.isfinite(pts).all())
    again = data_dic(s, "HO3D", "training", args, device="cpu", image_size=image_size, generator=torch.Generator().manual_seed(1))
    assert torch.equal(again["chamfer_points"], pts)
    # every point, moved back by the root and projected through the K of the map it came from, sits on a pixel centre whose depth it
    # carries and which the hand mask keeps
    root = ex["joints"][:, args.ROOT]
    r = image_size / 16
    K = ex["Ks"].double() * torch.tensor([r, r, 1.0], dtype=torch.float64).view(1, 3, 1)
    p = pts.double() + root.double().unsqueeze(1)
    uvw = torch.einsum("bij,bpj->bpi", K, p)
    u, v = uvw[..., 0] / uvw[..., 2] - 0.5, uvw[..., 1] / uvw[..., 2] - 0.5
    q, rr = u.round().long(), v.round().long()
    assert float((u - q).abs().max()) < 1e-4 and float((v - rr).abs().max()) < 1e-4
    for b in range(B):
        assert bool((ex["masks"][b, 0, rr[b], q[b]] != 0).all())
        assert torch.allclose(ex["depths"][b, rr[b], q[b]].double(), p[b, :, 2], rtol=1e-6)
    # root_xyz stands in for the joints on the evaluation split
    ev = dict(s, root_xyz=ex["joints"][:, args.ROOT].clone())
    del ev["xyz21"]
    ex2 = data_dic(ev, "HO3D", "evaluation", args, device="cpu", image_size=image_size, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ex2["chamfer_points"], pts)


def test_a_callers_chamfer_points_win(emulated_ops):
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic
    own = torch.rand(2, 5, 3)
    ex = data_dic(dict(_ho3d_sample(), chamfer_points=own), "HO3D", "training", options.make_args(depth_points=32), device="cpu", image_size=16)
    assert torch.equal(ex["chamfer_points"], own)


def test_data_dic_without_a_depth_image_builds_nothing(emulated_ops):
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic
    s = _ho3d_sample()
    del s["depth_crop"]
    ex = data_dic(s, "HO3D", "training", options.make_args(depth_points=32), device="cpu", image_size=16)
    assert "chamfer_points" not in ex and "depths" not in ex


def test_freihand_branch_builds_points_from_depths(emulated_ops):
    """The FreiHand branch with a sample that carries `depths` (train_hrnet.py attaches the mesh's depth map there): K as it is, the mask's
    first channel, the root joint."""
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic
    B, S = 2, 16
    g = torch.Generator().manual_seed(4)
    K = torch.tensor([[30.0, 0, 8.0], [0, 30.0, 8.0], [0, 0, 1.0]]).repeat(B, 1, 1)
    joints = torch.cat([0.1 * torch.rand(B, 21, 2, generator=g) - 0.05, 0.5 + 0.2 * torch.rand(B, 21, 1, generator=g)], -1)
    depths = 0.5 + 0.1 * torch.rand(B, S, S, generator=g)
    masks = (torch.rand(B, 3, S, S, generator=g) < 0.5).float()
    s = {"trans_images": torch.rand(B, 3, S, S), "trans_Ks": K, "trans_joints": joints, "trans_verts": joints[:, :4].clone(), "trans_masks": masks,
         "scales": torch.ones(B), "idxs": torch.arange(B), "depths": depths}
    args = options.make_args(depth_points=8)
    ex = data_dic(s, "FreiHand", "training", args, device="cpu", generator=torch.Generator().manual_seed(2))
    pts = ex["chamfer_points"].double() + joints[:, args.ROOT].double().unsqueeze(1)
    uvw = torch.einsum("bij,bpj->bpi", K.double(), pts)
    q, r = (uvw[..., 0] / uvw[..., 2] - 0.5).round().long(), (uvw[..., 1] / uvw[..., 2] - 0.5).round().long()
    for b in range(B):
        assert bool((masks[b, 0, r[b], q[b]] != 0).all()) and torch.allclose(depths[b, r[b], q[b]].double(), pts[b, :, 2], rtol=1e-6)
    assert "chamfer_points" not in data_dic(s, "FreiHand", "training", options.make_args(), device="cpu")


def test_train_hrnet_helpers():
    import sys
    sys.path.insert(0, kc.REPO)
    import train_hrnet as T
    from hifihr_amd import options
    assert not T.wants_depth_points(options.make_args(losses=["chamfer"]))
    assert not T.wants_depth_points(options.make_args(losses=["joint_3d"], depth_points=64))
    assert T.wants_depth_points(options.make_args(losses=["joint_3d", "point_mesh"], depth_points=64))
    z = {"images": 0, "open_2dj": 1, "open_2dj_con": 2, "depth_u16": 3}
    assert T.ho3d_optional_arrays(z) == {"open_2dj": 1, "open_2dj_con": 2, "depth_u16": 3}
    assert T.ho3d_optional_arrays({"images": 0, "open_2dj": 1}) == {}
