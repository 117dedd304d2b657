"""The HO-3D device-path extras on the MI355X: hifihr_ho3d_keypoints, hifihr_ho3d_depth_crop and hifihr_depth_points through the C ABI on
the cases of tests/test_hostsim_ho3d_extras.py (tests/ho3d_extras_cases.py), and the Python surface end to end: HO3DDeviceCache with
detections and depth frames, ops.depth_points, the synthetic frames, train_hrnet.py --dataset HO3D on the self-supervised style config, on
depth + point_mesh with depth_points, and an evaluation pass that fits to the detections."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import ho3d_extras_cases as hc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


@pytest.mark.parametrize("case", hc.DET_CASES, ids=_ids)
def test_detections_go_through_the_crop_window(lib, case):
    hc.detections_case(lib, "cuda", *case)


def test_keypoint_refusals_and_indices_outside_the_cache(lib):
    hc.keypoints_refusal_case(lib, "cuda")


@pytest.mark.parametrize("S", hc.DEPTH_SIZES)
@pytest.mark.parametrize("frame", hc.DEPTH_FRAMES, ids=_ids)
def test_depth_crop_is_pillows_nearest_resize(lib, frame, S):
    hc.depth_crop_case(lib, "cuda", *frame, S)


def test_depth_crop_refusals(lib):
    hc.depth_crop_refusal_case(lib, "cuda")


@pytest.mark.parametrize("P", hc.SELECT_P)
@pytest.mark.parametrize("shape", hc.SELECT_SHAPES, ids=_ids)
def test_point_selection_matches_the_restatement(lib, shape, P):
    hc.selection_case(lib, "cuda", *shape, P)


@pytest.mark.parametrize("with_origin", [False, True])
@pytest.mark.parametrize("kind", hc.K_KINDS)
def test_back_projection_matches_float64(lib, kind, with_origin):
    hc.backprojection_case(lib, "cuda", kind, with_origin)


def test_depth_points_refusals(lib):
    hc.depth_points_refusal_case(lib, "cuda")


def test_closed_loop_points_lie_on_the_rendered_mesh(lib):
    """Measured on an MI355X: profiles/depth_points_precision.txt."""
    from hifihr_amd import evaluate
    dev = torch.device("cuda")

    def surface(p, v, faces):
        return float(evaluate.point_to_surface(torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(faces)).to(dev),
                                               torch.from_numpy(p).to(dev))[0])
    hc.closed_loop_case(lib, "cuda", surface)


def test_ops_surface_renders_and_back_projects_the_same_points(lib):
    """ops.render + ops.render_depth + ops.depth_points on the closed loop's scene: the public functions give the C ABI's bits."""
    from hifihr_amd import ops
    dev = torch.device("cuda")
    verts, faces, K = hc.loop_scene()
    S = hc.LOOP_SIZE
    cam = hc.camera_from_K(K, S).to(dev)
    r = ops.RendererHandle(faces, verts.shape[1], image_size=S, aa=1)
    v = verts.to(dev)
    _, fid = ops.render(r, v, torch.ones(verts.shape[1], 3, device=dev), cam, torch.zeros(1, 3, device=dev),
                        torch.tensor([[0.0, 0.0, -1.0]], device=dev))
    depth, hits = ops.render_depth(r, v, cam, fid)
    n = int((hits > 0).sum())
    draws = torch.from_numpy(hc.every_pixel_draws(n)[None]).to(dev)
    Kt = torch.from_numpy(K).to(dev)
    pts, cnt, idx = ops.depth_points(depth, Kt, n, mask=hits > 0, draws=draws, return_index=True)
    want = hc.run_depth_points(lib, "cuda", depth[:, 0].cpu().numpy(), K[None], (hits > 0).float().cpu().numpy(), draws.cpu().numpy(), None)
    assert int(cnt[0]) == n and np.array_equal(idx.cpu().numpy(), want[2]) and np.array_equal(pts.cpu().numpy().view(np.int32), want[0].view(np.int32))
    # int64 masks (segms_gt), an origin, a [3,3] K, seeded draws: the same generator gives the same points
    root = torch.tensor([[0.1, -0.2, 11.0]], device=dev)
    a = ops.depth_points(depth, Kt, 64, mask=(hits > 0).long(), origin=root, generator=torch.Generator().manual_seed(3))
    b = ops.depth_points(depth[:, 0], Kt[None], 64, mask=(hits > 0).float()[:, None], origin=root[:, None], generator=torch.Generator().manual_seed(3))
    assert a[0].shape == (1, 64, 3) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not a[0].requires_grad
    free = ops.depth_points(depth, Kt, 64, mask=hits > 0)[0]
    assert bool(torch.isfinite(free).all()) and float((free[..., 2] - hc.LOOP_Z).abs().max()) < 1.0


# ---- the device data path ------------------------------------------------------------------------------------------------------------
_N, _FH, _FW, _S = 3, 48, 64, 16


def _frames(con3=True):
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (_N, _FH, _FW, 3)).astype(np.uint8)
    masks = (rng.random((_N, _FH, _FW)) < 0.5).astype(np.uint8) * 255
    Ks = np.tile(np.asarray([[40.0, 0, 30.0], [0, 40.0, 22.0], [0, 0, 1.0]], np.float32), (_N, 1, 1))
    xyz = np.concatenate([0.3 * rng.random((_N, 21, 2)) - 0.15, 0.5 + 0.2 * rng.random((_N, 21, 1))], -1).astype(np.float32)
    det = (rng.random((_N, 21, 2)) * [_FW, _FH]).astype(np.float32)
    con = rng.random((_N, 21, 1) if con3 else (_N, 21)).astype(np.float32)
    return imgs, masks, Ks, xyz, det, con, hc.depth_frames(_N, _FH, _FW, 9)


def _entries(cache, call):
    """The C entries `call` runs through cache.lib, in order."""
    seen, run = [], cache.lib._run
    cache.lib._run = lambda entry, *a, **k: (seen.append(entry), run(entry, *a, **k))[1]
    try:
        out = call()
    finally:
        del cache.lib._run
    return seen, out


@pytest.mark.parametrize("B,con3", [(1, True), (3, False)])
def test_device_cache_with_and_without_the_extras(B, con3):
    from hifihr_amd.data import HO3D_DEPTH_SCALE, HO3DDeviceCache, ho3d_crop_windows
    imgs, masks, Ks, xyz, det, con, d16 = _frames(con3)
    idx = [2] if B == 1 else [1, 0, 1]
    noise = dict(center_noise=np.asarray([[1.5, -2.0]] * B, np.float32), scale_noise=np.asarray([0.93] * B, np.float32))
    plain = HO3DDeviceCache(imgs, masks, Ks, xyz, inp_res=_S)
    seen, base = _entries(plain, lambda: plain.batch(idx, **noise))
    assert tuple(base) == ("img_crop", "hand_mask_crop", "K_crop", "uv21_crop", "xyz21") and seen == ["hifihr_ho3d_batch"]      # exactly the old dict
    both = HO3DDeviceCache(imgs, masks, Ks, xyz, inp_res=_S, open_2dj=det, open_2dj_con=con, depth_u16=d16)
    seen, got = _entries(both, lambda: both.batch(idx, **noise))
    assert seen == ["hifihr_ho3d_batch", "hifihr_ho3d_keypoints", "hifihr_ho3d_depth_crop"]
    assert tuple(got) == tuple(base) + HO3DDeviceCache.KEYPOINT_KEYS + HO3DDeviceCache.DEPTH_KEYS
    for k in base:
        assert torch.equal(got[k], base[k]), k
    center, scale, _, box = ho3d_crop_windows(plain.uv21_host[idx], noise["center_noise"], noise["scale_noise"], _S, (float(_FW), float(_FH)))
    want = hc.crop_window_ref(det, np.asarray(idx), center, scale, _S)
    assert np.array_equal(got["open_2dj_crop"].cpu().numpy().view(np.int32), want.view(np.int32))
    assert got["open_2dj_con"].shape == (B,) + con.shape[1:] and np.array_equal(got["open_2dj_con"].cpu().numpy(), con[idx])
    assert got["depth_crop"].shape == (B, _S, _S) and got["depth_crop"].dtype == torch.float32
    assert np.array_equal(got["depth_crop"].cpu().numpy(), hc.depth_crop_formula(d16, idx, box, _S, HO3D_DEPTH_SCALE))
    assert float(got["depth_crop"].max()) > 0
    # the projected joints as detections: uv21_crop's bits
    same = HO3DDeviceCache(imgs, masks, Ks, xyz, inp_res=_S, open_2dj=plain.uv21_host, open_2dj_con=con)
    out = same.batch(idx, **noise)
    assert tuple(out) == tuple(base) + HO3DDeviceCache.KEYPOINT_KEYS and torch.equal(out["open_2dj_crop"], out["uv21_crop"])
    # each extra alone
    only_d = HO3DDeviceCache(imgs, masks, Ks, xyz, inp_res=_S, depth_u16=torch.from_numpy(d16), depth_scale=0.5).batch(idx, **noise)
    assert tuple(only_d) == tuple(base) + HO3DDeviceCache.DEPTH_KEYS
    assert np.array_equal(only_d["depth_crop"].cpu().numpy(), hc.depth_crop_formula(d16, idx, box, _S, 0.5))
    torch.cuda.synchronize()


def test_device_cache_refuses_half_a_pair_and_wrong_shapes():
    from hifihr_amd.data import HO3DDeviceCache
    imgs, masks, Ks, xyz, det, con, d16 = _frames()
    for kw in (dict(open_2dj=det), dict(open_2dj_con=con), dict(open_2dj=det, open_2dj_con=con[:, :20]), dict(open_2dj=det[:2], open_2dj_con=con),
               dict(depth_u16=d16[:, :-1]), dict(depth_u16=d16.astype(np.int32))):
        with pytest.raises(ValueError):
            HO3DDeviceCache(imgs, masks, Ks, xyz, inp_res=_S, **kw)


def test_synthetic_frames_carry_detections_and_depth(synth_tables):
    from hifihr_amd import ops, synth
    from hifihr_amd.data import HO3D_DEPTH_SCALE
    dev = torch.device("cuda")
    mano, rend = ops.ManoLayerHandle(synth_tables), ops.RendererHandle(synth_tables.faces, 778, image_size=224, aa=3)
    plain = synth.make_ho3d_frames(mano, rend, 4, device=dev)
    full = synth.make_ho3d_frames(mano, rend, 4, device=dev, depth=True, open_2dj=True)
    assert tuple(plain) == ("images_u8", "hand_masks_u8", "Ks", "xyz21")
    assert set(full) == set(plain) | {"depths", "depth_u16", "open_2dj", "open_2dj_con"} and all(torch.equal(full[k], plain[k]) for k in plain)
    assert full["open_2dj"].shape == (4, 21, 2) and full["open_2dj_con"].shape == (4, 21, 1) and full["depth_u16"].dtype == torch.uint16
    # the detections are the projected joints (FreiHAND order) + 2 px of noise
    from hifihr_amd.traineval import HO3D2Frei
    uvw = torch.einsum("nij,nkj->nki", full["Ks"], full["xyz21"])
    noise = full["open_2dj"] - HO3D2Frei(uvw[..., :2] / uvw[..., 2:3])
    assert 1.2 < float(noise.std()) < 2.8
    back = full["depth_u16"].to(torch.int32).float() * HO3D_DEPTH_SCALE
    assert float((back - full["depths"]).abs().max()) <= 0.5 * HO3D_DEPTH_SCALE * 1.001 and int((full["depth_u16"].to(torch.int32) > 0).sum()) > 1000


# ---- train_hrnet.py --dataset HO3D ---------------------------------------------------------------------------------------------------
def _main(tmp_path, cfg, *cli, dataset="HO3D"):
    sys.path.insert(0, ROOT)
    import train_hrnet as T
    cfg = dict(cfg, base_out_path=str(tmp_path / "run"))
    f = tmp_path / "cfg.json"
    f.write_text(json.dumps(cfg))
    prev = torch.cuda.current_stream()
    try:
        return T.main(["--config_json", str(f), "--dataset", dataset, "--synthetic_size", "16", "--print_freq", "1", *cli])
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)


def _style_config():
    return json.load(open(os.path.join(ROOT, "tests", "data", "self_superv_ho3d_style_config.json")))


def test_train_hrnet_on_the_ho3d_self_supervised_style_config(tmp_path, capsys):
    """The loss list of the reference's config/HO3D/self_superv_ho3d_no_texture.json on synthetic HO-3D frames: on the parent the first batch
    dies in _open2d's assert (the batches carried no detections)."""
    assert _main(tmp_path, _style_config(), "--max_iters", "3") == 0
    out = capsys.readouterr().out
    assert "open_2dj=" in out and "open_bone_direc=" in out and "mpose=" in out and "mshape=" in out and "Done!" in out and "nan" not in out.lower()


def test_train_hrnet_on_ho3d_depth_and_point_mesh(tmp_path, capsys):
    """depth + point_mesh from the cropped depth frames: `depths` from HO3DDeviceCache(depth_u16=...), `chamfer_points` from ops.depth_points
    (depth_points = 64).  On the parent train_ho3d stops: "decoding and cropping HO-3D depth images is not built"."""
    cfg = dict(_style_config(), hand_model="mano", losses=["joint_3d", "mpose", "mshape", "depth", "point_mesh"], render_depth=True, depth_points=64)
    assert _main(tmp_path, cfg, "--max_iters", "3", "--graph", "0") == 0
    out = capsys.readouterr().out
    assert "depth=" in out and "point_mesh=" in out and "Done!" in out and "nan" not in out.lower() and "inf" not in out.lower().replace("info", "")
    import re
    vals = [float(v) for k in ("depth", "point_mesh") for v in re.findall(rf"\b{k}=([-+0-9.eE]+)", out)]
    assert len(vals) >= 6 and all(np.isfinite(vals)) and any(v > 0 for v in vals)


def test_ho3d_evaluation_fits_to_the_detections(tmp_path, capsys):
    """An evaluation-only pass with fit_keypoints: the batches of the HO-3D evaluation split now carry open_2dj, so the pass refines (on the
    parent it logs that no batch carried the target)."""
    cfg = dict(_style_config(), hand_model="mano", mode=["evaluation"], losses=["joint_3d", "mpose", "mshape"], fit_keypoints=True, fit_iters=8)
    assert _main(tmp_path, cfg) == 0
    out = capsys.readouterr().out
    assert "REFINED by 8 fit iterations against 'open_2dj' in 4 batches" in out and "[train_hrnet] HO3D evaluation:" in out


def test_train_hrnet_freihand_builds_points_from_the_mesh_depth(tmp_path, capsys):
    """The FreiHAND path: the ground-truth mesh's depth map stands in for a depth image (attach_mesh_depths) and, with depth_points, its
    back-projection is the target of point_mesh instead of the vertices -- in the captured step, written into its static input."""
    cfg = dict(_style_config(), train_datasets=["FreiHand"], hand_model="mano", losses=["joint_3d", "mpose", "mshape", "point_mesh"], depth_points=64)
    assert _main(tmp_path, cfg, "--max_iters", "3", dataset="FreiHand") == 0
    out = capsys.readouterr().out
    assert "point_mesh=" in out and "Done!" in out and "nan" not in out.lower()
