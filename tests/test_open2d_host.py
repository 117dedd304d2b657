"""Host side of the self-supervised keypoint terms (no GPU): the float64 restatement of tests/open2d_ref.py against what the reference's
own code gives (tests/golden/open2d.npz, tools/make_open2d_golden.py), the options, the names, `data_dic` on CPU tensors and the message
a requested term without its inputs fails with."""
import os
import types

import numpy as np
import pytest
import torch

import open2d_cases as oc
import open2d_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "open2d.npz")

# the `losses` lists of the reference's self-supervised configs (a config that sets `semi_ratio` is one of these with that key added)
SELF_SUPERV_LOSSES = {
    "config/FreiHAND/self_superv_freihand_w_texture.json": ["open_2dj", "mpose", "mshape", "mtex", "open_bone_direc", "texture_self", "mrgb_self",
                                                            "ssim_tex_self", "perceptual"],
    "config/FreiHAND/self_superv_freihand_no_texture.json": ["open_2dj", "mpose", "mshape", "mtex", "open_bone_direc"],
    "config/FreiHAND/test.json": ["open_2dj", "mpose", "mshape", "mtex", "open_bone_direc"],
    "config/HO3D/self_superv_ho3d_w_texture.json": ["open_2dj", "mpose", "mshape", "mtex", "open_bone_direc", "texture_self", "mrgb_self",
                                                    "ssim_tex_self"],
    "config/HO3D/self_superv_ho3d_no_texture.json": ["open_2dj", "mpose", "mshape", "mtex", "open_bone_direc"],
    "semi_ratio": ["open_2dj", "mpose", "mshape", "mtex", "open_bone_direc", "texture_self", "mrgb_self", "ssim_tex_self", "perceptual"],
}

U = 2.0 ** -24        # unit roundoff of float32: one rounding changes a value by at most U times its magnitude


def test_restatement_reproduces_the_reference():
    """The fixture is the reference's float32 evaluation; the restatement runs in float64 on the same float32 inputs, so the difference is
    the fixture's own rounding.  Every bound below counts the float32 roundings of the reference's evaluation (first order in U):
      rho(d)          dx, dy (1 U each); their squares (3 U); the sum (4 U); the square root halves that and rounds (3 U); d - 2.5 with
                      d <= 2 (d - 2.5) for d >= 5 (7 U), or d^2 / 10 (8 U); the one-hot weight w^2 is exact and cancels in one division: 9 U
      rho (c w)^2     c w (1 U), squared (3 U), times rho (9 U + 1 U): 13 U
      a sum of n non-negative addends adds at most (n - 1) U whatever its order; a ratio adds its two errors and 1 U:
      open_2dj        n = 5 x 21 = 105: numerator (13 + 104) U, denominator (3 + 104) U, ratio 225 U; one sample, n = 21: (33 + 23 + 1) U = 57 U
      open_2dj_de     210 squared differences of 3 U each, 209 U for the sum, 1 U for the mean: 213 U
      bone terms      ABSOLUTE (vn - von cancels): a unit-vector component is v / (|v| + 1e-4), v 1 U, |v| 3 U, + 1e-4 1 U, the division
                      1 U: 6 U of a value <= 1; the difference of two 12 U + 1 U |dn| <= 14 U; its square 2 |dn| 14 U + U dn^2 <= 60 U with
                      |dn| <= 2; two of them 120 U + 4 U = 124 U; the mean over 20 with 19 zeros and the factor 20 back: 2 U t <= 8 U: 132 U
      open_bone_direc addend t c_p c_c: 124 U + 2 U t <= 132 U absolute; the mean of n of them: 132 U + n U value (n = 100; one sample: 20)"""
    g = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(g[k]).double()
    j2d, det, con = t("j2d"), t("open_2dj"), t("open_2dj_con")
    assert j2d.shape == (5, 21, 2) and con.shape == (5, 21, 1) and g["j2d"].dtype == np.float32
    d = ref.norm2(det - j2d)
    assert bool((d < 5).any()) and bool((d > 5).any()) and bool((con == 0).any())              # both branches of rho, missed joints
    rel = lambda got, want: float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())
    assert rel(t("rho"), ref.rho(d)) <= 9 * U
    num, den = ref.joint_pieces(j2d, det, con)
    live = num > 0
    assert bool((t("joint_addends")[~live] == 0).all()) and rel(t("joint_addends")[live], num[live]) <= 13 * U
    assert rel(t("sample_open_2dj"), num.sum(1) / den.sum(1)) <= 57 * U
    bt, cc = ref.bone_pieces(j2d, det, con)
    assert float((t("bone_terms") - bt).abs().max()) <= 132 * U
    per = (bt * cc).mean(1)
    assert bool(((t("sample_bone_direc") - per).abs() <= 132 * U + 20 * U * per).all())
    out = ref.terms(j2d, det, con)
    want = t("terms")
    assert abs(float(out[0] - want[0])) <= 225 * U * float(out[0])
    assert abs(float(out[1] - want[1])) <= 132 * U + 100 * U * float(out[1])
    assert abs(float(out[2] - want[2])) <= 213 * U * float(out[2])


def test_names_options_and_reference_configs():
    from hifihr_amd import losses, ops, options
    assert ops.OPEN2D_TERMS == ("open_2dj", "open_bone_direc", "open_2dj_de") and set(ops.OPEN2D_TERMS) <= set(losses.TERMS)
    for name, lst in SELF_SUPERV_LOSSES.items():
        assert [k for k in lst if k not in losses.TERMS] == [], name
    a = options.make_args()
    assert a.lambda_j2d == 1e-3 and a.lambda_j2d_de == 1e-4 and a.semi_ratio is None            # options/train_options.py:108, 112, 165
    assert not any(k in a.losses for k in ops.OPEN2D_TERMS)
    cfg = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "self_superv_style_config.json")
    assert options.make_args(cfg).losses == SELF_SUPERV_LOSSES["config/FreiHAND/self_superv_freihand_w_texture.json"]


@pytest.mark.parametrize("missing", ["open_2dj", "open_2dj_con", "j2d"])
def test_a_requested_term_without_its_inputs_says_what_it_needs(missing):
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    ex = {"open_2dj": torch.zeros(2, 21, 2), "open_2dj_con": torch.ones(2, 21, 1)}
    out = {"j2d": torch.zeros(2, 21, 2)}
    (out if missing == "j2d" else ex).pop(missing)
    with pytest.raises(AssertionError, match="need examples\\['open_2dj'\\] and examples\\['open_2dj_con'\\]"):
        LossFunction()(ex, out, ["open_bone_direc"], "FreiHand", options.make_args())


def test_cpu_tensors_are_refused_not_computed_elsewhere():
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    ex = {"open_2dj": torch.zeros(2, 21, 2), "open_2dj_con": torch.ones(2, 21, 1)}
    with pytest.raises(Exception) as e:
        LossFunction()(ex, {"j2d": torch.zeros(2, 21, 2)}, ["open_2dj"], "FreiHand", options.make_args())
    assert not isinstance(e.value, (AssertionError, KeyError))


# ---- data_dic on CPU tensors: the checks tests/open2d_cases.py makes of the device launch -------------------------------------------
def _sample(B, semi, warped):
    det, con = oc.keypoint_cache()
    idx, total, _ = oc.keypoint_inputs(B, "random", semi)
    g = torch.Generator().manual_seed(B)
    joints = torch.cat([0.1 * torch.rand(B, 21, 2, generator=g) - 0.05, 0.5 + 0.2 * torch.rand(B, 21, 1, generator=g)], -1)
    K = torch.tensor([[500.0, 0, 112], [0, 500.0, 112], [0, 0, 1]]).repeat(B, 1, 1)
    s = {"trans_images": torch.zeros(B, 3, 8, 8), "trans_Ks": K, "trans_joints": joints, "idxs": idx, "open_2dj_con": con[idx]}
    s["trans_open_2dj" if warped else "open_2dj"] = det[idx]
    if warped:
        s["open_2dj"] = torch.full_like(det[idx], -1.0)                  # the warped detections win
    return s, det[idx], con[idx], idx


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("semi", [None, 0.5])
@pytest.mark.parametrize("warped", [False, True])
def test_data_dic_freihand_branch(B, semi, warped):
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic, proj_func
    s, det, con, idx = _sample(B, semi, warped)
    ex = data_dic(s, "FreiHand", "training", options.make_args(semi_ratio=semi), device="cpu")
    j2d_gt = proj_func(s["trans_joints"], s["trans_Ks"])
    want_det, want_con = ref.semi_mix(det, con, j2d_gt, idx, semi)
    assert torch.equal(ex["open_2dj"], want_det) and torch.equal(ex["open_2dj_con"], want_con) and ex["open_2dj_con"].shape == (B, 21, 1)
    if B > 1 and semi:
        pick = ref.semi_choice(idx, semi)
        assert bool(pick.any()) and not bool(pick.all())
    tex = ref.texture_con(con.double(), idx)
    assert ex["texture_con"].shape == (B,) and torch.equal(ex["texture_con"] > 0, con.reshape(B, 21).min(1)[0] > np.float32(0.1))
    assert bool(((ex["texture_con"].double() - tex).abs() <= oc.TEX_ROUNDINGS * U * tex.abs()).all())
    # evaluation batches are never mixed
    ev = data_dic({**{k.replace("trans_", ""): v for k, v in s.items()}, "open_2dj": det}, "FreiHand", "evaluation",
                  options.make_args(semi_ratio=semi), device="cpu")
    assert torch.equal(ev["open_2dj"], det) and torch.equal(ev["open_2dj_con"], con)


def test_data_dic_without_detections_is_unchanged_and_flat_confidences_pass():
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic
    s, det, con, idx = _sample(3, 0.5, False)
    bare = {k: v for k, v in s.items() if not k.startswith("open_2dj")}
    assert set(data_dic(bare, "FreiHand", "training", options.make_args(semi_ratio=0.5), device="cpu")) == {"imgs", "idxs", "Ks", "Ps", "joints", "j2d_gt"}
    ex = data_dic(dict(s, open_2dj_con=con.view(3, 21)), "FreiHand", "training", options.make_args(semi_ratio=0.5), device="cpu")
    assert ex["open_2dj_con"].shape == (3, 21) and torch.equal(ex["open_2dj_con"], ref.semi_mix(det, con.view(3, 21), ex["j2d_gt"], idx, 0.5)[1])


def test_data_dic_ho3d_branch():
    from hifihr_amd import options
    from hifihr_amd.traineval import data_dic
    g = torch.Generator().manual_seed(3)
    B = 4
    s = {"img_crop": torch.zeros(B, 3, 8, 8), "K_crop": torch.eye(3).repeat(B, 1, 1), "open_2dj_crop": 224 * torch.rand(B, 21, 2, generator=g),
         "open_2dj_con": torch.rand(B, 21, 1, generator=g)}
    ex = data_dic(s, "HO3D", "training", options.make_args(), device="cpu", image_size=8)
    assert torch.equal(ex["open_2dj"], s["open_2dj_crop"]) and torch.equal(ex["open_2dj_con"], s["open_2dj_con"])
    want = s["open_2dj_con"].double().reshape(B, 21).mean(1)                                    # utils/traineval_util.py:191
    assert bool(((ex["texture_con"].double() - want).abs() <= oc.TEX_ROUNDINGS * U * want).all())
    s.pop("open_2dj_crop")
    assert "open_2dj" not in data_dic(s, "HO3D", "training", options.make_args(), device="cpu", image_size=8)


def test_synthetic_keypoint_files_load(tmp_path):
    """--openpose_keypoints: the reference's [keypoints, confidences] layout, confidences as [n][21] or [n][21][1]."""
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train_hrnet as T
    rng = np.random.default_rng(0)
    det, con = rng.random((6, 21, 2)).astype(np.float32), rng.random((6, 21)).astype(np.float32)
    for c in (con, con[..., None]):
        f = tmp_path / "kp.json"
        f.write_text(json.dumps([det.tolist(), c.tolist()]))
        got_det, got_con = T.load_openpose_keypoints(str(f), 4)
        assert got_det.shape == (4, 21, 2) and got_con.shape == (4, 21, 1)
        assert np.array_equal(got_det, det[:4]) and np.array_equal(got_con[..., 0], con[:4])
    with pytest.raises(ValueError):
        T.load_openpose_keypoints(str(f), 7)
    args = types.SimpleNamespace(losses=["mpose", "mrgb_self"])
    assert T.wants_keypoints(args) and not T.wants_keypoints(types.SimpleNamespace(losses=["mpose", "texture"]))
