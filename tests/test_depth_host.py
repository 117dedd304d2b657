"""Host-only checks of the depth map and its loss (no kernel runs): the restatements of tests/depth_ref.py against the C rasteriser and
against each other, the options, the front end, the loss name and its assert, the Evaluator's keyword, the data path's pass-through and
the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import depth_cases as dc
import depth_ref as dr


@pytest.mark.parametrize("kind", dc.KINDS)
def test_float32_restatement_is_the_oracle_zbuf_at_aa1(kind):
    """The restatement mirrors oracle/raster_oracle.c's expression order: at one sample per pixel its depth has the bits of the zbuf."""
    verts, faces, cam = dc.scene(kind)
    for H in (8, 9, 17, 48):
        p2f, zbuf = dc.oracle_raster(verts, cam, faces, H)
        depth, hits, _ = dr.depth_f32(verts.numpy(), cam.numpy(), faces, p2f, H, 1)
        want = np.where(p2f >= 0, zbuf, np.float32(0)).astype(np.float32)
        assert np.array_equal(depth.view(np.int32), want.view(np.int32)) and np.array_equal(hits, (p2f >= 0).astype(np.int32))


def test_restatements_agree_and_average_only_covered_samples():
    H, aa, B, F, seed = 9, 3, 2, 12, 2
    verts, faces, cam, _ = dc.grad_inputs(H, aa, B, F, seed)
    p2f, zbuf = dc.oracle_raster(verts, cam, faces.numpy(), H * aa)
    depth, hits, clamped = dr.depth_f32(verts.numpy(), cam.numpy(), faces.numpy(), p2f, H, aa)
    assert clamped == 0 and 0 < int((hits > 0).sum()) and int(((hits > 0) & (hits < aa * aa)).sum()) > 0, "no partly covered pixel"
    z = np.where(p2f >= 0, zbuf, 0).astype(np.float64).reshape(B, H, aa, H, aa).sum(axis=(2, 4))
    mean = np.where(hits > 0, z / np.maximum(hits, 1), 0.0)
    assert np.abs(depth - mean).max() <= 1e-6                         # the background (zbuf = -1) is not in the average
    d64 = dr.depth_torch(verts.double(), cam, faces, p2f, hits, H, aa)
    assert float((d64 - torch.as_tensor(mean)).abs().max()) <= 1e-6


def test_ordered_loss_sums_are_the_plain_sums():
    d, hits, D, mask, trunc = dc.loss_inputs(3, 300, "mixed")
    for t in (0.0, trunc):
        s = dr.loss_sums_ordered(d.numpy(), hits.numpy(), D.numpy(), mask.numpy(), t)
        ok, e = dr.loss_valid(d.numpy(), hits.numpy(), D.numpy(), mask.numpy(), t)
        assert np.array_equal(s[:, 1], ok.sum(1).astype(np.float64))
        assert np.abs(s[:, 0] - np.where(ok, np.abs(e), 0).sum(1)).max() <= 1e-12


def test_options_default_and_override():
    from hifihr_amd import options
    a = options.make_args()
    assert (a.render_depth, a.lambda_depth, a.depth_trunc, a.depth_metric) == (False, 1.0, 0.0, False) and "depth" not in a.losses
    b = options.make_args(render_depth=True, lambda_depth=10.0, depth_trunc=0.03, depth_metric=True)
    assert (b.render_depth, b.lambda_depth, b.depth_trunc, b.depth_metric) == (True, 10.0, 0.03, True)
    assert "depth" not in options.baseline_config2_args().losses and options.baseline_config2_args().render_depth is False


def test_front_end_switches_the_option_on():
    import train_hrnet
    from hifihr_amd import options
    a = options.make_args()
    assert train_hrnet.render_depth_kwargs(a) == dict(render_depth=False)
    assert train_hrnet.render_depth_kwargs(options.make_args(render_depth=True)) == dict(render_depth=True)
    assert train_hrnet.render_depth_kwargs(options.make_args(losses=a.losses + ["depth"])) == dict(render_depth=True)
    assert train_hrnet.render_depth_kwargs(options.make_args(depth_metric=True)) == dict(render_depth=True)
    assert train_hrnet.build_args(train_hrnet.parse(["--render_depth"])).render_depth is True
    assert train_hrnet.build_args(train_hrnet.parse([])).render_depth is False
    assert train_hrnet.wants_depths(a) is False and train_hrnet.wants_depths(options.make_args(depth_metric=True)) is True
    assert train_hrnet.wants_depths(options.make_args(losses=["depth"])) is True


def test_loss_function_needs_the_model_option():
    from hifihr_amd import losses, options
    assert "depth" in losses.TERMS
    args = options.make_args()
    ex = {"segms_gt": torch.zeros(1, 4, 4, dtype=torch.int64), "depths": torch.zeros(1, 4, 4)}
    with pytest.raises(AssertionError, match="render_depth"):
        losses.LossFunction()(ex, {}, ["depth"], "FreiHand", args)
    assert losses.LossFunction()(ex, {}, [], "FreiHand", args) == {}


def test_the_loss_name_reaches_the_kernels():
    """With the model's outputs present the term goes to ops.depth_loss, which has no CPU path."""
    from hifihr_amd import losses, options
    from hifihr_amd._lib import HifihrError
    ex = {"segms_gt": torch.ones(1, 4, 4, dtype=torch.int64), "depths": torch.ones(1, 4, 4)}
    out = {"re_depth": torch.ones(1, 1, 4, 4), "_re_depth_hits": torch.ones(1, 4, 4, dtype=torch.int32)}
    with pytest.raises(HifihrError):
        losses.LossFunction()(ex, out, ["depth"], "FreiHand", options.make_args())


def test_ops_refuse_cpu_tensors():
    from hifihr_amd import evaluate, ops
    from hifihr_amd._lib import HifihrError
    d, h, D = torch.ones(1, 1, 4, 4), torch.ones(1, 4, 4, dtype=torch.int32), torch.ones(1, 4, 4)
    with pytest.raises(HifihrError):
        ops.render_depth(None, torch.zeros(1, 4, 3), torch.zeros(1, 4), torch.zeros(1, 4, 4, dtype=torch.int32))
    for fn in (ops.depth_loss, ops.depth_loss_sums, evaluate.depth_error):
        with pytest.raises(HifihrError):
            fn(d, h, D)


def test_evaluator_keyword():
    import train_hrnet
    from hifihr_amd import evaluate, options
    assert evaluate.Evaluator().depth is False and evaluate.Evaluator(depth=True).depth is True
    assert evaluate.Evaluator(depth=True).summary() == {}
    assert train_hrnet.make_evaluator(options.make_args(), "cpu").depth is False
    assert train_hrnet.make_evaluator(options.make_args(depth_metric=True), "cpu").depth is True
    with pytest.raises(ValueError, match="render_depth"):
        evaluate.Evaluator(depth=True).collect({"joints": torch.zeros(1, 21, 3), "mano_verts": torch.zeros(1, 778, 3)}, {}, "FreiHand")


def test_data_path_passes_depths_through():
    from hifihr_amd import options, synth
    from hifihr_amd.traineval import data_dic
    B, H = 2, 224
    sample = {"trans_images": torch.rand(B, 3, H, H), "trans_Ks": torch.eye(3).repeat(B, 1, 1), "trans_joints": torch.rand(B, 21, 3) + 0.5,
              "trans_verts": torch.rand(B, 778, 3), "trans_masks": torch.ones(B, 3, H, H), "scales": torch.ones(B), "idxs": torch.arange(B),
              "depths": torch.rand(B, H, H)}
    args = options.make_args()
    ex = data_dic(sample, "FreiHand", "training", args, device="cpu")
    assert torch.equal(ex["depths"], sample["depths"])
    assert "depths" not in data_dic({k: v for k, v in sample.items() if k != "depths"}, "FreiHand", "training", args, device="cpu")
    ho = synth.to_ho3d_sample(sample)
    assert torch.equal(ho["depth_crop"], sample["depths"]) and "depth_crop" not in synth.to_ho3d_sample({k: v for k, v in sample.items() if k != "depths"})
    ex = data_dic(ho, "HO3D", "training", args, device="cpu")
    assert torch.equal(ex["depths"], sample["depths"])
    ex = data_dic(ho, "HO3D", "training", args, device="cpu", image_size=112)
    assert tuple(ex["depths"].shape) == (B, 112, 112) and torch.equal(ex["depths"], sample["depths"][:, ::2, ::2])
