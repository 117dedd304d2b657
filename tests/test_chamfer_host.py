"""Host-only checks of the Chamfer distance's Python surface (no kernel runs): the options, the loss name, the Evaluator's keys, the
refusal of CPU tensors; and the restatement's gradient (tests/chamfer_ref.py) against torch float64 autograd of the dense formulation."""
import numpy as np
import pytest
import torch

import chamfer_ref as cr


def test_options_default_and_override():
    from hifihr_amd import options
    a = options.make_args()
    assert a.lambda_chamfer == 1.0 and a.chamfer_metric is False and "chamfer" not in a.losses
    b = options.make_args(lambda_chamfer=250.0, chamfer_metric=True)
    assert b.lambda_chamfer == 250.0 and b.chamfer_metric is True
    assert "chamfer" not in options.baseline_config2_args().losses


def test_the_loss_name_is_known_and_reaches_the_kernels():
    """The name is not ignored: LossFunction goes to ops.chamfer_distance, which has no CPU path."""
    from hifihr_amd import losses, options
    from hifihr_amd._lib import HifihrError
    assert "chamfer" in losses.TERMS
    args = options.make_args()
    with pytest.raises(HifihrError):
        losses.LossFunction()({"verts": torch.zeros(1, 5, 3)}, {"mano_verts": torch.zeros(1, 4, 3)}, ["chamfer"], "FreiHand", args)
    assert losses.LossFunction()({"verts": torch.zeros(1, 5, 3)}, {"mano_verts": torch.zeros(1, 4, 3)}, [], "FreiHand", args) == {}


def test_ops_refuse_cpu_tensors():
    from hifihr_amd import evaluate, ops
    from hifihr_amd._lib import HifihrError
    for fn in (ops.chamfer_distance, ops.chamfer_sums, evaluate.chamfer):
        with pytest.raises(HifihrError):
            fn(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))


def test_evaluator_keyword_and_keys():
    import train_hrnet
    from hifihr_amd import evaluate, options
    assert evaluate.CHAMFER_KEYS == ("mesh_chamfer", "mesh_al_chamfer") and not set(evaluate.CHAMFER_KEYS) & set(evaluate.BENCHMARK_KEYS)
    assert evaluate.Evaluator().chamfer is False and evaluate.Evaluator(chamfer=True).chamfer is True
    assert evaluate.Evaluator(benchmark=True).chamfer is False
    assert evaluate.Evaluator().summary() == {} and evaluate.Evaluator(chamfer=True).summary() == {}
    assert train_hrnet.make_evaluator(options.make_args(), "cpu").chamfer is False
    assert train_hrnet.make_evaluator(options.make_args(chamfer_metric=True), "cpu").chamfer is True
    assert train_hrnet.build_args(train_hrnet.parse([])).chamfer_metric is False
    report = train_hrnet.benchmark_report({"f_score_5": 0.5, "mesh_chamfer": 1.5e-4, "mesh_al_chamfer": 5e-5, "pose_3d": 1.0})
    assert report.splitlines() == ["f_score_5: 0.500000", "mesh_chamfer: 1.500000e-04", "mesh_al_chamfer: 5.000000e-05"]
    assert train_hrnet.benchmark_report({"f_score_5": 0.5}) == "f_score_5: 0.500000"


def test_restatement_gradient_matches_autograd_of_the_dense_form():
    """A tie-free seeded case: value and gradients of tests/chamfer_ref.py against torch float64 autograd of
    w_xy mean_b mean_i min_j |x_i - y_j|^2 + w_yx mean_b mean_j min_i |x_i - y_j|^2."""
    g = torch.Generator().manual_seed(0)
    x32, y32 = torch.rand(2, 19, 3, generator=g), torch.rand(2, 31, 3, generator=g)
    w, gout = (0.7, 1.3), -1.7
    ref = cr.chamfer(x32.numpy(), y32.numpy(), w[0], w[1], gout)
    x, y = x32.double().requires_grad_(True), y32.double().requires_grad_(True)
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    value = float(np.float32(w[0])) * d.min(2).values.mean(1).mean() + float(np.float32(w[1])) * d.min(1).values.mean(1).mean()
    (value * float(np.float32(gout))).backward()
    assert abs(float(value.detach()) - ref["value"]) <= 1e-14 * abs(ref["value"])
    for got, want in ((ref["gx"], x.grad.numpy()), (ref["gy"], y.grad.numpy())):
        assert float(np.abs(want).max()) > 0 and float(np.abs(got - want).max()) <= 1e-13 * float(np.abs(want).max())
    # a direction of weight 0 gets no gradient from its own term
    only = cr.chamfer(x32.numpy(), y32.numpy(), 0.0, 1.0, 1.0)
    x.grad, y.grad = None, None
    d = ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)
    d.min(1).values.mean(1).mean().backward()
    assert float(np.abs(only["gx"] - x.grad.numpy()).max()) <= 1e-13 and float(np.abs(only["gy"] - y.grad.numpy()).max()) <= 1e-13
