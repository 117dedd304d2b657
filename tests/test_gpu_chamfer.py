"""The Chamfer distance on the MI355X: hifihr_chamfer_fwd / _bwd through the C ABI on the cases of tests/test_hostsim_chamfer.py
(tests/chamfer_cases.py; reference: the float64 restatement of tests/chamfer_ref.py, pinned to the reference's ChamferLoss by
tests/golden/chamfer.npz), and the Python surface end to end: ops.chamfer_distance, the loss name `chamfer` on the MANO and the
NIMBLE-shaped model, the captured step, evaluate.chamfer and Evaluator(chamfer=True)."""
import os

import numpy as np
import pytest
import torch

import chamfer_cases as cc
import chamfer_ref as cr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


def test_known_answers(lib):
    cc.known_answers_case(lib, "cuda")


@pytest.mark.parametrize("ni", range(5))
def test_boundaries_match_the_restatement(lib, ni):
    """N = the ni-th of {1, Q-1, Q, Q+1, 2Q+3} against every M of {1, T-1, T, T+1, 2T+5}"""
    Ns, Ms = cc.boundary_sizes(lib)
    for M in Ms:
        cc.boundary_case(lib, "cuda", Ns[ni], M)


def test_ties_go_to_the_lowest_index(lib):
    cc.tie_case(lib, "cuda")


@pytest.mark.parametrize("N,M", [(778, 778), (5990, 778), (1500, 5990)])
def test_product_sizes(lib, N, M):
    cc.product_case(lib, "cuda", 2, N, M)


def test_zero_weights(lib):
    cc.zero_weight_case(lib, "cuda")


def test_null_gradients(lib):
    cc.null_gradient_case(lib, "cuda")


def test_reference_chamfer_loss(lib):
    cc.golden_case(lib, "cuda", GOLDEN)


def test_refusals_leave_the_outputs_untouched(lib):
    cc.refusal_case(lib, "cuda")


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def _grad_close(got, ref):
    bound = cc.EPS32 * np.abs(ref) + 1e-10 * float(np.abs(ref).max())
    return bool((np.abs(got.double().cpu().numpy() - ref) <= bound).all())


def test_ops_match_the_restatement_through_autograd(lib):
    """ops.chamfer_distance -> backward against the float64 restatement under the bounds of the kernel cases: x alone, then both."""
    from hifihr_amd import ops
    q, t = cc.geometry(lib)
    xs, ys = cc.seeded_points(2, q + 1, t + 1, seed=21)
    ref = cr.chamfer(xs, ys, *cc.W, cc.GOUT)
    for both in (False, True):
        x, y = torch.as_tensor(xs).cuda().requires_grad_(True), torch.as_tensor(ys).cuda().requires_grad_(both)
        val = ops.chamfer_distance(x, y, *cc.W)
        assert val.dim() == 0 and val.dtype == torch.float32
        (val * cc.GOUT).backward()
        assert abs(float(val.detach()) - ref["value"]) <= cc.EPS32 * abs(ref["value"])
        assert _grad_close(x.grad, ref["gx"])
        assert (y.grad is None) if not both else _grad_close(y.grad, ref["gy"])
    sums = ops.chamfer_sums(torch.as_tensor(xs).cuda(), torch.as_tensor(ys).cuda())
    assert sums.dtype == torch.float64 and sums.shape == (2, 2) and not sums.requires_grad
    assert float(np.max(np.abs(sums.cpu().numpy() - ref["sums"]) / ref["sums"])) <= 1e-12
    unit = cr.chamfer(xs, ys)
    assert abs(float(ops.chamfer_distance(torch.as_tensor(xs).cuda(), torch.as_tensor(ys).cuda())) - unit["value"]) <= cc.EPS32 * unit["value"]


def _model(tables, hand_model="mano", nimble_tables=None):
    from hifihr_amd.models import Model
    torch.manual_seed(0)
    return Model(True, torch.device("cuda"), False, hand_model, False, "res18", mano_tables=tables, nimble_tables=nimble_tables).cuda().train()


def _batch(model, B, args):
    from hifihr_amd import synth
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda")
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, first_index=0, device=dev)
    return data_dic(sample, "FreiHand", "training", args, device=dev)


def _value_of(pred, target, lam):
    """lambda * the restatement's value at unit weights, and the bound of one fp32 rounding plus the fp32 rounding of the weight"""
    ref = cr.chamfer(pred.detach().float().cpu().numpy(), target.detach().float().cpu().numpy(), lam, lam)
    return ref["value"], cc.EPS32 * abs(ref["value"])


def test_loss_function_on_the_mano_model(synth_tables, monkeypatch):
    """Model + LossFunction at B = 2 with `chamfer` added to the default list: the key, finite, the restatement's value on
    outputs['mano_verts'] against examples['verts']; every other term has the bits it has without the name; the total is the sum; a
    point cloud of another size as the target; without the name nothing changes."""
    from hifihr_amd import ops, options
    from hifihr_amd.losses import LossFunction
    base = options.baseline_config2_args(train_batch=2)
    args = options.baseline_config2_args(train_batch=2, losses=base.losses + ["chamfer"], lambda_chamfer=250.0)
    model = _model(synth_tables)
    ex = _batch(model, 2, base)
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    with torch.no_grad():
        out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    assert "_pred_root" not in out                                   # the MANO tail hands out nothing new
    lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
    lf = LossFunction()
    d0 = lf(lex, out, base.losses, "FreiHand", base)
    parts0 = [names for _, _, names in lf._total_parts]
    d1 = lf(lex, out, args.losses, "FreiHand", args)
    assert set(d1) == set(d0) | {"chamfer"} and "chamfer" not in d0
    for k in d0:
        assert torch.equal(d0[k], d1[k]), k
    assert [names for _, _, names in lf._total_parts] == parts0 + [["chamfer"]]
    # without the name the term's code is not reached at all: no launch is added to the default step
    with monkeypatch.context() as m:
        m.setattr(ops, "_chamfer_run", lambda *a, **k: pytest.fail("the default loss list reached the Chamfer kernels"))
        again = lf(lex, out, base.losses, "FreiHand", base)
        assert set(again) == set(d0) and [names for _, _, names in lf._total_parts] == parts0
        with pytest.raises(pytest.fail.Exception):
            lf(lex, out, args.losses, "FreiHand", args)
    want, bound = _value_of(out["mano_verts"], lex["verts"], 250.0)
    assert d1["chamfer"].dim() == 0 and want > 0.0 and abs(float(d1["chamfer"]) - want) <= bound, (float(d1["chamfer"]), want)
    assert torch.equal(d1["chamfer"], ops.chamfer_distance(out["mano_verts"], lex["verts"], 250.0, 250.0))
    total = lf.total(d1, args.losses)
    stacked = torch.stack([d1[k] for k in args.losses]).double().sum()
    assert abs(float(total) - float(stacked)) <= 1e-6 * abs(float(stacked))
    # a point cloud as the target: M is neither 778 nor 5990
    cloud = (lex["verts"][:, ::3] + 0.001).contiguous()[:, :257]
    assert cloud.shape[1] == 257
    d2 = lf(dict(lex, chamfer_points=cloud), out, ["chamfer"], "FreiHand", args)
    want, bound = _value_of(out["mano_verts"], cloud, 250.0)
    assert abs(float(d2["chamfer"]) - want) <= bound
    # ... and a caller's own prediction
    mine = out["mano_verts"][:, :300].contiguous()
    d3 = lf(lex, dict(out, chamfer_points=mine), ["chamfer"], "FreiHand", args)
    want, bound = _value_of(mine, lex["verts"], 250.0)
    assert abs(float(d3["chamfer"]) - want) <= bound


def test_loss_function_on_the_nimble_shaped_model(synth_tables):
    """hand_model = 'nimble' with synthetic tables: the prediction is the dense skin outputs['verts'] made root-relative with
    outputs['_pred_root'], and the gradient of the term alone reaches the layer's parameters (the shape and pose heads)."""
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.nimble_tables import synthetic_nimble_tables
    args = options.baseline_config2_args(train_batch=2, hand_model="nimble", losses=["chamfer"], lambda_chamfer=100.0)
    model = _model(synth_tables, "nimble", synthetic_nimble_tables(0))
    from hifihr_amd import ops, synth
    from hifihr_amd.traineval import data_dic
    mano, rend = ops.ManoLayerHandle(synth_tables), ops.RendererHandle(synth_tables.faces, 778, image_size=224, aa=3)
    ex = data_dic(synth.make_batch(mano, rend, 2, device=torch.device("cuda")), "FreiHand", "training", args, device=torch.device("cuda"))
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    assert out["verts"].shape[1:] == (5990, 3) and out["_pred_root"].shape == (2, 1, 3)
    lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
    d = LossFunction()(lex, out, ["chamfer"], "FreiHand", args)
    want, bound = _value_of(out["verts"] - out["_pred_root"], lex["verts"], 100.0)
    assert want > 0.0 and abs(float(d["chamfer"].detach()) - want) <= bound, (float(d["chamfer"].detach()), want)
    d["chamfer"].backward()
    for name in ("pose_reg", "shape_reg"):
        g = [p.grad for p in getattr(model.hand_encoder, name).parameters()]
        assert all(x is not None and torch.isfinite(x).all() for x in g) and any(float(x.abs().max()) > 0 for x in g), name


def test_captured_step_replays_with_the_term(synth_tables):
    """traineval's captured step with `chamfer`: it replays, the loss is finite, the term has the bits of the eager step's (its forward is
    bitwise repeatable) and the parameters move."""
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, forward_backward
    from test_gpu_e2e import _warm_eager
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        B = 2
        base = options.baseline_config2_args(train_batch=B)
        args = options.baseline_config2_args(train_batch=B, losses=base.losses + ["chamfer"], lambda_chamfer=250.0)
        model, model2 = _model(synth_tables), _model(synth_tables)
        model2.load_state_dict(model.state_dict())
        ex = _batch(model, B, args)
        opt, opt2 = FusedAdam(FlatParams(model), lr=1e-4), FusedAdam(FlatParams(model2), lr=1e-4)
        g = GraphedTrainStep(model2, LossFunction(), opt2, ex, args, warmup=2)
        before = opt2.flatp.flat.detach().clone()
        _warm_eager(model, opt, ex, args)                  # the first eager step of a model dispatches other kernels than every later one
        _, dic_e = forward_backward(model, LossFunction(), opt, ex, args)
        loss_g, dic_g = g()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_g)) and float(dic_g["chamfer"].detach()) > 0.0
        assert torch.equal(dic_e["chamfer"].detach(), dic_g["chamfer"].detach()), (float(dic_e["chamfer"].detach()), float(dic_g["chamfer"].detach()))
        assert float((opt2.flatp.flat.detach() - before).abs().max()) > 0.0
        loss_g2, _ = g()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_g2))
        g.release()
    finally:
        torch.cuda.set_stream(prev)


def test_evaluate_chamfer_and_the_evaluator_keys(lib):
    """evaluate.chamfer = chamfer_sums / (N, M); Evaluator(chamfer=True) adds exactly CHAMFER_KEYS, equal to a direct computation from
    the collected predictions; without the keyword the dictionary has the keys it has today."""
    from hifihr_amd import evaluate, ops
    g = torch.Generator().manual_seed(4)
    n, root_id = 6, 9
    verts_gt = (torch.randn(n, 778, 3, generator=g) * 0.05 + 0.3)
    xyz_gt = (torch.randn(n, 21, 3, generator=g) * 0.05 + 0.3)
    root = xyz_gt[:, root_id:root_id + 1]
    verts_pred = ((verts_gt - root) * 1.05 + 0.004 * torch.randn(n, 778, 3, generator=g)).cuda()
    xyz_pred = ((xyz_gt - root) + 0.004 * torch.randn(n, 21, 3, generator=g)).cuda()
    pair = evaluate.chamfer(verts_pred, (verts_gt - root).cuda())
    sums = ops.chamfer_sums(verts_pred, (verts_gt - root).cuda())
    assert pair.dtype == torch.float64 and pair.shape == (n, 2)
    mean = sums.cpu().numpy() / np.asarray([778.0, 778.0])           # one fp64 division: at most one unit in the last place apart
    assert bool((np.abs(pair.cpu().numpy() - mean) <= 2.0 ** -52 * mean).all())
    other = evaluate.chamfer(verts_pred[:, :300].contiguous(), (verts_gt - root).cuda())
    ref = cr.chamfer(verts_pred[:, :300].cpu().numpy(), (verts_gt - root).numpy())
    assert np.allclose(other.cpu().numpy(), ref["sums"] / np.asarray([300.0, 778.0]), rtol=1e-12, atol=0.0)
    summaries = {}
    for key, kw in (("plain", {}), ("bench", dict(benchmark=True)), ("chamfer", dict(chamfer=True)), ("both", dict(benchmark=True, chamfer=True))):
        ev = evaluate.Evaluator(**kw)
        for lo in range(0, n, 4):
            ev.collect({"joints": xyz_pred[lo:lo + 4], "mano_verts": verts_pred[lo:lo + 4]}, {}, "FreiHand", render=False)
        summaries[key] = ev.summary(xyz_gt.numpy(), verts_gt.numpy(), root_id=root_id)
    assert set(summaries["plain"]) == {"pose_3d", "vert_3d"}
    assert set(summaries["bench"]) == {"pose_3d", "vert_3d"} | set(evaluate.BENCHMARK_KEYS)
    assert set(summaries["chamfer"]) == {"pose_3d", "vert_3d"} | set(evaluate.CHAMFER_KEYS)
    assert set(summaries["both"]) == set(summaries["bench"]) | set(evaluate.CHAMFER_KEYS)
    for k in summaries["bench"]:
        assert summaries["both"][k] == summaries["bench"][k], k
    for k in ("pose_3d", "vert_3d"):
        assert summaries["chamfer"][k] == summaries["plain"][k] == summaries["bench"][k], k
    aligned = evaluate.align_w_scale(verts_gt.cuda(), verts_pred)
    want = {"mesh_chamfer": float(evaluate.chamfer(verts_pred, (verts_gt.cuda() - root.cuda())).sum(1).mean(0)),
            "mesh_al_chamfer": float(evaluate.chamfer(aligned, verts_gt.cuda()).sum(1).mean(0))}
    for k in evaluate.CHAMFER_KEYS:
        assert summaries["chamfer"][k] == want[k] == summaries["both"][k] and want[k] > 0.0, (k, summaries["chamfer"][k], want[k])
    assert want["mesh_al_chamfer"] < want["mesh_chamfer"]
