"""The point-to-mesh distance on the MI355X: hifihr_point_mesh_fwd / _bwd through the C ABI on the cases of
tests/test_hostsim_point_mesh.py (tests/point_mesh_cases.py; reference: the float64 restatement of tests/point_mesh_ref.py, bounds in the
cases' module docstring), and the Python surface end to end: ops.point_mesh_distance, the loss name `point_mesh` on the MANO and the
NIMBLE-shaped model, the captured step, evaluate.point_to_surface and Evaluator(point_mesh=True)."""
import numpy as np
import pytest
import torch

import point_mesh_cases as pc
import point_mesh_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


def test_known_answers(lib):
    pc.known_answers_case(lib, "cuda")


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("ni", range(5))
def test_boundaries_match_the_restatement(lib, direction, ni):
    """The ni-th query count of {1, Q-1, Q, Q+1, 2Q+3} against every searched count of {1, T-1, T, T+1, 2T+5}, for the (Q, T) of the points ->
    faces search (direction 0: Q points, T faces) and of the faces -> points search (direction 1: Q faces, T points)"""
    Ns, Fs = pc.boundary_sizes(lib, direction)
    pairs = [(Ns[ni], F) for F in Fs] if direction == 0 else [(N, Fs[ni]) for N in Ns]
    for N, F in pairs:
        pc.boundary_case(lib, "cuda", N, F)


def test_ties_go_to_the_lowest_index(lib):
    pc.tie_case(lib, "cuda")


def test_mano_topology(lib):
    pc.mano_case(lib, "cuda", 4)


def test_soup_at_2048_points_4096_faces(lib):
    pc.soup_product_case(lib, "cuda", 1, 2048, 4096)


def test_zero_weights(lib):
    pc.zero_weight_case(lib, "cuda")


def test_null_gradients(lib):
    pc.null_gradient_case(lib, "cuda")


def test_refusals_leave_the_outputs_untouched(lib):
    pc.refusal_case(lib, "cuda")


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def _grad_close(got, ref):
    bound = pc.EPS32 * np.abs(ref) + 1e-10 * float(np.abs(ref).max())
    err = np.abs(got.double().cpu().numpy() - ref)
    print(f"[point_mesh] gradient: max error {float(err.max()):.2e}, worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    return bool((err <= bound).all())


def test_ops_match_the_restatement_through_autograd(lib):
    """ops.point_mesh_distance -> backward against the float64 restatement under the bounds of the kernel cases: the vertices alone, then
    both; point_mesh_sums; the face table is validated on first use."""
    from hifihr_amd import ops
    qp, tf, qf, tp = pc.geometry(lib)
    ps, vs, fs = pc.seeded_soup(2, qp + 1, pc.soup_verts(qf + 1), qf + 1, seed=21)
    ref = pr.point_mesh(ps, vs, fs, *pc.W, pc.GOUT)
    faces = torch.as_tensor(fs).cuda()
    for both in (False, True):
        p, v = torch.as_tensor(ps).cuda().requires_grad_(both), torch.as_tensor(vs).cuda().requires_grad_(True)
        val = ops.point_mesh_distance(p, v, faces, *pc.W)
        assert val.dim() == 0 and val.dtype == torch.float32
        (val * pc.GOUT).backward()
        assert abs(float(val.detach()) - ref["value"]) <= pc.EPS32 * abs(ref["value"])
        assert _grad_close(v.grad, ref["gv"])
        assert (p.grad is None) if not both else _grad_close(p.grad, ref["gp"])
    sums = ops.point_mesh_sums(torch.as_tensor(ps).cuda(), torch.as_tensor(vs).cuda(), faces)
    assert sums.dtype == torch.float64 and sums.shape == (2, 2) and not sums.requires_grad
    assert float(np.max(np.abs(sums.cpu().numpy() - ref["sums"]) / ref["sums"])) <= 1e-12
    one = ops.point_mesh_sums(torch.as_tensor(ps).cuda(), torch.as_tensor(vs).cuda(), faces, 1.0, 0.0)
    assert torch.equal(one[:, 0], sums[:, 0]) and not bool(one[:, 1].any())
    unit = pr.point_mesh(ps, vs, fs)
    got = float(ops.point_mesh_distance(torch.as_tensor(ps).cuda(), torch.as_tensor(vs).cuda(), faces))
    assert abs(got - unit["value"]) <= pc.EPS32 * unit["value"]
    for bad in ([[0, 1, vs.shape[1]]], [[0, 1, 1]], [[-1, 1, 2]]):
        with pytest.raises(ValueError):
            ops.point_mesh_distance(torch.as_tensor(ps).cuda(), torch.as_tensor(vs).cuda(), torch.tensor(bad, dtype=torch.int32).cuda())


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


def _value_of(points, verts, faces, lam_pf, lam_fp):
    """the restatement's value at the given weights, and the bound of one fp32 rounding"""
    ref = pr.point_mesh(points.detach().float().cpu().numpy(), verts.detach().float().cpu().numpy(), faces.cpu().numpy(), lam_pf, lam_fp)
    return ref["value"], pc.EPS32 * abs(ref["value"])


def test_loss_function_on_the_mano_model(synth_tables, monkeypatch):
    """Model + LossFunction at B = 2 with `point_mesh` added to the default list: the key, the restatement's value for examples['verts']
    against the mesh outputs['mano_verts'] / outputs['_faces_i32']; every other term has the bits it has without the name; the total is the
    sum; the second direction; a point cloud as the target; a caller's own mesh; without the name nothing changes."""
    from hifihr_amd import ops, options
    from hifihr_amd.losses import LossFunction
    base = options.baseline_config2_args(train_batch=2)
    args = options.baseline_config2_args(train_batch=2, losses=base.losses + ["point_mesh"], lambda_point_mesh=250.0)
    model = _model(synth_tables)
    ex = _batch(model, 2, base)
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    with torch.no_grad():
        out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    assert "_skin_faces_i32" not in out                              # the MANO tail hands out nothing new
    lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
    lf = LossFunction()
    d0 = lf(lex, out, base.losses, "FreiHand", base)
    parts0 = [names for _, _, names in lf._total_parts]
    total0 = lf.total(d0, base.losses)
    d1 = lf(lex, out, args.losses, "FreiHand", args)
    assert set(d1) == set(d0) | {"point_mesh"} and "point_mesh" not in d0
    for k in d0:
        assert torch.equal(d0[k], d1[k]), k
    assert [names for _, _, names in lf._total_parts] == parts0 + [["point_mesh"]]
    # without the name the term's code is not reached at all: no launch is added to the default step, dictionary and total keep their bits
    with monkeypatch.context() as m:
        m.setattr(ops, "_point_mesh_run", lambda *a, **k: pytest.fail("the default loss list reached the point-to-mesh kernels"))
        again = lf(lex, out, base.losses, "FreiHand", base)
        assert set(again) == set(d0) and [names for _, _, names in lf._total_parts] == parts0
        assert all(torch.equal(again[k], d0[k]) for k in d0) and torch.equal(lf.total(again, base.losses), total0)
        with pytest.raises(pytest.fail.Exception):
            lf(lex, out, args.losses, "FreiHand", args)
    faces = out["_faces_i32"]
    want, bound = _value_of(lex["verts"], out["mano_verts"], faces, 250.0, 0.0)
    assert d1["point_mesh"].dim() == 0 and want > 0.0 and abs(float(d1["point_mesh"]) - want) <= bound, (float(d1["point_mesh"]), want)
    assert torch.equal(d1["point_mesh"], ops.point_mesh_distance(lex["verts"], out["mano_verts"], faces, 250.0, 0.0))
    d1 = lf(lex, out, args.losses, "FreiHand", args)
    total = lf.total(d1, args.losses)
    stacked = torch.stack([d1[k] for k in args.losses]).double().sum()
    assert abs(float(total) - float(stacked)) <= 1e-6 * abs(float(stacked))
    # the second direction
    two = options.baseline_config2_args(train_batch=2, losses=["point_mesh"], lambda_point_mesh=250.0, lambda_point_mesh_faces=100.0)
    d2 = lf(lex, out, ["point_mesh"], "FreiHand", two)
    want2, bound2 = _value_of(lex["verts"], out["mano_verts"], faces, 250.0, 100.0)
    assert want2 > want and abs(float(d2["point_mesh"]) - want2) <= bound2
    # a point cloud as the target: N is neither 778 nor 5990
    cloud = (lex["verts"][:, ::3] + 0.001).contiguous()[:, :257]
    assert cloud.shape[1] == 257
    d3 = lf(dict(lex, chamfer_points=cloud), out, ["point_mesh"], "FreiHand", args)
    want, bound = _value_of(cloud, out["mano_verts"], faces, 250.0, 0.0)
    assert abs(float(d3["point_mesh"]) - want) <= bound
    # ... and a caller's own mesh under the reference's keys
    mine = faces[:300].contiguous()
    d4 = lf(lex, dict(out, verts=out["mano_verts"], faces=mine.unsqueeze(0).expand(2, -1, -1)), ["point_mesh"], "FreiHand", args)
    want, bound = _value_of(lex["verts"], out["mano_verts"], mine, 250.0, 0.0)
    assert abs(float(d4["point_mesh"]) - want) <= bound


def test_gradient_reaches_pose_and_shape_on_the_mano_model(synth_tables):
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    args = options.baseline_config2_args(train_batch=2, losses=["point_mesh"], lambda_point_mesh=100.0)
    model = _model(synth_tables)
    ex = _batch(model, 2, args)
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
    d = LossFunction()(lex, out, ["point_mesh"], "FreiHand", args)
    d["point_mesh"].backward()
    for name in ("pose_reg", "shape_reg"):
        g = [p.grad for p in getattr(model.hand_encoder, name).parameters()]
        assert all(x is not None and torch.isfinite(x).all() for x in g) and any(float(x.abs().max()) > 0 for x in g), name


def test_loss_function_on_the_nimble_shaped_model(synth_tables):
    """hand_model = 'nimble' with synthetic tables: the mesh is the dense skin outputs['verts'] made root-relative with outputs['_pred_root'],
    with the layer's own faces outputs['_skin_faces_i32'], and the gradient of the term alone reaches the shape and pose heads."""
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.nimble_tables import synthetic_nimble_tables
    args = options.baseline_config2_args(train_batch=2, hand_model="nimble", losses=["point_mesh"], lambda_point_mesh=100.0)
    model = _model(synth_tables, "nimble", synthetic_nimble_tables(0))
    from hifihr_amd import ops, synth
    from hifihr_amd.traineval import data_dic
    mano, rend = ops.ManoLayerHandle(synth_tables), ops.RendererHandle(synth_tables.faces, 778, image_size=224, aa=3)
    ex = data_dic(synth.make_batch(mano, rend, 2, device=torch.device("cuda")), "FreiHand", "training", args, device=torch.device("cuda"))
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    faces = out["_skin_faces_i32"]
    assert out["verts"].shape[1:] == (5990, 3) and faces.dim() == 2 and faces.shape[1] == 3 and faces.dtype == torch.int32
    assert 0 <= int(faces.min()) and int(faces.max()) < 5990 and torch.equal(faces, model.hand_layer.mesh_face[0])
    lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
    lf = LossFunction()
    d = lf(lex, out, ["point_mesh"], "FreiHand", args)
    assert float(lf.total(d, ["point_mesh"]).detach()) == float(d["point_mesh"].detach())
    want, bound = _value_of(lex["verts"], out["verts"] - out["_pred_root"], faces, 100.0, 0.0)
    assert want > 0.0 and abs(float(d["point_mesh"].detach()) - want) <= bound, (float(d["point_mesh"].detach()), want)
    d["point_mesh"].backward()
    for name in ("pose_reg", "shape_reg"):
        g = [p.grad for p in getattr(model.hand_encoder, name).parameters()]
        assert all(x is not None and torch.isfinite(x).all() for x in g) and any(float(x.abs().max()) > 0 for x in g), name


def test_captured_step_replays_with_the_term(synth_tables):
    """traineval's captured step with `point_mesh`: it replays, the loss is finite, the term has the bits of the eager step's (its forward
    is bitwise repeatable) and the parameters move."""
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
        args = options.baseline_config2_args(train_batch=B, losses=base.losses + ["point_mesh"], lambda_point_mesh=250.0,
                                             lambda_point_mesh_faces=50.0)
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
        assert bool(torch.isfinite(loss_g)) and float(dic_g["point_mesh"].detach()) > 0.0
        assert torch.equal(dic_e["point_mesh"].detach(), dic_g["point_mesh"].detach()), (float(dic_e["point_mesh"].detach()),
                                                                                         float(dic_g["point_mesh"].detach()))
        assert float((opt2.flatp.flat.detach() - before).abs().max()) > 0.0
        loss_g2, _ = g()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_g2))
        g.release()
    finally:
        torch.cuda.set_stream(prev)


def test_point_to_surface_and_the_evaluator_keys(lib, synth_tables):
    """evaluate.point_to_surface = the restatement's sum_pf / N; Evaluator(point_mesh=True) adds exactly POINT_MESH_KEYS, equal to a direct
    computation from the collected predictions; a prediction equal to the ground truth gives exactly 0; without the keyword the dictionary
    has the keys it has today."""
    from hifihr_amd import evaluate
    faces_np = np.asarray(synth_tables.faces, np.int32)
    faces = torch.as_tensor(faces_np).cuda()
    vt = torch.as_tensor(np.asarray(synth_tables.v_template, np.float32))
    g = torch.Generator().manual_seed(4)
    n, root_id = 6, 9
    verts_gt = vt[None] + 0.3 + 0.002 * torch.randn(n, 778, 3, generator=g)
    xyz_gt = (torch.randn(n, 21, 3, generator=g) * 0.05 + 0.3)
    root = xyz_gt[:, root_id:root_id + 1]
    verts_pred = ((verts_gt - root) * 1.05 + 0.002 * torch.randn(n, 778, 3, generator=g)).cuda()
    xyz_pred = ((xyz_gt - root) + 0.004 * torch.randn(n, 21, 3, generator=g)).cuda()
    gt_rel = (verts_gt - root).cuda()
    got = evaluate.point_to_surface(verts_pred, faces, gt_rel)
    ref = pr.point_mesh(gt_rel.cpu().numpy(), verts_pred.cpu().numpy(), faces_np)
    assert got.dtype == torch.float64 and got.shape == (n,)
    err = float(np.max(np.abs(got.cpu().numpy() - ref["sums"][:, 0] / 778.0) / (ref["sums"][:, 0] / 778.0)))
    print(f"[point_mesh] point_to_surface against the restatement: relative error {err:.2e} (bound 1e-12)")
    assert err <= 1e-12
    assert not bool(evaluate.point_to_surface(gt_rel, faces, gt_rel).any())              # on the surface: exactly 0
    summaries = {}
    for key, kw in (("plain", {}), ("bench", dict(benchmark=True)), ("p2s", dict(point_mesh=True)),
                    ("all", dict(benchmark=True, chamfer=True, point_mesh=True)), ("cham", dict(benchmark=True, chamfer=True))):
        ev = evaluate.Evaluator(**kw)
        for lo in range(0, n, 4):
            ev.collect({"joints": xyz_pred[lo:lo + 4], "mano_verts": verts_pred[lo:lo + 4], "_faces_i32": faces}, {}, "FreiHand", render=False)
        summaries[key] = ev.summary(xyz_gt.numpy(), verts_gt.numpy(), root_id=root_id)
    assert set(summaries["plain"]) == {"pose_3d", "vert_3d"}
    assert set(summaries["p2s"]) == {"pose_3d", "vert_3d"} | set(evaluate.POINT_MESH_KEYS)
    assert set(summaries["all"]) == set(summaries["cham"]) | set(evaluate.POINT_MESH_KEYS)
    for k in summaries["cham"]:
        assert summaries["all"][k] == summaries["cham"][k], k
    for k in ("pose_3d", "vert_3d"):
        assert summaries["p2s"][k] == summaries["plain"][k] == summaries["bench"][k], k
    aligned = evaluate.align_w_scale(verts_gt.cuda(), verts_pred)
    want = {"mesh_p2s": float(evaluate.point_to_surface(verts_pred, faces, verts_gt.cuda() - root.cuda()).mean(0)),
            "mesh_al_p2s": float(evaluate.point_to_surface(aligned, faces, verts_gt.cuda()).mean(0))}
    for k in evaluate.POINT_MESH_KEYS:
        assert summaries["p2s"][k] == want[k] == summaries["all"][k] and want[k] > 0.0, (k, summaries["p2s"][k], want[k])
    assert want["mesh_al_p2s"] < want["mesh_p2s"]
    ev = evaluate.Evaluator(point_mesh=True, faces=faces)                                 # a prediction equal to the ground truth
    ev.collect({"joints": xyz_gt.cuda(), "mano_verts": verts_gt.cuda()}, {}, "FreiHand", render=False)
    assert ev.summary(xyz_gt.numpy(), verts_gt.numpy())["mesh_p2s"] == 0.0
    with pytest.raises(ValueError):
        ev = evaluate.Evaluator(point_mesh=True)
        ev.collect({"joints": xyz_gt.cuda(), "mano_verts": verts_gt.cuda()}, {}, "FreiHand", render=False)
        ev.summary(xyz_gt.numpy(), verts_gt.numpy())
