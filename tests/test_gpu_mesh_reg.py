"""The mesh regularisers `triangle` / `normal_consistency` on the MI355X: hifihr_mesh_topology_* and hifihr_mesh_reg_fwd / _bwd through the
C ABI on the cases of tests/test_hostsim_mesh_reg.py (tests/mesh_reg_cases.py; reference: the float64 restatement of
tests/mesh_reg_ref.py), and the Python surface end to end: ops.mesh_regularizers, Model's topology, the two loss names, the captured step."""
import numpy as np
import pytest
import torch

import mesh_reg_cases as mc
import mesh_reg_ref as mr

pytestmark = pytest.mark.gpu
_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


def test_known_answers(lib):
    mc.known_answers_case(lib, "cuda")


def test_topology_counts(lib, synth_tables):
    mc.topology_case(lib, "cuda", synth_tables)


@pytest.mark.parametrize("case", mc.RANDOM_CASES, ids=_ids)
def test_jittered_grids_match_the_restatement(lib, case):
    mc.random_case(lib, "cuda", *case)


def test_mano_topology_matches_the_restatement(lib, synth_tables):
    mc.mano_case(lib, "cuda", synth_tables)


def test_fan_and_book(lib):
    mc.fan_case(lib, "cuda")


def test_isolated_vertex(lib):
    mc.isolated_vertex_case(lib, "cuda")


def test_refusals_leave_the_outputs_untouched(lib):
    mc.refusal_case(lib, "cuda")


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_ops_match_the_restatement_through_autograd(lib):
    """ops.MeshTopology + ops.mesh_regularizers -> backward, against the float64 restatement under the bound of the kernel cases."""
    from hifihr_amd import ops
    B, n, m = mc.RANDOM_CASES[1]
    verts, faces = mc.grid_verts(n, m, B, jitter=0.25, seed=5), mc.grid_faces(n, m)
    topo = ops.MeshTopology(faces, n * m)
    ref = mr.mesh_regularizers(verts, faces, *mc.LAM, gout=mc.GOUT)
    r32 = mr.mesh_regularizers(verts, faces, *mc.LAM, gout=mc.GOUT, dtype=torch.float32)
    assert (topo.V, topo.E, topo.Q) == (n * m, len(ref["topo"]["edges"]), len(ref["topo"]["quads"]))
    v = verts.cuda().requires_grad_(True)
    out = ops.mesh_regularizers(topo, v, *mc.LAM)
    (out * torch.tensor(mc.GOUT, device="cuda")).sum().backward()
    eo, eg = float((out.detach().double().cpu() - ref["out"]).abs().max()), float((v.grad.double().cpu() - ref["gverts"]).abs().max())
    assert eo <= mc._bound(float((r32["out"].double() - ref["out"]).abs().max()), ref["out"])
    assert eg <= mc._bound(float((r32["gverts"].double() - ref["gverts"]).abs().max()), ref["gverts"])
    assert ops.mesh_topology_of(torch.as_tensor(faces).cuda(), n * m).Q == topo.Q


def _model(tables):
    from hifihr_amd.models import Model
    torch.manual_seed(0)
    return Model(True, torch.device("cuda"), False, "mano", False, "res18", mano_tables=tables).cuda().train()


def _batch(model, B, args):
    from hifihr_amd import synth
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda")
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, first_index=0, device=dev)
    return data_dic(sample, "FreiHand", "training", args, device=dev)


def test_loss_function_returns_both_terms(synth_tables):
    """Model + LossFunction at B = 2 with the two names added to the default list: both keys, finite, equal to ops.mesh_regularizers on
    outputs['mano_verts']; every other term has the bits it has without the two names; the total is the sum."""
    from hifihr_amd import ops, options
    from hifihr_amd.losses import LossFunction
    base = options.baseline_config2_args(train_batch=2)
    args = options.baseline_config2_args(train_batch=2, losses=base.losses + ["triangle", "normal_consistency"])
    model = _model(synth_tables)
    ex = _batch(model, 2, base)
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    with torch.no_grad():
        out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    assert isinstance(out["_mesh_topo"], ops.MeshTopology) and out["_mesh_topo"] is model._mesh_topo
    assert (out["_mesh_topo"].V, out["_mesh_topo"].E, out["_mesh_topo"].Q) == (778, 2315, 2299)
    lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
    lf = LossFunction()
    d0 = lf(lex, out, base.losses, "FreiHand", base)
    d1 = lf(lex, out, args.losses, "FreiHand", args)
    assert set(d1) == set(d0) | {"triangle", "normal_consistency"}
    for k in d0:
        assert torch.equal(d0[k], d1[k]), k
    want = ops.mesh_regularizers(out["_mesh_topo"], out["mano_verts"], args.lambda_laplacian, args.lambda_normal_consistency)
    assert torch.equal(torch.stack([d1["triangle"], d1["normal_consistency"]]), want)
    assert bool(torch.isfinite(want).all()) and float(want[0]) > 0.0 and float(want[1]) > 0.0
    assert [names for _, _, names in lf._total_parts][-1] == ["triangle", "normal_consistency"]
    total = lf.total(d1, args.losses)
    stacked = torch.stack([d1[k] for k in args.losses]).double().sum()
    assert abs(float(total) - float(stacked)) <= 1e-6 * abs(float(stacked))
    # one name alone: the other is absent and its weight is 0
    d2 = lf(lex, out, ["triangle"], "FreiHand", args)
    assert set(d2) >= {"triangle"} and "normal_consistency" not in d2 and torch.equal(d2["triangle"], d1["triangle"])
    # outputs that do not come from Model: the topology is built from the faces and cached
    plain = {k: v for k, v in out.items() if k != "_mesh_topo"}
    d3 = lf(lex, plain, ["triangle", "normal_consistency"], "FreiHand", args)
    assert torch.equal(d3["triangle"], d1["triangle"]) and torch.equal(d3["normal_consistency"], d1["normal_consistency"])
    # the reference's keys, when a caller supplies both
    d4 = lf(lex, dict(plain, verts=out["mano_verts"], faces=out["mano_faces"]), ["triangle", "normal_consistency"], "FreiHand", args)
    assert torch.equal(d4["triangle"], d1["triangle"]) and torch.equal(d4["normal_consistency"], d1["normal_consistency"])


def test_captured_step_replays_with_the_two_terms(synth_tables):
    """traineval's captured step with the two names: it replays, the loss is finite, the two terms have the bits of the eager step's
    (their forward is bitwise repeatable) and the parameters move."""
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
        args = options.baseline_config2_args(train_batch=B, losses=base.losses + ["triangle", "normal_consistency"])
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
        assert bool(torch.isfinite(loss_g))
        for k in ("triangle", "normal_consistency"):
            assert torch.equal(dic_e[k].detach(), dic_g[k].detach()), (k, float(dic_e[k].detach()), float(dic_g[k].detach()))
        moved = float((opt2.flatp.flat.detach() - before).abs().max())
        assert moved > 0.0
        loss_g2, _ = g()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_g2))
        g.release()
    finally:
        torch.cuda.set_stream(prev)


# the settings of the reference's config/FreiHAND/fully_superv_freihand_shape.json that reach the step (paths, logging and worker counts left out)
FULLY_SUPERV_FREIHAND_SHAPE = {
    "train_datasets": ["FreiHand"], "val_datasets": ["FreiHand"], "total_epochs": 120, "init_lr": 0.001, "lr_steps": [30, 60, 90, 120, 150],
    "lr_gamma": 0.5, "save_interval": 1, "train_batch": 128, "val_batch": 8, "if_test": False, "save_mode": "only_latest",
    "lambda_j2d_gt": 0.0001, "lambda_j3d": 100, "lambda_bone_direc": 0.1, "lambda_scale": 10000, "lambda_silhouette": 10, "lambda_pose": 0.000001,
    "losses": ["joint_2d", "joint_3d", "bone_direc", "scale", "sil", "triangle"], "task": "train", "mode": ["training"],
}


def test_front_end_trains_on_a_config_that_lists_triangle(tmp_path, capsys):
    """`train_hrnet.py --config_json` on the reference's fully-supervised FreiHAND configuration (batch and length cut down): the captured
    step runs with `triangle` instead of stopping with KeyError: loss terms ['triangle'] were requested but not produced."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import train_hrnet as T
    cfg = dict(FULLY_SUPERV_FREIHAND_SHAPE, base_out_path=str(tmp_path / "run"), train_batch=4, total_epochs=1)
    f = tmp_path / "cfg.json"
    f.write_text(json.dumps(cfg))
    prev = torch.cuda.current_stream()
    try:
        assert T.main(["--config_json", str(f), "--synthetic_size", "8", "--max_iters", "2", "--print_freq", "1"]) == 0
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)          # main() switches to a non-default stream for graph capture
    cap = capsys.readouterr()
    assert "triangle=" in cap.out and "Done!" in cap.out, cap.out[-2000:]
    assert "capture failed" not in cap.err, cap.err[-2000:]
