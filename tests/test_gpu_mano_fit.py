"""The one-launch keypoint fit (csrc/mano_fit.hip: hifihr_mano_fit; hifihr_amd/ops.py mano_fit; hifihr_amd/fit.py) on the MI355X.  The kernel
cases are those of tests/test_hostsim_mano_fit.py (tests/mano_fit_cases.py) plus the 151-iteration trajectory and its recovery; the
reference is the float64 restatement of tests/mano_fit_ref.py, the bounds come from its float32 evaluation on the same case."""
import pytest
import torch

import mano_fit_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    return get_lib()


@pytest.fixture(scope="module")
def tables_of(synth_tables, mano_dense):
    return {"synth": synth_tables, "dense": mano_dense[0]}


@pytest.mark.parametrize("case", fc.EVAL_CASES, ids=lambda c: c[0])
def test_iters_0_matches_float64_autograd(lib, tables_of, case):
    fc.eval_case(lib, "cuda", tables_of[case[6]], *case[:6])


@pytest.mark.parametrize("iters,with3d", [(1, False), (5, False), (5, True)])
def test_trajectory_matches_the_float64_restatement(lib, synth_tables, iters, with3d):
    fc.trajectory_case(lib, "cuda", synth_tables, iters, with3d=with3d)


@pytest.mark.parametrize("with3d", [False, True], ids=["2d", "3d"])
def test_151_iterations_match_and_recover(lib, synth_tables, with3d):
    out, r64, case = fc.trajectory_case(lib, "cuda", synth_tables, 151, with3d=with3d)
    fc.recovery_check(out, r64, case)


def test_invariances(lib, synth_tables):
    fc.invariance_case(lib, "cuda", synth_tables, iters=5)


def test_a_non_finite_hand_stops_alone(lib, synth_tables):
    fc.nonfinite_case(lib, "cuda", synth_tables, iters=3)


def test_refusals_leave_the_outputs_untouched(lib, synth_tables):
    fc.refusal_case(lib, "cuda", synth_tables)


@pytest.fixture(scope="module")
def model_and_batch(synth_tables):
    from hifihr_amd import options, synth
    from hifihr_amd.models import Model
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = Model(True, dev, False, "mano", False, "res18", mano_tables=synth_tables).to(dev).eval()
    args = options.baseline_config2_args(train_batch=3)
    batch = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, 3, device=dev, open_2dj=True)
    ex = data_dic(batch, "FreiHand", "training", args, device=dev)
    with torch.no_grad():
        out = model("FreiHand", False, ex["imgs"], Ks=ex["Ps"], root_xyz=ex["joints"][:, 9].unsqueeze(1))
    return model, ex, out


def _pixel_error(j2d, det, con):
    c = (con.reshape(con.shape[0], 21) > 0).float()
    return float((((j2d - det) ** 2).sum(2).sqrt() * c).sum() / c.sum())


def test_fit_keypoints_on_a_model(model_and_batch):
    from hifihr_amd import fit, ops
    from hifihr_amd.traineval import proj_func
    model, ex, out = model_and_batch
    root = ex["joints"][:, 9]
    before = _pixel_error(proj_func(out["joints"] + root.unsqueeze(1), ex["Ks"]), ex["open_2dj"], ex["open_2dj_con"])
    res = fit.fit_keypoints(model, out, ex["open_2dj"], ex["open_2dj_con"], ex["Ks"], root_xyz=root)
    after = _pixel_error(res["j2d"], ex["open_2dj"], ex["open_2dj_con"])
    print(f"mean reprojection error to the detections: {before:.3f} px -> {after:.3f} px; done {res['fit_done'].tolist()}")
    assert res["fit_done"].tolist() == [151] * 3 and after < before
    joints, verts = ops.mano_full(model.hand_layer.handle, res["pose_params"], res["shape_params"], model.root_id, None)[:2]
    assert torch.equal(res["joints"], joints) and torch.equal(res["mano_verts"], verts)
    assert res["fit_trace"].shape == (3, 152, 8) and bool(torch.isfinite(res["fit_trace"]).all())
    # the inputs are left as they were
    assert not torch.equal(res["pose_params"], out["pose_params"])


def test_graph_replay_gives_the_eager_bits(model_and_batch):
    from hifihr_amd import fit, ops
    model, ex, out = model_and_batch
    h = model.hand_layer.handle
    root = ex["joints"][:, 9].contiguous()
    conf = ex["open_2dj_con"].reshape(3, 21).contiguous()
    prior = fit.tsa_tables(root.device)
    call = lambda: ops.mano_fit(h, out["pose_params"], out["shape_params"], root, ex["Ks"], ex["open_2dj"], conf, iters=10, prior=prior)
    eager = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = call()
    torch.cuda.current_stream().wait_stream(side)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e, c)
    assert captured[4].tolist() == [10] * 3


def test_run_evaluation_refines_from_a_cache_with_detections(model_and_batch, capsys):
    """train_hrnet.run_evaluation on a real FreiHandDeviceCache that holds detections: with the option on every batch carries open_2dj and
    is refined (the summary changes); with it off the pass is the one made before.  (Last in the file: the pass leaves the model in
    training mode.)"""
    import train_hrnet
    from hifihr_amd import options, synth
    from hifihr_amd.data import FreiHandDeviceCache
    model = model_and_batch[0]
    dev = torch.device("cuda", 0)
    s = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, 5, device=dev, images="render", open_2dj=True)
    arrays = {"images": (s["trans_images"].permute(0, 2, 3, 1) * 255).round().to(torch.uint8).numpy(),
              "masks": (s["trans_masks"][:, 0] * 255).to(torch.uint8).numpy(), "Ks": s["trans_Ks"].numpy(),
              "joints": s["trans_joints"].numpy(), "verts": s["trans_verts"].numpy()}
    cache = FreiHandDeviceCache(arrays["images"], arrays["masks"], arrays["Ks"], arrays["joints"], arrays["verts"], device=dev,
                                open_2dj=s["trans_open_2dj"].numpy(), open_2dj_con=s["open_2dj_con"].numpy())
    off = options.baseline_config2_args(val_batch=3)
    on = options.baseline_config2_args(val_batch=3, fit_keypoints=True, fit_iters=30)
    capsys.readouterr()
    plain = train_hrnet.run_evaluation(model, cache, arrays, off, dev)
    assert capsys.readouterr().out == ""
    fitted = train_hrnet.run_evaluation(model, cache, arrays, on, dev)
    assert "REFINED by 30 fit iterations against 'open_2dj' in 2 batches" in capsys.readouterr().out
    print({k: (plain[k], fitted[k]) for k in plain if isinstance(plain[k], float)})
    assert set(plain) == set(fitted) and plain != fitted
    assert all(v == v and abs(v) != float("inf") for v in fitted.values() if isinstance(v, float))
    model.eval()
