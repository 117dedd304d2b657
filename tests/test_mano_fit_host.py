"""Host-side pieces of the keypoint fit (hifihr_amd/fit.py), no GPU and no kernel: the prior's formula and tables against the reference's own
tsa_pose_loss (tests/golden/mano_fit.npz, tools/make_mano_fit_golden.py), root_from_keypoints against numpy's least squares, the option
plumbing with `ops` stubbed, and the refusal of the NIMBLE-shaped layer."""
import os
import types

import numpy as np
import pytest
import torch

import mano_fit_ref as ref
from hifihr_amd import fit, options


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mano_fit.npz")))


def test_prior_formula_is_the_references(golden):
    """ref.prior_per_hand with the reference's own tables and its [1, 1, 2] weights on every row (the root's included) is tsa_pose_loss."""
    x = torch.from_numpy(golden["tsaposes"]).double().reshape(-1, 48)
    lo, hi = (torch.from_numpy(golden[k]).double().reshape(1, 48) for k in ("min_nonloss", "max_nonloss"))
    w = torch.tensor([1.0, 1.0, 2.0], dtype=torch.float64).repeat(16).view(1, 48)
    per_hand = ref.prior_per_hand(x, lo, hi, w)
    # float32 fixture values of sums of 48 addends: 48 roundings
    assert np.allclose(per_hand.numpy(), golden["sample_loss"], rtol=48 * 2.0 ** -24, atol=0)
    assert abs(float(per_hand.mean()) - float(golden["loss"][0])) <= 6 * 48 * 2.0 ** -24 * float(golden["loss"][0])
    assert float(per_hand[-1]) == 0.0                     # every component exactly on a bound: the comparisons are strict
    assert bool((x[:-1] > hi).any(0).all()) and bool((x[:-1] < lo).any(0).all())      # the inputs straddle every bound


def test_tsa_tables_are_the_references(golden):
    assert fit.TSA_HI.dtype == np.float32 and fit.TSA_HI.shape == (16, 3)
    assert np.array_equal(fit.TSA_HI, golden["max_nonloss"]) and np.array_equal(fit.TSA_LO, golden["min_nonloss"])
    assert np.array_equal(fit.TSA_W[1:], np.tile(np.float32([1, 1, 2]), (15, 1))) and not fit.TSA_W[0].any()
    assert bool((fit.TSA_LO < fit.TSA_HI).all())


def _skeleton(B, seed):
    g = torch.Generator().manual_seed(seed)
    J = 0.05 * torch.randn(B, 21, 3, generator=g, dtype=torch.float64)
    t = torch.cat([0.03 * torch.randn(B, 2, generator=g, dtype=torch.float64), 0.6 + 0.05 * torch.rand(B, 1, generator=g, dtype=torch.float64)], 1)
    K = torch.tensor([[480.0, 0.7, 112.0], [0.0, 470.0, 109.0], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(B, 1, 1)
    p = ((J + t.unsqueeze(1)).unsqueeze(2) * K.unsqueeze(1)).sum(3)
    uv = p[:, :, :2] / p[:, :, 2:3]
    conf = torch.rand(B, 21, generator=g, dtype=torch.float64)
    conf[:, 4] = 0.0
    return J, t, K, uv, conf, g


def test_root_from_keypoints_matches_lstsq():
    J, t, K, uv, conf, g = _skeleton(4, 3)
    assert float((fit.root_from_keypoints(J, uv, conf, K) - t).abs().max()) < 1e-9            # exact detections: the true translation
    uv = uv + 1.5 * torch.randn(uv.shape, generator=g, dtype=torch.float64)
    uv[:, 4] = 1e4                                                                            # a wild detection at confidence 0 does not count
    got = fit.root_from_keypoints(J, uv, conf.unsqueeze(-1), K)
    for b in range(4):
        k0, k1, k2 = K[b].numpy()
        rows = np.concatenate([k0[None] - uv[b, :, 0:1].numpy() * k2[None], k1[None] - uv[b, :, 1:2].numpy() * k2[None]], 0)
        c = np.concatenate([conf[b].numpy()] * 2)[:, None]
        rhs = -(rows * np.concatenate([J[b].numpy()] * 2, 0)).sum(1, keepdims=True)
        want = np.linalg.lstsq(rows * c, rhs * c, rcond=None)[0][:, 0]
        assert np.abs(got[b].numpy() - want).max() <= 1e-9 * np.abs(want).max()


def test_option_defaults_and_flag():
    import train_hrnet
    args = options.make_args(None)
    assert args.fit_keypoints is False and args.fit_iters == 151 and args.fit_target == "open_2dj"
    assert fit.fit_options(args) == dict(iters=151, target="open_2dj", weights=fit.FIT_WEIGHT_DEFAULTS)
    assert not train_hrnet.wants_keypoints(args) and not train_hrnet.fit_wants_detections(args)
    on = train_hrnet.build_args(train_hrnet.parse(["--fit_keypoints", "--override", '{"fit_iters": 7, "fit_w_3d": 2.5}']))
    assert on.fit_keypoints is True and fit.fit_options(on)["iters"] == 7 and fit.fit_options(on)["weights"][2] == 2.5
    assert train_hrnet.fit_wants_detections(on) and not train_hrnet.wants_keypoints(on)     # the fit's need is not a loss's
    on.fit_target = "j2d_gt"
    assert not train_hrnet.fit_wants_detections(on)
    assert train_hrnet.build_args(train_hrnet.parse([])).fit_keypoints is False


class _Stub:
    """Stands in for hifihr_amd.ops: records the calls, returns tensors of the right shapes."""

    def __init__(self):
        self.calls = []

    def mano_fit(self, handle, pose, beta, root, K, kp2d, conf, kp3d=None, conf3d=None, **kw):
        self.calls.append(("mano_fit", dict(kw, root=root.clone(), conf=conf.clone())))
        B = pose.shape[0]
        return pose + 1, beta + 1, root + 1, torch.zeros(B, kw["iters"] + 1, 8), torch.full((B,), kw["iters"], dtype=torch.int32)

    def mano_full(self, handle, pose, beta, root_id, root_xyz):
        self.calls.append(("mano_full", dict(root_id=root_id, pose=pose.clone())))
        B = pose.shape[0]
        return torch.full((B, 21, 3), 0.25), torch.full((B, 778, 3), 0.5), None, None, pose, beta


@pytest.fixture
def stubbed(monkeypatch):
    import hifihr_amd
    stub = _Stub()
    monkeypatch.setattr(hifihr_amd, "ops", stub, raising=False)
    monkeypatch.setitem(__import__("sys").modules, "hifihr_amd.ops", stub)
    model = types.SimpleNamespace(hand_model="mano", root_id=9, hand_layer=types.SimpleNamespace(handle=object()))
    B = 2
    outputs = {"pose_params": torch.zeros(B, 48), "shape_params": torch.zeros(B, 10), "joints": torch.zeros(B, 21, 3),
               "mano_verts": torch.zeros(B, 778, 3), "re_img": torch.ones(B, 3, 4, 4)}
    J, t, K, uv, conf, _ = _skeleton(B, 5)
    outputs["joints"] = J.float()
    ex = {"Ks": K.float(), "open_2dj": uv.float(), "open_2dj_con": conf.float().unsqueeze(-1), "j2d_gt": uv.float() + 1.0}
    return stub, model, outputs, ex, t


def test_option_off_makes_no_call(stubbed):
    stub, model, outputs, ex, _ = stubbed
    out, did = fit.refine_outputs(model, outputs, ex, options.make_args(None))
    assert out is outputs and did is False and stub.calls == []


def test_option_on_refines_joints_and_keeps_the_render(stubbed):
    stub, model, outputs, ex, t = stubbed
    args = options.make_args(None, fit_keypoints=True, fit_iters=9, fit_w_shape=0.3)
    out, did = fit.refine_outputs(model, outputs, ex, args)
    assert did is True and [c[0] for c in stub.calls] == ["mano_fit", "mano_full"]            # ONE mano_full at the result
    kw = stub.calls[0][1]
    assert kw["iters"] == 9 and kw["weights"] == (1.0, 1.0, 0.0, 1.0, 0.3, 0.01) and kw["root_id"] == 9
    assert float((kw["root"].double() - t).abs().max()) < 1e-4                                # no root given: root_from_keypoints
    assert torch.equal(stub.calls[1][1]["pose"], torch.ones(2, 48))                           # ... at the REFINED parameters
    assert float(out["joints"][0, 0, 0]) == 0.25 and float(out["mano_verts"][0, 0, 0]) == 0.5 and out["re_img"] is outputs["re_img"]
    assert out["fit_trace"].shape == (2, 10, 8) and out["j2d"].shape == (2, 21, 2) and outputs["joints"] is not out["joints"]
    # a given root is the start; the pass's own root joint is handed on
    stub.calls.clear()
    fit.refine_outputs(model, outputs, ex, args, root_xyz=torch.full((2, 1, 3), 0.5), root_id=0)
    assert torch.equal(stub.calls[0][1]["root"], torch.full((2, 3), 0.5)) and stub.calls[0][1]["root_id"] == 0 and stub.calls[1][1]["root_id"] == 0


def test_target_selection(stubbed):
    stub, model, outputs, ex, _ = stubbed
    args = options.make_args(None, fit_keypoints=True, fit_target="j2d_gt")
    fit.refine_outputs(model, outputs, ex, args)
    assert bool((stub.calls[0][1]["conf"] == 1).all())
    stub.calls.clear()
    del ex["j2d_gt"]
    out, did = fit.refine_outputs(model, outputs, ex, args)                                   # the batch does not carry the target
    assert did is False and out is outputs and stub.calls == []
    with pytest.raises(ValueError):
        fit.refine_outputs(model, outputs, ex, options.make_args(None, fit_keypoints=True, fit_target="heatmap"))


def test_nimble_is_refused(stubbed):
    stub, model, outputs, ex, _ = stubbed
    model.hand_model = "nimble"
    with pytest.raises(NotImplementedError, match="NIMBLE"):
        fit.fit_keypoints(model, outputs, ex["open_2dj"], ex["open_2dj_con"], ex["Ks"])
    assert stub.calls == []


def test_fit_log_line(capsys):
    import train_hrnet
    train_hrnet.fit_keypoints_log(options.make_args(None), 0)
    assert capsys.readouterr().out == ""
    train_hrnet.fit_keypoints_log(options.make_args(None, fit_keypoints=True, fit_iters=5), 3)
    assert "REFINED by 5 fit iterations" in capsys.readouterr().out
    train_hrnet.fit_keypoints_log(options.make_args(None, fit_keypoints=True), 0)
    assert "network's own" in capsys.readouterr().out


class _Cache:
    """Stands in for FreiHandDeviceCache on the CPU: batch() carries no detections (as the real one), batch_examples() does."""

    def __init__(self, n, with_detections):
        J, t, K, uv, conf, _ = _skeleton(n, 9)
        self.n, self.J, self.K, self.uv, self.conf = n, J.float(), K.float(), uv.float(), conf.float().unsqueeze(-1)
        self.open_2dj = self.uv if with_detections else None
        self.calls = []

    def _common(self, idx):
        B = len(idx)
        return {"Ks": self.K[idx], "joints": self.J[idx], "verts": torch.zeros(B, 778, 3), "scales": torch.ones(B), "idxs": idx}

    def batch(self, idx, rots=None):
        self.calls.append("batch")
        c = self._common(idx)
        return {"trans_images": torch.zeros(len(idx), 3, 8, 8), "trans_masks": torch.zeros(len(idx), 3, 8, 8), "trans_Ks": c["Ks"],
                "trans_joints": c["joints"], "trans_verts": c["verts"], "scales": c["scales"], "idxs": idx}

    def batch_examples(self, idx, rots=None):
        self.calls.append("batch_examples")
        assert rots is not None and not np.asarray(rots).any()
        c = self._common(idx)
        K = c["Ks"]
        c.update(imgs=torch.zeros(len(idx), 3, 8, 8), Ps=torch.cat([K, torch.zeros_like(K[:, :, :1])], 2), open_2dj=self.uv[idx],
                 open_2dj_con=self.conf[idx])
        return c


class _Collector:
    def __init__(self):
        self.seen = []

    def collect(self, out, ex, dat_name, render=False):
        self.seen.append(out)

    def summary(self, *a, **k):
        return {"batches": len(self.seen)}


def _run_eval(monkeypatch, stub, cache, args):
    import train_hrnet
    ev = _Collector()
    monkeypatch.setattr(train_hrnet, "make_evaluator", lambda a, d: ev)

    class _Model:
        hand_model, root_id, hand_layer = "mano", 9, types.SimpleNamespace(handle=object())
        eval = train = lambda self: self

        def __call__(self, dat_name, mode_train, imgs, Ks=None, root_xyz=None):
            B = imgs.shape[0]
            return {"pose_params": torch.zeros(B, 48), "shape_params": torch.zeros(B, 10), "joints": torch.zeros(B, 21, 3),
                    "mano_verts": torch.zeros(B, 778, 3)}

    summary = train_hrnet.run_evaluation(_Model(), cache, {"joints": None, "verts": None}, args, "cpu")
    return ev, summary


def test_run_evaluation_refines_every_batch_that_carries_detections(stubbed, monkeypatch, capsys):
    """The batch path of run_evaluation itself: with the option on and a cache that holds detections the batches come with open_2dj and
    every one of them is refined; the same cache with the option off is read through the two calls made before and nothing is fitted."""
    stub = stubbed[0]
    args = options.make_args(None, fit_keypoints=True, fit_iters=4, val_batch=2, render=False)
    cache = _Cache(5, with_detections=True)
    ev, summary = _run_eval(monkeypatch, stub, cache, args)
    fits = [c for c in stub.calls if c[0] == "mano_fit"]
    assert summary == {"batches": 3} and len(fits) == 3 and cache.calls == ["batch_examples"] * 3
    assert all("fit_trace" in o and float(o["joints"][0, 0, 0]) == 0.25 for o in ev.seen)
    assert "REFINED by 4 fit iterations" in capsys.readouterr().out
    # option off: the earlier path, no fit
    stub.calls.clear()
    cache = _Cache(5, with_detections=True)
    ev, _ = _run_eval(monkeypatch, stub, cache, options.make_args(None, val_batch=2, render=False))
    assert stub.calls == [] and cache.calls == ["batch"] * 3 and all("fit_trace" not in o for o in ev.seen)
    assert capsys.readouterr().out == ""
    # option on, a cache without detections: nothing to fit to, and the log says so
    cache = _Cache(5, with_detections=False)
    ev, _ = _run_eval(monkeypatch, stub, cache, args)
    assert stub.calls == [] and cache.calls == ["batch"] * 3 and "network's own" in capsys.readouterr().out


def test_eval_arrays_keep_their_detections_only_for_the_fit(tmp_path):
    import train_hrnet
    n, m = 4, 3
    z = dict(images=np.zeros((n, 8, 8, 3), np.uint8), masks=np.zeros((n, 8, 8), np.uint8), Ks=np.zeros((n, 3, 3), np.float32),
             joints=np.zeros((n, 21, 3), np.float32), verts=np.zeros((n, 778, 3), np.float32),
             open_2dj=np.ones((n, 21, 2), np.float32), open_2dj_con=np.ones((n, 21, 1), np.float32))
    z.update({"eval_" + k: v[:m] for k, v in list(z.items())})
    path = str(tmp_path / "cache.npz")
    np.savez(path, **z)
    cli = types.SimpleNamespace(freihand_cache=path, openpose_keypoints=None)
    tr, ev = train_hrnet.load_or_make_dataset(cli, None, "cpu")
    assert "open_2dj" in tr and "open_2dj" not in ev                                          # as before
    tr, ev = train_hrnet.load_or_make_dataset(cli, None, "cpu", eval_keypoints=True)
    assert ev["open_2dj"].shape == (m, 21, 2) and ev["open_2dj_con"].shape == (m, 21, 1)

