"""The benchmark metrics on the MI355X: hifihr_point_error_hist / hifihr_fscore_counts through the C ABI on the cases of
tests/test_hostsim_benchmark_metrics.py (tests/benchmark_cases.py), and hifihr_amd.evaluate's pck_auc / fscore / Evaluator(benchmark=True)
end to end.  References: the float64 restatement of tests/benchmark_ref.py, the reference's EvalUtil (tests/golden/benchmark_metrics.npz)."""
import os

import numpy as np
import pytest
import torch

import benchmark_cases as bc
import benchmark_ref as br

pytestmark = pytest.mark.gpu
_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


@pytest.mark.parametrize("shape", bc.HIST_SHAPES, ids=_ids)
def test_histogram_counts_equal_the_restatement(lib, shape):
    bc.hist_raw_case(lib, "cuda", *shape)


def test_histogram_skips_an_invisible_keypoint(lib):
    bc.hist_masked_case(lib, "cuda")


def test_histogram_counts_exact_hits_in_their_bin(lib):
    bc.hist_constructed_case(lib, "cuda")


def test_pck_auc_matches_the_reference_evalutil(lib, golden_dir):
    bc.hist_fixture_case(lib, "cuda", golden_dir)


@pytest.mark.parametrize("shape", bc.FSCORE_SHAPES, ids=_ids)
def test_fscore_counts_equal_the_restatement(lib, shape):
    bc.fscore_raw_case(lib, "cuda", *shape)


def test_fscore_constructed_cases(lib):
    bc.fscore_constructed_case(lib, "cuda")


def test_aligned_forms_are_bracketed_by_the_float64_reference(lib, golden_dir):
    bc.aligned_case(lib, "cuda", golden_dir)


def test_refusals_leave_the_outputs_untouched(lib):
    bc.refusal_case(lib, "cuda")


def test_fscore_function_divides_by_each_set(lib):
    """hifihr_amd.evaluate.fscore: float64 [B, T] on the device; precision over Np, recall over Ng."""
    from hifihr_amd.evaluate import fscore
    pred, gt, thr = bc._fscore_inputs(2, 300, 200, 2)
    assert bc._fscore_gap_ok(pred, gt, thr)
    F, P, R = fscore(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), tuple(thr))
    assert F.is_cuda and F.dtype == torch.float64 and tuple(F.shape) == (2, 2)
    ref = br.fscore_counts(pred, gt, thr)
    Fr, Pr, Rr = br.fscore_from_counts(ref, 300, 200)
    assert np.array_equal(P.cpu().numpy(), ref[:, 0] / 300.0) and np.array_equal(R.cpu().numpy(), ref[:, 1] / 200.0)
    assert np.abs(F.cpu().numpy() - Fr).max() <= 1e-15 and ref[:, 0].sum() > 0 and ref[:, 1].sum() > 0


def _evaluator(g, benchmark):
    from hifihr_amd.evaluate import Evaluator
    ev = Evaluator(benchmark=benchmark)
    for sl in (slice(0, 4), slice(4, 6)):
        ev.collect({"joints": torch.from_numpy(g["pr_j"][sl]).cuda(), "mano_verts": torch.from_numpy(g["pr_v"][sl]).cuda()}, {}, "FreiHand", render=False)
    return ev


def test_evaluator_benchmark_keys(lib, golden_dir, monkeypatch):
    from hifihr_amd.evaluate import BENCHMARK_KEYS
    g = np.load(os.path.join(golden_dir, "eval.npz"))
    thr, fthr, ROOT = np.linspace(0.0, 0.05, 100), np.array([0.005, 0.015]), 9
    plain = _evaluator(g, False).summary(g["gt_j"], g["gt_v"])
    assert set(plain) == {"pose_3d", "vert_3d"}                                   # benchmark=False: exactly the old keys ...
    assert plain == _evaluator(g, False).summary(g["gt_j"], g["gt_v"], root_id=ROOT)
    assert _evaluator(g, True).summary() == {}                                     # ... and so without ground truth

    copies = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(tuple(self.shape)), to_host(self, *a, **k))[1])
    ev = _evaluator(g, True)
    s = ev.summary(g["gt_j"], g["gt_v"])
    s_root = _evaluator(g, True).summary(g["gt_j"], g["gt_v"], root_id=ROOT)
    monkeypatch.undo()
    assert len(copies) == 2, copies                                                # one device-to-host copy per benchmark summary
    assert all(t.is_cuda for t in ev.xyz_pred + ev.verts_pred)
    assert list(s) == ["pose_3d", "vert_3d"] + list(BENCHMARK_KEYS) and len(BENCHMARK_KEYS) == 12
    assert s["pose_3d"] == plain["pose_3d"] and s["vert_3d"] == plain["vert_3d"]
    assert abs(s["xyz_al_mean3d"] - s["pose_3d"]) <= 1e-6 * s["pose_3d"] and abs(s["mesh_al_mean3d"] - s["vert_3d"]) <= 1e-6 * s["vert_3d"]
    for k in BENCHMARK_KEYS:                                                       # root_id moves the un-aligned forms only
        if "_al_" in k:
            assert abs(s_root[k] - s[k]) <= 1e-6 * abs(s[k]), k
    assert s_root["xyz_mean3d"] != s["xyz_mean3d"] and s_root["mesh_mean3d"] != s["mesh_mean3d"]
    # the un-aligned forms against the restatement, on the ground truth as given and relative to its joint ROOT (an fp32 subtraction)
    gt_j, gt_v = g["gt_j"].astype(np.float32), g["gt_v"].astype(np.float32)
    for got, gj, gv in ((s, gt_j, gt_v), (s_root, gt_j - gt_j[:, ROOT:ROOT + 1], gt_v - gt_j[:, ROOT:ROOT + 1])):
        for name, pred, gt in (("xyz", g["pr_j"], gj), ("mesh", g["pr_v"], gv)):
            assert br.threshold_gap_ok(br.distances(pred, gt), thr)
            m = br.pck_measures(*br.hist_counts(pred, gt, None, thr), thr)
            assert abs(got[name + "_mean3d"] - m["mean"]) <= 1e-12 and abs(got[name + "_auc3d"] - m["auc"]) <= 1e-12, (name, got, m)
        assert bc._fscore_gap_ok(g["pr_v"], gv, fthr)
        F = br.fscore_from_counts(br.fscore_counts(g["pr_v"], gv, fthr), 778, 778)[0].mean(0)
        assert abs(got["f_score_5"] - F[0]) <= 1e-14 and abs(got["f_score_15"] - F[1]) <= 1e-14
    assert 0 < s["f_al_score_5"] < s["f_al_score_15"] <= 1 and 0 < s["xyz_al_auc3d"] < 1 and 0 < s["mesh_al_auc3d"] < 1
