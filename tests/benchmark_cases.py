"""Shared bodies of the benchmark-metric tests (hifihr_point_error_hist, hifihr_fscore_counts and what hifihr_amd.evaluate makes of
their counts): tests/test_hostsim_benchmark_metrics.py runs them on the emulator (device='cpu'), tests/test_gpu_benchmark_metrics.py
on the MI355X (device='cuda').

Counts are compared for EQUALITY with the float64 restatement of tests/benchmark_ref.py.  That is sound only while no distance sits
on a threshold by less than the two computations may differ, so every case first asserts, from the restatement alone, that no float64
distance lies within 1e-9 x threshold of a threshold (the two sides differ by a few ulp, 1e-16 relative, at the most) -- except the
exact hits a case constructs, which are exact in both (differences of fp32 values, squares and roots of powers of two).
The aligned forms pass through an fp32 buffer: there the counts are bracketed, see `aligned_case`."""
import ctypes
import os

import numpy as np
import torch

import benchmark_ref as br
import kernel_cases as kc

EINVAL = -1
HIST_SHAPES = [(1, 1, 1), (3, 1, 2), (257, 21, 100), (5, 778, 100), (4, 23, 128)]          # (n, K, T); 257: past one 64-sample stride x 4
FSCORE_SHAPES = [(1, 1, 1, 2), (2, 3, 5, 8), (3, 778, 778, 2), (1, 255, 257, 8), (1, 256, 256, 2), (1, 1025, 1023, 2), (1, 511, 513, 2),
                 (1, 5990, 778, 2), (2, 63, 65, 2)]                                          # (B, Np, Ng, T); tile 512, 64 queries a workgroup
_DBL_P = ctypes.POINTER(ctypes.c_double)


def _thr(T):
    return np.linspace(0.0, 0.05, T) if T > 1 else np.array([0.025])


def _hand_pair(rng, shape, noise=0.012):
    gt = (0.05 * rng.standard_normal(shape)).astype(np.float32)
    pred = (gt + noise * rng.standard_normal(shape) * rng.uniform(0.2, 2.5, shape[:-1] + (1,))).astype(np.float32)
    return pred, gt


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def run_hist(lib, device, pred, gt, vis, thr):
    """-> (hist [K, T+1], sum [K]) as numpy; the outputs start as garbage and the call runs twice: the same bits both times."""
    K, T = pred.shape[1], len(thr)
    p, g, v = _t(pred, device), _t(gt, device), _t(vis, device)
    outs = []
    for fill in (0x5A5A5A5A, -7):
        hist = torch.full((K, T + 1), fill, dtype=torch.int32, device=device)
        sums = torch.full((K,), float(fill) * 1e300, dtype=torch.float64, device=device)
        lib.point_error_hist(p, g, v, thr, hist, sums)
        outs.append((hist.cpu().numpy(), sums.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]), "hist: two calls differ"
    assert np.array_equal(outs[0][1].view(np.int64), outs[1][1].view(np.int64)), "sum_d: two calls differ in their bits"
    return outs[0]


def run_fscore(lib, device, pred, gt, thr):
    B, T = pred.shape[0], len(thr)
    p, g = _t(pred, device), _t(gt, device)
    outs = []
    for fill in (0x5A5A5A5A, -7):
        counts = torch.full((B, 2, T), fill, dtype=torch.int32, device=device)
        lib.fscore_counts(p, g, thr, counts)
        outs.append(counts.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "fscore counts: two calls differ"
    return outs[0]


def _sums_close(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    print(f"[benchmark] sum_d worst relative error {float((err / np.maximum(np.abs(ref[ok]), 1e-300)).max()) if ok.any() else 0.0:.3e}")
    assert (err <= 1e-12 * np.abs(ref[ok])).all(), (got, ref)


# ---- histogram ------------------------------------------------------------------------------------------------------------------------
def hist_raw_case(lib, device, n, K, T):
    rng = np.random.default_rng(1000 + n + 7 * K + 13 * T)
    pred, gt = _hand_pair(rng, (n, K, 3))
    thr = _thr(T)
    assert br.threshold_gap_ok(br.distances(pred, gt), thr), "a distance sits on a threshold: take another seed"
    ref_hist, ref_sum = br.hist_counts(pred, gt, None, thr)
    hist, sums = run_hist(lib, device, pred, gt, None, thr)
    assert np.array_equal(hist, ref_hist), (np.argwhere(hist != ref_hist)[:5], hist[hist != ref_hist][:5], ref_hist[hist != ref_hist][:5])
    assert (hist.sum(1) == n).all()
    _sums_close(sums, ref_sum)


def hist_masked_case(lib, device):
    """Keypoint 2 is invisible in every sample (its row is zeros and the means skip it), the others in about a third of them."""
    from hifihr_amd.evaluate import pck_measures
    n, K, T = 70, 6, 100
    rng = np.random.default_rng(77)
    pred, gt = _hand_pair(rng, (n, K, 3))
    vis = (rng.uniform(size=(n, K)) > 0.35).astype(np.uint8)
    vis[:, 2] = 0
    vis[rng.integers(0, n, 5), 4] = 200                                 # any non-zero byte is "visible"
    thr = _thr(T)
    assert br.threshold_gap_ok(br.distances(pred, gt), thr)
    ref_hist, ref_sum = br.hist_counts(pred, gt, vis, thr)
    hist, sums = run_hist(lib, device, pred, gt, vis, thr)
    assert np.array_equal(hist, ref_hist) and not hist[2].any() and sums[2] == 0.0 and hist[[0, 1, 3, 4, 5]].sum() == int((vis != 0).sum())
    _sums_close(sums, ref_sum)
    got, want = pck_measures(hist, sums, thr), br.pck_measures(ref_hist, ref_sum, thr)
    # what "skipped" means: the measures of the five other keypoints alone
    alone = br.pck_measures(np.delete(ref_hist, 2, 0), np.delete(ref_sum, 2), thr)
    for m in (want, alone):
        assert abs(got["mean"] - m["mean"]) <= 1e-12 and abs(got["auc"] - m["auc"]) <= 1e-12
        assert float(np.abs(got["pck_curve"] - m["pck_curve"]).max()) <= 1e-12


def hist_constructed_case(lib, device):
    """Exact hits: d = 0.5 on thr[1] = 0.5 counts IN bin 1 (<=), d = 0 counts at thr[0] = 0, a NaN coordinate and d = 2 land in the last bin."""
    thr = np.linspace(0.0, 1.0, 3)
    gt = np.full((4, 2, 3), 0.25, np.float32)
    pred = gt.copy()
    pred[0, :, 0] += 0.5                                                # d = 0.5 exactly, both keypoints
    pred[2, 0, 1] = np.nan                                              # sample 2: keypoint 0 not a number ...
    pred[2, 1, 0] += 0.75                                               # ... keypoint 1 in (0.5, 1]
    pred[3, :, 2] += 2.0                                                # beyond the last threshold
    d = br.distances(pred, gt)
    assert d[0, 0] == 0.5 and d[1, 0] == 0.0 and np.isnan(d[2, 0]) and br.threshold_gap_ok(d, thr, allow=(0.0, 0.5))
    hist, sums = run_hist(lib, device, pred, gt, None, thr)
    ref_hist, ref_sum = br.hist_counts(pred, gt, None, thr)
    assert np.array_equal(ref_hist, [[1, 1, 0, 2], [1, 1, 1, 1]])       # the restatement itself, against the counts by hand
    assert np.array_equal(hist, ref_hist), hist
    assert np.isnan(sums[0]) and sums[1] == 0.5 + 0.0 + 0.75 + 2.0
    _sums_close(sums, ref_sum)


def hist_fixture_case(lib, device, golden_dir):
    """The reference's own EvalUtil (tests/golden/benchmark_metrics.npz): thresholds, curve, AUC and mean to 1e-12 absolute."""
    from hifihr_amd import evaluate
    g = np.load(os.path.join(golden_dir, "benchmark_metrics.npz"))
    for name in ("joints", "mesh", "masked"):
        pred, gt, vis = g[name + "_pred"], g[name + "_gt"], g[name + "_vis"]
        if name == "masked":
            assert not vis[:, 5].any() and vis.min() == 0 and vis[:, [0, 1, 2]].any()
        thr = np.linspace(0.0, 0.05, 100)
        assert br.threshold_gap_ok(br.distances(pred, gt), thr)
        measures = []
        hist, sums = run_hist(lib, device, pred, gt, vis if name == "masked" else None, thr)
        measures.append(evaluate.pck_measures(hist, sums, thr))
        if device == "cuda":                                            # the public function (GPU tensors only)
            measures.append(evaluate.pck_auc(_t(pred, device), _t(gt, device), _t(vis, device) if name == "masked" else None, 0.0, 0.05, 100))
        for m in measures:
            errs = (float(np.abs(m["thresholds"] - g[name + "_thresholds"]).max()), float(np.abs(m["pck_curve"] - g[name + "_curve"]).max()),
                    abs(m["auc"] - float(g[name + "_auc"])), abs(m["mean"] - float(g[name + "_mean"])))
            print(f"[benchmark] {name} vs EvalUtil: thresholds {errs[0]:.2e} curve {errs[1]:.2e} auc {errs[2]:.2e} mean {errs[3]:.2e}")
            assert max(errs) <= 1e-12, (name, errs)


# ---- F-score --------------------------------------------------------------------------------------------------------------------------
def _fscore_inputs(B, Np, Ng, T):
    rng = np.random.default_rng(2000 + B + 3 * Np + 5 * Ng)
    pred = (0.05 * rng.standard_normal((B, Np, 3))).astype(np.float32)
    if Np == Ng:
        gt = (pred + 0.006 * rng.standard_normal((B, Ng, 3))).astype(np.float32)[:, rng.permutation(Ng)]
    else:
        gt = (0.05 * rng.standard_normal((B, Ng, 3))).astype(np.float32)
    if max(Np, Ng) < 16:                                                # a handful of points: bring them within reach of the thresholds
        pred, gt = (pred * 0.1).astype(np.float32), (gt * 0.1).astype(np.float32)
    thr = np.array([0.005, 0.015]) if T == 2 else np.linspace(0.002, 0.03, T)
    return pred, gt, thr


def _fscore_gap_ok(pred, gt, thr, allow=()):
    return br.threshold_gap_ok(np.concatenate([np.concatenate(pair) for pair in br.fscore_distances(pred, gt)]), thr, allow=allow)


def _check_f(counts, Np, Ng):
    from hifihr_amd.evaluate import fscore_from_counts
    F, P, R = (x.numpy() for x in fscore_from_counts(torch.from_numpy(counts), Np, Ng))
    Fr, Pr, Rr = br.fscore_from_counts(counts.astype(np.int64), Np, Ng)
    assert F.dtype == np.float64 and np.isfinite(F).all()
    assert np.abs(F - Fr).max() <= 1e-15 and np.array_equal(P, Pr) and np.array_equal(R, Rr)
    assert np.abs(P * Np - counts[:, 0]).max() <= 1e-9 and np.abs(R * Ng - counts[:, 1]).max() <= 1e-9    # precision over Np, recall over Ng
    return F, P, R


def fscore_raw_case(lib, device, B, Np, Ng, T):
    pred, gt, thr = _fscore_inputs(B, Np, Ng, T)
    assert _fscore_gap_ok(pred, gt, thr), "a nearest distance sits on a threshold: take another seed"
    ref = br.fscore_counts(pred, gt, thr)
    counts = run_fscore(lib, device, pred, gt, thr)
    assert np.array_equal(counts, ref), (counts, ref)
    _check_f(counts, Np, Ng)
    if Np > 100:
        assert 0 < ref.sum() < ref.size * max(Np, Ng), "the case counts nothing or everything: it would not see a wrong neighbour"


def fscore_constructed_case(lib, device):
    z = lambda *rows: np.array([rows], np.float32)
    # the distance EQUALS the threshold: not counted (strict), counted under the next one
    pred, gt, thr = z([0, 0, 0]), z([0.5, 0, 0]), np.array([0.5, 0.75])
    assert _fscore_gap_ok(pred, gt, thr, allow=(0.5,))
    c = run_fscore(lib, device, pred, gt, thr)
    assert np.array_equal(c, [[[0, 1], [0, 1]]]) and np.array_equal(c, br.fscore_counts(pred, gt, thr))
    F, _, _ = _check_f(c, 1, 1)
    assert F.tolist() == [[0.0, 1.0]]
    # the sets farther apart than every threshold: P + R = 0, F = 0 and not NaN
    pred = np.array([[[0, 0, 0], [0.1, 0, 0]]], np.float32)
    gt, thr = pred + np.float32(10.0), np.array([0.005, 0.015])
    c = run_fscore(lib, device, pred, gt, thr)
    assert not c.any() and np.array_equal(c, br.fscore_counts(pred, gt, thr))
    F, P, R = _check_f(c, 2, 2)
    assert F.tolist() == [[0.0, 0.0]] and not P.any() and not R.any()
    # pred == gt: every point counted, F = 1
    pred = (0.05 * np.random.default_rng(5).standard_normal((2, 37, 3))).astype(np.float32)
    c = run_fscore(lib, device, pred, pred.copy(), thr)
    assert (c == 37).all() and np.array_equal(c, br.fscore_counts(pred, pred, thr))
    assert (_check_f(c, 37, 37)[0] == 1.0).all()
    # two prediction points equidistant (0.25) from the one ground-truth point; Np != Ng: precision over 2, recall over 1
    pred, gt, thr = z([-0.25, 0, 0], [0.25, 0, 0]), z([0, 0, 0]), np.array([0.5, 0.25, 0.125])
    assert _fscore_gap_ok(pred, gt, thr, allow=(0.25,))
    c = run_fscore(lib, device, pred, gt, thr)
    assert np.array_equal(c, [[[2, 0, 0], [1, 0, 0]]]) and np.array_equal(c, br.fscore_counts(pred, gt, thr))
    F, P, R = _check_f(c, 2, 1)
    assert P[0, 0] == 1.0 and R[0, 0] == 1.0 and F[0, 0] == 1.0
    # denominators: one of two predicted points near the single ground-truth point -> P = 1/2, R = 1/1, F = 2/3
    pred, gt, thr = z([0, 0, 0], [1, 0, 0]), z([0.001, 0, 0]), np.array([0.005])
    c = run_fscore(lib, device, pred, gt, thr)
    F, P, R = _check_f(c, 2, 1)
    assert np.array_equal(c, [[[1], [1]]]) and P[0, 0] == 0.5 and R[0, 0] == 1.0 and abs(F[0, 0] - 2.0 / 3.0) <= 1e-15
    # a point that is not a number is never near anything and never anyone's neighbour (include/hifihr.h)
    pred[0, 1, 0] = np.nan
    c = run_fscore(lib, device, pred, gt, thr)
    assert np.array_equal(c, [[[1], [1]]]) and np.array_equal(c, br.fscore_counts(pred, gt, thr))


# ---- aligned forms --------------------------------------------------------------------------------------------------------------------
def aligned_case(lib, device, golden_dir):
    """The `_al_` forms count on the fp32 output of the device's alignment; the reference is float64 (the restatement of align_w_scale,
    kernel_cases.procrustes_contract_ref, on the inputs of tests/golden/eval.npz).  Storing an aligned coordinate as fp32 moves it by at
    most 2^-24 max|coordinate|, a distance by at most sqrt(3) x that; gap = 2^-22 max|coordinate| is that bound rounded up.  So, per cell,
        count_ref(d <= thr - gap) <= cumulative count <= count_ref(d <= thr + gap)             (F-score: the same with <)
    and the AUC / F values lie between those of the two bounds.  The bracket hides nothing: from the reference alone, at most 2 % of the
    cells have two different bounds."""
    g = np.load(os.path.join(golden_dir, "eval.npz"))
    thr, fthr = np.linspace(0.0, 0.05, 100), np.array([0.005, 0.015])
    for pk, gk in (("pr_j", "gt_j"), ("pr_v", "gt_v")):
        pred, gt = g[pk].astype(np.float32), g[gk].astype(np.float32)
        ref = kc.procrustes_contract_ref(torch.from_numpy(pred), torch.from_numpy(gt))
        assert ref["unique"].all()
        n, K = pred.shape[:2]
        gap = 2.0 ** -22 * max(float(np.abs(ref["aligned"]).max()), float(np.abs(gt).max()))
        gt64 = gt.astype(np.float64)
        d = np.sqrt(((ref["aligned"] - gt64) ** 2).sum(2))
        lo = np.stack([(d <= t - gap).sum(0) for t in thr], 1)
        hi = np.stack([(d <= t + gap).sum(0) for t in thr], 1)
        share = float((lo != hi).mean())
        print(f"[benchmark] aligned {pk}: gap {gap:.2e}, cells with two bounds {share:.4%}")
        assert share <= 0.02
        p, q = _t(pred, device), _t(gt, device)
        aligned, err = torch.empty_like(p), torch.empty(n, device=device)
        lib.procrustes_error(p, q, aligned, err)
        al = aligned.cpu().numpy()
        hist, sums = run_hist(lib, device, al, gt, None, thr)
        cum = np.cumsum(hist[:, :-1], 1)
        assert (lo <= cum).all() and (cum <= hi).all(), np.argwhere((lo > cum) | (cum > hi))[:5]
        as_hist = lambda c: np.concatenate([np.diff(c, axis=1, prepend=0), n - c[:, -1:]], 1)
        m_lo, m, m_hi = (br.pck_measures(as_hist(c), sums, thr) for c in (lo, cum, hi))
        assert m_lo["auc"] <= m["auc"] <= m_hi["auc"], (m_lo["auc"], m["auc"], m_hi["auc"])
        assert abs(m["mean"] - float(d.mean())) <= gap                                  # every distance within gap of the reference's
        assert abs(m["mean"] - float(err.double().sum()) / (n * K)) <= 1e-6 * m["mean"]    # = the MPJPE / MPVPE the entry itself reports
        if K < 100:
            continue
        # F-score of the aligned mesh
        dist = br.fscore_distances(ref["aligned"], gt64)
        f_lo = np.array([[[int((x < t - gap).sum()) for t in fthr] for x in pair] for pair in dist])
        f_hi = np.array([[[int((x < t + gap).sum()) for t in fthr] for x in pair] for pair in dist])
        assert float((f_lo != f_hi).mean()) <= 0.02
        c = run_fscore(lib, device, al, gt, fthr)
        assert (f_lo <= c).all() and (c <= f_hi).all(), (f_lo, c, f_hi)
        F_lo, F, F_hi = (br.fscore_from_counts(x, K, K)[0] for x in (f_lo, c, f_hi))
        assert (F_lo <= F).all() and (F <= F_hi).all() and 0 < F.mean() < 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(lib, device, name, args, outs, what):
    before = [o.clone() for o in outs]
    if device == "cpu":
        kc.launch_log(lib)
    rc = getattr(lib.c, name)(*args)
    assert rc == EINVAL, f"{name}: {what}: returned {rc}, not HIFIHR_EINVAL"
    if device == "cpu":
        left = kc.launch_log(lib)
        assert not left, f"{name}: {what}: refused but launched {left}"
    else:
        torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o.view(torch.uint8), b.view(torch.uint8)), f"{name}: {what}: refused but wrote an output"


def refusal_case(lib, device):
    from hifihr_amd._lib import _fp as fp
    ip, vp = lambda t: ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int32)), lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda a: a.ctypes.data_as(_DBL_P)
    n, K, T = 5, 3, 4
    pred, gt = (_t(a, device) for a in _hand_pair(np.random.default_rng(1), (n, K, 3)))
    hist = torch.full((K, 128 + 2), 0x5A5A5A5A, dtype=torch.int32, device=device)
    sums = torch.full((K,), -3e300, dtype=torch.float64, device=device)
    good = np.linspace(0.0, 0.05, 129)
    bad_thr = {"nan": [0.0, np.nan, 0.02, 0.03], "inf": [0.0, 0.01, 0.02, np.inf], "-inf": [-np.inf, 0.01, 0.02, 0.03], "equal": [0.0, 0.01, 0.01, 0.03],
               "decreasing": [0.0, 0.02, 0.01, 0.03]}
    base = dict(pred=fp(pred), gt=fp(gt), n=n, K=K, thr=dp(good), T=T, hist=ip(hist), sums=vp(sums))
    cases = [("pred NULL", dict(pred=None)), ("gt NULL", dict(gt=None)), ("thr NULL", dict(thr=None)), ("hist NULL", dict(hist=None)),
             ("sum NULL", dict(sums=None)), ("n = 0", dict(n=0)), ("n < 0", dict(n=-1)), ("K = 0", dict(K=0)), ("K < 0", dict(K=-2)),
             ("T = 0", dict(T=0)), ("T < 0", dict(T=-1)), ("T = 129", dict(T=129))]
    keep = []
    for what, vals in bad_thr.items():
        keep.append(np.array(vals, np.float64))
        cases.append((f"threshold {what}", dict(thr=dp(keep[-1]))))
    for what, change in cases:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_point_error_hist",
                 (a["pred"], a["gt"], None, a["n"], a["K"], a["thr"], a["T"], a["hist"], a["sums"], None), (hist, sums), what)
    lib.point_error_hist(pred, gt, None, good[:128], hist[:, :129].contiguous(), sums)          # T = 128 itself is accepted

    B, Np, Ng, T = 2, 5, 4, 2
    pred, gt = _t(np.zeros((B, Np, 3), np.float32), device), _t(np.ones((B, Ng, 3), np.float32), device)
    counts = torch.full((B, 2, 8), 0x5A5A5A5A, dtype=torch.int32, device=device)
    good = np.linspace(0.005, 0.05, 9)
    base = dict(pred=fp(pred), gt=fp(gt), B=B, Np=Np, Ng=Ng, thr=dp(good), T=T, counts=ip(counts))
    cases = [("pred NULL", dict(pred=None)), ("gt NULL", dict(gt=None)), ("thr NULL", dict(thr=None)), ("counts NULL", dict(counts=None)),
             ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("Np = 0", dict(Np=0)), ("Np < 0", dict(Np=-3)), ("Ng = 0", dict(Ng=0)), ("Ng < 0", dict(Ng=-1)),
             ("T = 0", dict(T=0)), ("T < 0", dict(T=-1)), ("T = 9", dict(T=9))]
    for what, vals in {"nan": [0.005, np.nan], "inf": [np.inf, 0.015], "zero": [0.005, 0.0], "negative": [-0.005, 0.015]}.items():
        keep.append(np.array(vals, np.float64))
        cases.append((f"threshold {what}", dict(thr=dp(keep[-1]))))
    for what, change in cases:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_fscore_counts", (a["pred"], a["gt"], a["B"], a["Np"], a["Ng"], a["thr"], a["T"], a["counts"], None), (counts,), what)
    lib.fscore_counts(pred, gt, good[:8], counts)                                                # T = 8 itself is accepted
    assert not counts.cpu().numpy().any()                                                        # the sets are sqrt(3) apart
