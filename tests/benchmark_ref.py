"""Float64 numpy restatement of the two count definitions behind the benchmark metrics (include/hifihr.h: hifihr_point_error_hist,
hifihr_fscore_counts), written from the definitions, with a brute-force nearest neighbour.

PCK / AUC: the histogram is EvalUtil's `data <= threshold` (reference utils/fh_utils.py:755-762) binned; what is made of it is pinned
to the reference's own EvalUtil by tests/golden/benchmark_metrics.npz (tools/make_benchmark_golden.py).

F-score: the FreiHAND benchmark's calculate_fscore (nearest-neighbour distance of every point to the other set, strictly below the
threshold; F = 2 P R / (P + R), 0 when P + R = 0).  It has NO counterpart under the reference tree, and neither the benchmark's eval.py
nor open3d is available where these fixtures are made: parity with the benchmark's script is UNPINNED, this restatement is the test's
only reference for it.

Inputs are fp32 values widened to float64, so the differences are exact and d^2 = (dx dx + dy dy) + dz dz rounds as the kernels' does."""
import numpy as np

_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def distances(pred, gt):
    d = np.asarray(pred, np.float64) - np.asarray(gt, np.float64)
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def hist_counts(pred, gt, vis, thr):
    """-> (hist int64 [K, T+1], sum float64 [K]): hist[k][t] = #{thr[t-1] < d <= thr[t]}, hist[k][T] = #{d > thr[T-1] or NaN}."""
    d, thr = distances(pred, gt), np.asarray(thr, np.float64)
    n, K = d.shape
    vis = np.ones((n, K), bool) if vis is None else np.asarray(vis) != 0
    hist, sums = np.zeros((K, len(thr) + 1), np.int64), np.zeros(K)
    for k in range(K):
        dk = d[vis[:, k], k]
        cum = np.array([(dk <= t).sum() for t in thr], np.int64)            # NaN <= t is False
        hist[k, :-1] = np.diff(cum, prepend=0)
        hist[k, -1] = len(dk) - cum[-1]
        sums[k] = dk.sum()
    return hist, sums


def cumulative_le(pred, gt, thr):
    """[K, T]: #{d <= thr[t]} per keypoint (all visible)."""
    d = distances(pred, gt)
    return np.stack([(d <= t).sum(0) for t in np.asarray(thr, np.float64)], 1).astype(np.int64)


def nearest(a, b):
    """[len(a)]: distance of every point of a to its nearest point of b, brute force; a pair whose d^2 is NaN is skipped."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty(len(a))
    for lo in range(0, len(a), 512):
        d = a[lo:lo + 512, None, :] - b[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        out[lo:lo + 512] = np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(1))
    return out


def fscore_distances(pred, gt):
    """Per sample: (nearest(pred -> gt), nearest(gt -> pred))."""
    return [(nearest(p, g), nearest(g, p)) for p, g in zip(pred, gt)]


def fscore_counts(pred, gt, thr, shift=0.0):
    """int64 [B, 2, T]: counts of nearest distances < thr + shift (STRICT)."""
    dist = fscore_distances(pred, gt)
    return np.array([[[int((d < t + shift).sum()) for t in thr] for d in pair] for pair in dist], np.int64)


def fscore_from_counts(counts, Np, Ng):
    P, R = counts[:, 0] / float(Np), counts[:, 1] / float(Ng)
    S = P + R
    return np.where(S > 0, 2 * P * R / np.where(S > 0, S, 1.0), 0.0), P, R


def pck_measures(hist, sums, thr):
    """EvalUtil.get_measures from counts, written independently of hifihr_amd.evaluate.pck_measures: a loop over keypoints like the reference's."""
    thr = np.asarray(thr, np.float64)
    norm = _trapezoid(np.ones_like(thr), thr)
    means, aucs, curves = [], [], []
    for k in range(hist.shape[0]):
        vis = int(hist[k].sum())
        if vis == 0:
            continue
        curve = np.cumsum(hist[k, :-1]) / float(vis)
        means.append(sums[k] / vis); aucs.append(_trapezoid(curve, thr) / norm); curves.append(curve)
    return {"mean": float(np.mean(means)), "auc": float(np.mean(aucs)), "pck_curve": np.mean(np.array(curves), 0), "thresholds": thr}


def threshold_gap_ok(d, thr, rel=1e-9, allow=()):
    """No finite distance lies within rel x threshold of a threshold -- except exact hits on the thresholds listed in `allow`."""
    d = np.asarray(d, np.float64).ravel()
    d = d[np.isfinite(d)]
    for t in np.asarray(thr, np.float64):
        near = np.abs(d - t) <= rel * abs(t)
        if t in allow:
            near &= d != t
        if near.any():
            return False
    return True
