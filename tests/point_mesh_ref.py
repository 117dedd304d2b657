"""The float64 restatement of the point-to-mesh distance as include/hifihr.h defines it ("Point-to-mesh distance"; csrc/point_mesh.hip), the
reference of tests/point_mesh_cases.py: a numpy form (values, choices, weights and the analytic gradient) and a torch form for autograd.

The numpy form evaluates the same expressions in the same order as the kernel on the float32 inputs widened to float64; numpy evaluates each
operation by itself (no contraction), the region chain is a first-match selection and the one division per pair is IEEE-rounded, so d2, the
arg-min (ties to the lowest index: np.argmin returns the FIRST occurrence, and a later chunk of points replaces an earlier one only when
strictly smaller) and the weights are the kernel's bits.  Points are taken in chunks so that the larger cases stay within a few hundred MB.
The gradient takes the choices and the weights as constants and sums in ascending index order (np.add.at is unbuffered and walks its index
array in order)."""
import numpy as np

CHUNK = 256


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def face_records(v, faces):
    """v [V, 3] float64, faces [F, 3] (clamped into [0, V)) -> a, ab, ac [F, 3], abab, abac, acac [F]"""
    f = np.clip(np.asarray(faces, np.int64), 0, v.shape[0] - 1)
    a = v[f[:, 0]]
    ab, ac = v[f[:, 1]] - a, v[f[:, 2]] - a
    return a, ab, ac, _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)


def closest(ap, ab, ac, abab, abac, acac, xp=np):
    """ap, ab, ac [..., 3], the dot products [...] (broadcast against each other) -> (w0, w1, w2, d2, region), float64.  xp: numpy, or torch
    for the autograd form (tests call closest_torch)."""
    where = xp.where
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4, d5, d6 = d1 - abab, d2 - abac, d1 - abac, d2 - acac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2, e3a, e3b = d1 - d3, d2 - d6, d4 - d3, d5 - d6
    e3, den = e3a + e3b, (va + vb) + vc
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (e1 > 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (e2 > 0), (va <= 0) & (e3a >= 0) & (e3b >= 0) & (e3 > 0), den > 0]
    reg = xp.zeros_like(d1) if xp is not np else np.zeros(d1.shape)
    for code in range(6, -1, -1):                        # the FIRST region whose test holds: the earlier ones overwrite the later ones
        reg = where(conds[code], reg * 0 + code, reg)
    one, zero = reg * 0 + 1.0, reg * 0
    num = where(reg == 2, d1, where(reg == 4, d2, where(reg == 5, e3a, where(reg == 6, one, zero))))
    dsel = where(reg == 2, e1, where(reg == 4, e2, where(reg == 5, e3, where(reg == 6, den, one))))
    q = num / dsel
    omq = 1.0 - q
    tv, tw = vb * q, vc * q
    iv = where(tv < 0, zero, where(tv > 1, one, tv))
    rest = 1.0 - iv
    iw = where(tw < 0, zero, where(tw > rest, rest, tw))
    w1 = where(reg == 1, one, where(reg == 2, q, where(reg == 5, omq, where(reg == 6, iv, zero))))
    w2 = where(reg == 3, one, where((reg == 4) | (reg == 5), q, where(reg == 6, iw, zero)))
    w0 = where(reg == 0, one, where((reg == 2) | (reg == 4), omq, where(reg == 6, rest - iw, zero)))
    dx = ap[..., 0] - (ab[..., 0] * w1 + ac[..., 0] * w2)
    dy = ap[..., 1] - (ab[..., 1] * w1 + ac[..., 1] * w2)
    dz = ap[..., 2] - (ab[..., 2] * w1 + ac[..., 2] * w2)
    return w0, w1, w2, (dx * dx + dy * dy) + dz * dz, reg


def residual(pd, a, ab, ac, w):
    """r = p - cp from the stored weights: rows of points against rows of faces, [K, 3]"""
    return (pd - a) - (ab * w[:, 1:2] + ac * w[:, 2:3])


def point_mesh(p, v, faces, w_pf=1.0, w_fp=1.0, gout=1.0, second=False):
    """p [B, N, 3], v [B, V, 3] (float32 values), faces [F, 3].  -> dict: idx_pf [B, N] / idx_fp [B, F] int32, bary_pf [B, N, 3] / bary_fp
    [B, F, 3], min_pf / min_fp float64, sums [B, 2], value (float64, before the one rounding to float32), gp [B, N, 3] / gv [B, V, 3]
    float64 for the gradient `gout` of the value.  BOTH directions are always searched here (the tests compare an unsearched direction's
    arrays with their canaries, not with these); value and gradients honour a weight of exactly 0.  The weights and gout are taken as the
    float32 values the kernel receives.  second=True adds gap_pf / gap_fp: the second-best d2 minus the best of every query."""
    p, v = np.asarray(p, np.float32), np.asarray(v, np.float32)
    faces = np.asarray(faces, np.int64)
    B, N, V, F = p.shape[0], p.shape[1], v.shape[1], faces.shape[0]
    w_pf, w_fp, gout = float(np.float32(w_pf)), float(np.float32(w_fp)), float(np.float32(gout))
    fc = np.clip(faces, 0, V - 1)
    idx_pf, idx_fp = np.zeros((B, N), np.int32), np.zeros((B, F), np.int32)
    min_pf, min_fp = np.zeros((B, N)), np.zeros((B, F))
    bary_pf, bary_fp = np.zeros((B, N, 3)), np.zeros((B, F, 3))
    gap_pf, gap_fp = np.full((B, N), np.inf), np.full((B, F), np.inf)
    gp, gv = np.zeros((B, N, 3)), np.zeros((B, V, 3))
    c_pf, c_fp = w_pf * 2.0 / (B * N), w_fp * 2.0 / (B * F)
    ar_f = np.arange(F)
    for b in range(B):
        pd, vd = p[b].astype(np.float64), v[b].astype(np.float64)
        a, ab, ac, abab, abac, acac = face_records(vd, faces)
        best, besti, bestw, second_fp = np.full(F, np.inf), np.zeros(F, np.int64), np.zeros((F, 3)), np.full(F, np.inf)
        for lo in range(0, N, CHUNK):
            hi = min(N, lo + CHUNK)
            w0, w1, w2, d2, _ = closest(pd[lo:hi, None, :] - a[None], ab[None], ac[None], abab[None], abac[None], acac[None])
            ar = np.arange(hi - lo)
            j = d2.argmin(1)
            idx_pf[b, lo:hi], min_pf[b, lo:hi] = j, d2[ar, j]
            bary_pf[b, lo:hi] = np.stack([w0[ar, j], w1[ar, j], w2[ar, j]], -1)
            i = d2.argmin(0)
            cand = d2[i, ar_f]
            if second:
                if F > 1:
                    gap_pf[b, lo:hi] = np.partition(d2, 1, axis=1)[:, 1] - d2[ar, j]
                rest = np.partition(d2, 1, axis=0)[1] if hi - lo > 1 else np.full(F, np.inf)
                second_fp = np.minimum(np.maximum(best, cand), np.minimum(second_fp, rest))  # the two smallest of both pairs
            take = cand < best                           # strictly: an earlier chunk keeps a tie
            best, besti = np.where(take, cand, best), np.where(take, lo + i, besti)
            bestw = np.where(take[:, None], np.stack([w0[i, ar_f], w1[i, ar_f], w2[i, ar_f]], -1), bestw)
        idx_fp[b], min_fp[b], bary_fp[b] = besti, best, bestw
        gap_fp[b] = second_fp - best
        # gradients: the stored choices and weights as constants
        r_pf = residual(pd, a[idx_pf[b]], ab[idx_pf[b]], ac[idx_pf[b]], bary_pf[b])          # [N, 3]
        r_fp = residual(pd[besti], a, ab, ac, bestw)                                         # [F, 3]
        s_p = np.zeros((N, 3))
        np.add.at(s_p, besti, r_fp)                      # sum over { f : c[f] == i } of r(i, f), ascending f
        zp = np.zeros((N, 3))
        gp[b] = gout * ((zp if w_pf == 0.0 else c_pf * r_pf) + (zp if w_fp == 0.0 else c_fp * s_p))
        acc = np.zeros((F, 3, 3))
        np.add.at(acc, idx_pf[b], bary_pf[b][:, :, None] * r_pf[:, None, :])                 # sum over { i : a[i] == f }, ascending i
        own = bestw[:, :, None] * r_fp[:, None, :]
        zs = np.zeros((F, 3, 3))
        slab = -((zs if w_pf == 0.0 else c_pf * acc) + (zs if w_fp == 0.0 else c_fp * own))
        s_v = np.zeros((V, 3))
        np.add.at(s_v, fc.reshape(-1), slab.reshape(-1, 3))                                  # corners in ascending 3 f + k
        gv[b] = gout * s_v
    sums = np.stack([min_pf.sum(1), min_fp.sum(1)], 1)
    value = (w_pf * np.mean(sums[:, 0] / N) if w_pf != 0.0 else 0.0) + (w_fp * np.mean(sums[:, 1] / F) if w_fp != 0.0 else 0.0)
    out = dict(idx_pf=idx_pf, idx_fp=idx_fp, bary_pf=bary_pf, bary_fp=bary_fp, min_pf=min_pf, min_fp=min_fp, sums=sums, value=float(value),
               gp=gp, gv=gv)
    if second:
        out.update(gap_pf=gap_pf, gap_fp=gap_fp)
    return out


def d2_at(p, v, faces, point_idx, face_idx):
    """The restatement's d2 and closest points for chosen pairs: p [N, 3], v [V, 3] of one sample, index arrays [K] -> (d2 [K], cp [K, 3])"""
    pd, vd = np.asarray(p, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    a, ab, ac, abab, abac, acac = face_records(vd, faces)
    fi, pi = np.asarray(face_idx, np.int64), np.asarray(point_idx, np.int64)
    w0, w1, w2, d2, _ = closest(pd[pi] - a[fi], ab[fi], ac[fi], abab[fi], abac[fi], acac[fi])
    return d2, a[fi] + (ab[fi] * w1[:, None] + ac[fi] * w2[:, None])


def vertex_corner_table(faces, V):
    """-> (off int32 [V + 1], corner int32 [3 F]): the corners 3 f + k of every vertex, ascending inside a vertex (include/hifihr.h)"""
    flat = np.clip(np.asarray(faces, np.int64), 0, V - 1).reshape(-1)
    order = np.argsort(flat, kind="stable")
    off = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=off[1:])
    return off.astype(np.int32), order.astype(np.int32)


def point_mesh_torch(p, v, faces, w_pf=1.0, w_fp=1.0):
    """The same definition as a float64 torch expression for autograd: p [B, N, 3], v [B, V, 3] float64 tensors (requires_grad as the caller
    wishes), faces [F, 3] integer tensor -> the 0-d value.  The whole [B, N, F] matrix at once: small cases and timing only.  Autograd
    differentiates the closest point too; by the envelope property that adds nothing away from the region boundaries."""
    import torch
    f = faces.long().clamp(0, v.shape[1] - 1)
    a = v[:, f[:, 0]]
    ab, ac = v[:, f[:, 1]] - a, v[:, f[:, 2]] - a
    ap = p[:, :, None, :] - a[:, None]
    _, _, _, d2, _ = closest(ap, ab[:, None], ac[:, None], _dot(ab, ab)[:, None], _dot(ab, ac)[:, None], _dot(ac, ac)[:, None], xp=torch)
    N, F = p.shape[1], f.shape[0]
    value = 0.0
    if w_pf != 0.0:
        value = value + float(np.float32(w_pf)) * (d2.min(2).values.sum(1) / N).mean()
    if w_fp != 0.0:
        value = value + float(np.float32(w_fp)) * (d2.min(1).values.sum(1) / F).mean()
    return value
