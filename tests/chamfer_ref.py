"""The float64 numpy restatement of the Chamfer distance as include/hifihr.h defines it ("Chamfer distance"; csrc/chamfer.hip), the
reference of tests/chamfer_cases.py.

The same expression in the same order as the kernel -- d2 = (dx dx + dy dy) + dz dz on the float32 inputs widened to float64, numpy
evaluates each operation by itself (no contraction) --, so d2, the arg-min (np.argmin returns the FIRST occurrence: ties to the lowest
index) and the minima are the kernel's integers and bits.  The gradient takes the arg-min as a constant and sums in ascending index order
(np.add.at is unbuffered and walks its index array in order)."""
import numpy as np


def d2_matrix(x, y):
    """x [N, 3], y [M, 3] float32 -> float64 [N, M]"""
    xd, yd = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    dx, dy, dz = (xd[:, None, k] - yd[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def chamfer(x, y, w_xy=1.0, w_yx=1.0, gout=1.0):
    """x [B, N, 3], y [B, M, 3] (float32 values).  -> dict: idx_xy [B, N] / idx_yx [B, M] int32, min_xy / min_yx float64, sums [B, 2],
    value (float64, before the one rounding to float32), gx [B, N, 3] / gy [B, M, 3] float64 for the gradient `gout` of the value.  The
    weights and gout are taken as the float32 values the kernel receives."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    w_xy, w_yx, gout = float(np.float32(w_xy)), float(np.float32(w_yx)), float(np.float32(gout))
    idx_xy, idx_yx = np.zeros((B, N), np.int32), np.zeros((B, M), np.int32)
    min_xy, min_yx = np.zeros((B, N), np.float64), np.zeros((B, M), np.float64)
    gx, gy = np.zeros((B, N, 3), np.float64), np.zeros((B, M, 3), np.float64)
    c_xy, c_yx = w_xy * 2.0 / (B * N), w_yx * 2.0 / (B * M)
    for b in range(B):
        d2 = d2_matrix(x[b], y[b])
        a, c = d2.argmin(1), d2.argmin(0)
        idx_xy[b], idx_yx[b] = a, c
        min_xy[b], min_yx[b] = d2[np.arange(N), a], d2[c, np.arange(M)]
        xd, yd = x[b].astype(np.float64), y[b].astype(np.float64)
        sx, sy = np.zeros((N, 3)), np.zeros((M, 3))
        np.add.at(sx, c, xd[c] - yd)                     # sum over { j : c[j] == i } of (x[i] - y[j]), ascending j
        np.add.at(sy, a, yd[a] - xd)                     # sum over { i : a[i] == j } of (y[j] - x[i]), ascending i
        zx = np.zeros((N, 3)) if w_xy == 0.0 else c_xy * (xd - yd[a])
        zy = np.zeros((M, 3)) if w_yx == 0.0 else c_yx * (yd - xd[c])
        gx[b] = gout * (zx + (np.zeros((N, 3)) if w_yx == 0.0 else c_yx * sx))
        gy[b] = gout * (zy + (np.zeros((M, 3)) if w_xy == 0.0 else c_xy * sy))
    sums = np.stack([min_xy.sum(1), min_yx.sum(1)], 1)
    value = (w_xy * np.mean(sums[:, 0] / N) if w_xy != 0.0 else 0.0) + (w_yx * np.mean(sums[:, 1] / M) if w_yx != 0.0 else 0.0)
    return dict(idx_xy=idx_xy, idx_yx=idx_yx, min_xy=min_xy, min_yx=min_yx, sums=sums, value=float(value), gx=gx, gy=gy)
