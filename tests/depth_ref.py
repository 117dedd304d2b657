"""Restatements of the depth map and the depth loss (include/hifihr.h "Depth map"; csrc/depth.hip), independent of the kernels:

  depth_f32        the forward in float32 NumPy, one rounding per operation in the expression order of oracle/raster_oracle.c (NumPy's
                   float32 ufuncs round after every operation and fuse nothing, like the -ffp-contract=off builds): the bit-for-bit target;
  depth_torch      the forward in torch at a chosen dtype (float64: the reference of the gradient through autograd; float32: the yardstick
                   of the gradient's bound), with face_id and hits as constants;
  loss_sums_ordered / loss_value / loss_grad    the loss in float64, the sums in the kernel's stated order.
Test infrastructure only."""
import numpy as np
import torch

EPS = np.float32(1e-8)
THREADS = 256          # kDepthThreads of csrc/depth.hip: the loss sums are taken by 256 lanes with stride 256, then folded (see below)


def project_f32(verts, cam):
    """(X fx + Z px) / Z, (Y fy + Z py) / Z, Z in float32: the projection of oracle/render_oracle.project_ndc.  verts [B,V,3], cam [B,4]."""
    v, c = np.asarray(verts, dtype=np.float32), np.asarray(cam, dtype=np.float32)
    X, Y, Z = v[..., 0], v[..., 1], v[..., 2]
    fx, fy, px, py = (c[:, k][:, None] for k in range(4))
    return np.stack([(X * fx + Z * px) / Z, (Y * fy + Z * py) / Z, Z], axis=-1).astype(np.float32)


def _centres_f32(S):
    i = (S - 1 - np.arange(S)).astype(np.float32)
    return (np.float32(-1.0) + (np.float32(2.0) * i + np.float32(1.0)) / np.float32(S)).astype(np.float32)      # pix_to_ndc(S - 1 - index, S)


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def sample_pz_f32(ndc, faces, face_id):
    """pz of every sample for the face face_id names (garbage where face_id < 0), and whether the denominator clamp is active there.
    ndc float32 [B,V,3]; faces [F,3]; face_id int32 [B,S,S].  -> (pz float32 [B,S,S], clamped bool [B,S,S])."""
    B, S = face_id.shape[0], face_id.shape[1]
    faces = np.asarray(faces).astype(np.int64)
    f = np.clip(face_id, 0, None).astype(np.int64)
    bi = np.arange(B)[:, None, None]
    v = [ndc[bi, faces[f, k]] for k in range(3)]                         # [B,S,S,3] each
    x0, y0, z0 = v[0][..., 0], v[0][..., 1], v[0][..., 2]
    x1, y1, z1 = v[1][..., 0], v[1][..., 1], v[1][..., 2]
    x2, y2, z2 = v[2][..., 0], v[2][..., 1], v[2][..., 2]
    c = _centres_f32(S)
    xf, yf = np.broadcast_to(c[None, None, :], f.shape), np.broadcast_to(c[None, :, None], f.shape)
    with np.errstate(all="ignore"):
        area = _edge(x2, y2, x0, y0, x1, y1) + EPS
        w0 = _edge(xf, yf, x1, y1, x2, y2) / area
        w1 = _edge(xf, yf, x2, y2, x0, y0) / area
        w2 = _edge(xf, yf, x0, y0, x1, y1) / area
        t0 = w0 * z1 * z2
        t1 = z0 * w1 * z2
        t2 = z0 * z1 * w2
        tsum = t0 + t1 + t2
        denom = np.maximum(tsum, EPS)
        b0, b1, b2 = t0 / denom, t1 / denom, t2 / denom
        pz = b0 * z0 + b1 * z1 + b2 * z2
    assert pz.dtype == np.float32
    return pz, ~(tsum > EPS)


def depth_f32(verts, cam, faces, face_id, H, aa):
    """-> (depth float32 [B,H,H], hits int32 [B,H,H], clamped samples among the covered ones): the sum over the covered samples in row-major
    sample order, one division by hits, 0 where hits == 0."""
    face_id = np.asarray(face_id)
    B, S = face_id.shape[0], H * aa
    assert face_id.shape == (B, S, S)
    pz, clamped = sample_pz_f32(project_f32(verts, cam), faces, face_id)
    cov = face_id >= 0
    pzr, covr = pz.reshape(B, H, aa, H, aa), cov.reshape(B, H, aa, H, aa)
    total, hits = np.zeros((B, H, H), np.float32), np.zeros((B, H, H), np.int32)
    for i in range(aa):
        for j in range(aa):
            c = covr[:, :, i, :, j]
            total = np.where(c, total + pzr[:, :, i, :, j], total).astype(np.float32)
            hits += c
    with np.errstate(all="ignore"):
        depth = np.where(hits > 0, total / hits.astype(np.float32), np.float32(0.0)).astype(np.float32)
    return depth, hits, int((clamped & cov).sum())


def depth_torch(verts, cam, faces, face_id, hits, H, aa, dtype=torch.float64):
    """The same definition in torch at `dtype`, differentiable in verts; face_id [B,S,S] and hits [B,H,H] are constants; the denominator
    clamp is torch.clamp (no gradient where it is active).  -> depth [B,H,H]."""
    B, S, dev = verts.shape[0], H * aa, verts.device
    cam = cam.to(device=dev, dtype=dtype)
    X, Y, Z = verts[..., 0], verts[..., 1], verts[..., 2]
    fx, fy, px, py = (cam[:, k].unsqueeze(1) for k in range(4))
    ndc = torch.stack([(X * fx + Z * px) / Z, (Y * fy + Z * py) / Z, Z], dim=-1)
    face_id = torch.as_tensor(face_id).to(dev).long()
    faces = torch.as_tensor(faces).to(dev).long()
    cov = face_id >= 0
    f = face_id.clamp(min=0)
    bi = torch.arange(B, device=dev).view(B, 1, 1)
    v = [ndc[bi, faces[f, k]] for k in range(3)]
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = (t.unbind(-1) for t in v)
    i = torch.arange(S, dtype=dtype, device=dev)
    c = -1.0 + (2.0 * (S - 1 - i) + 1.0) / S
    xf, yf = c.view(1, 1, S), c.view(1, S, 1)
    area = _edge(x2, y2, x0, y0, x1, y1) + 1e-8
    w0 = _edge(xf, yf, x1, y1, x2, y2) / area
    w1 = _edge(xf, yf, x2, y2, x0, y0) / area
    w2 = _edge(xf, yf, x0, y0, x1, y1) / area
    t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
    denom = (t0 + t1 + t2).clamp(min=1e-8)
    pz = (t0 / denom) * z0 + (t1 / denom) * z1 + (t2 / denom) * z2
    pz = torch.where(cov, pz, torch.zeros((), dtype=dtype, device=dev))
    total = pz.view(B, H, aa, H, aa).sum(dim=(2, 4))
    hits = torch.as_tensor(hits).to(dev)
    return torch.where(hits > 0, total / hits.clamp(min=1).to(dtype), torch.zeros((), dtype=dtype, device=dev))


# ---- loss ---------------------------------------------------------------------------------------------------------------------------
def loss_valid(d, hits, D, mask, trunc):
    """[B,HW] bool, and d - D in float64 (exact for float32 inputs)."""
    d64, D64 = np.asarray(d, np.float32).astype(np.float64), np.asarray(D, np.float32).astype(np.float64)
    e = d64 - D64
    ok = (np.asarray(hits) > 0) & (np.asarray(D, np.float32) > 0)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    t = float(np.float32(trunc))
    if t != 0.0:
        ok &= np.abs(e) <= t
    return ok, e


def loss_sums_ordered(d, hits, D, mask, trunc):
    """sums [B,2] float64 in the kernel's order: lane t of 256 adds its pixels t, t + 256, ... in turn; each wave of 64 lanes folds by halves
    (lane l += lane l + 32, then 16, 8, 4, 2, 1); the four waves are added as ((w0 + w1) + w2) + w3."""
    ok, e = loss_valid(d, hits, D, mask, trunc)
    B, HW = ok.shape
    out = np.zeros((B, 2), np.float64)
    for k, val in enumerate((np.where(ok, np.abs(e), 0.0), ok.astype(np.float64))):
        n = -(-HW // THREADS) * THREADS
        pad = np.zeros((B, n), np.float64)
        pad[:, :HW] = val
        rows = pad.reshape(B, n // THREADS, THREADS)
        lanes = np.zeros((B, THREADS), np.float64)
        for r in range(rows.shape[1]):
            lanes = lanes + rows[:, r]
        w = lanes.reshape(B, 4, 64).copy()
        o = 32
        while o > 0:
            shifted = np.zeros_like(w)
            shifted[:, :, :64 - o] = w[:, :, o:]          # a lane past the end reads itself in hardware; only lane 0's chain matters
            w = w + shifted
            o //= 2
        out[:, k] = ((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]
    return out


def loss_value(sums, lam):
    """out as the finish step forms it: float32(lam * (sum_b sum) / max(sum_b count, 1)), image by image."""
    s = n = 0.0
    for b in range(sums.shape[0]):
        s += float(sums[b, 0])
        n += float(sums[b, 1])
    return np.float32(float(np.float32(lam)) * (s / max(n, 1.0)))


def loss_grad(d, hits, D, mask, trunc, sums, gout, lam):
    """gdepth by formula: float32(gout lam / max(count, 1)) times sign(d - D) on the valid pixels, 0 elsewhere."""
    ok, e = loss_valid(d, hits, D, mask, trunc)
    n = 0.0
    for b in range(sums.shape[0]):
        n += float(sums[b, 1])
    scale = np.float32(float(np.float32(gout)) * float(np.float32(lam)) / max(n, 1.0))
    return np.where(ok, np.sign(e).astype(np.float32) * scale, np.float32(0.0)).astype(np.float32)
