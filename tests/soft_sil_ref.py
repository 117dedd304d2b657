"""A torch restatement of the soft silhouette (include/hifihr.h, "Soft silhouette") and of its two losses: brute force over every
pixel x face, gradients by autograd.  In float64 it is the reference of tests/soft_sil_cases.py; evaluated in float32 (`dtype`) it is the
yardstick the bounds there were sized by.  Test infrastructure only: not an oracle of PyTorch3D (whose semantics it restates from memory,
like the kernel), not a fallback."""
import math

import torch

RASTER_EPS = 1e-8


def default_blur(sigma):
    return math.log(1.0 / 1e-4 - 1.0) * sigma


def pix_to_ndc(i, S):
    return -1.0 + (2.0 * i + 1.0) / S


def _edge_fn(px, py, a, b):
    return (px - a[..., 0]) * (b[..., 1] - a[..., 1]) - (py - a[..., 1]) * (b[..., 0] - a[..., 0])


def _seg_dist2(px, py, a, b):
    ex, ey = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    t = (((px - a[..., 0]) * ex + (py - a[..., 1]) * ey) / (ex * ex + ey * ey)).clamp(0.0, 1.0)
    qx, qy = a[..., 0] + t * ex - px, a[..., 1] + t * ey - py
    return qx * qx + qy * qy


def _softplus(x):
    return x.clamp(min=0.0) + torch.log1p(torch.exp(-x.abs()))


def _window(ndc, faces, H, blur):
    """(y0, y1, x0, x1): a pixel window outside of which no face of `faces` can participate in any image of ndc [B,V,2] -- their common
    bounding box grown by sqrt(blur) and two pixels, in pixel indices (pixel i samples pix_to_ndc(H - 1 - i)); the whole image when the
    box is not finite."""
    v = ndc[:, faces.reshape(-1)].detach()
    lo, hi = v.amin((0, 1)), v.amax((0, 1))
    if not (bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all())):
        return 0, H, 0, H
    grow = math.sqrt(blur) + 4.0 / H
    win = []
    for k in (1, 0):                                             # rows from y, columns from x
        first = H - 1 - ((float(hi[k]) + grow + 1.0) * H / 2.0 - 0.5)
        last = H - 1 - ((float(lo[k]) - grow + 1.0) * H / 2.0 - 0.5)
        win += [min(max(int(math.floor(first)), 0), H), min(max(int(math.ceil(last)) + 1, 0), H)]
    return tuple(win)


def _chunk_terms(ndc, z, faces, H, sigma, blur, win=None):
    """ndc [B,V,2], z [B,V], faces [f,3] -> (softplus terms [B,f,h,w] with 0 where the face does not participate, dist, inside, valid,
    participates) on the pixel window win = (y0, y1, x0, x1) (default: the whole image)."""
    dt, dev = ndc.dtype, ndc.device
    v = [ndc[:, faces[:, k]].unsqueeze(2).unsqueeze(2) for k in range(3)]                  # [B,f,1,1,2]
    zf = torch.stack([z[:, faces[:, k]] for k in range(3)], -1)                            # [B,f,3]
    idx = torch.arange(H, device=dev, dtype=dt)
    c = pix_to_ndc(H - 1 - idx, H)
    y0, y1, x0, x1 = win if win is not None else (0, H, 0, H)
    px, py = c[x0:x1].view(1, 1, 1, -1), c[y0:y1].view(1, 1, -1, 1)                        # [.., yi, xi]
    area = _edge_fn(v[2][..., 0], v[2][..., 1], v[0], v[1])
    w = [_edge_fn(px, py, v[1], v[2]) / area, _edge_fn(px, py, v[2], v[0]) / area, _edge_fn(px, py, v[0], v[1]) / area]
    inside = (w[0] > 0) & (w[1] > 0) & (w[2] > 0)
    dist = torch.stack([_seg_dist2(px, py, v[0], v[1]), _seg_dist2(px, py, v[1], v[2]), _seg_dist2(px, py, v[2], v[0])], 0).min(0).values
    valid = ((zf > 0).all(-1).view(*zf.shape[:2], 1, 1)) & (area.abs() > RASTER_EPS)
    part = valid & (inside | (dist < blur))
    d = torch.where(inside, -dist, dist)
    return torch.where(part, _softplus(-d / sigma), torch.zeros((), dtype=dt, device=dev)), dist, inside, valid, part


GAP = 5e-5      # a (pixel, face) pair that is not inside and has |dist - blur| < GAP * blur is "near": fp32 and fp64 may disagree on it


def soft_silhouette(verts, faces, cam, H, sigma, blur, w=None, dtype=torch.float64, device="cpu", chunk=128, w_skips_near=False, windowed=False):
    """verts [B,V,3], faces [F,3], cam [B,4] (any float dtype: taken as they are, converted to `dtype`) ->
    {"alpha" [B,H,H], "S" [B,H,H], "gap": min |dist - blur| / blur over the pairs that are not inside (inf without one),
     "near" [B,H,H]: how many near pairs (GAP) a pixel has, "faces_hit" [B]: the faces that participate in at least one pixel,
     "gverts": d sum(alpha * w) / d verts when w [B,H,H] is given (w_skips_near: w is first zeroed at the pixels that have a near pair;
     "w" is the w used)}.  Faces are walked `chunk` at a time to bound the memory; the gradient is
    taken per chunk with the upstream d alpha / d S = exp(-S) of the finished sum.  windowed: image by image, every chunk is evaluated only on
    the pixel window its faces can reach (_window) -- the same brute force on the pairs that can be non-zero, for the large cases; "gap" is
    then the minimum over those windows."""
    if windowed and verts.shape[0] > 1:
        outs = [soft_silhouette(verts[b:b + 1], faces, cam[b:b + 1], H, sigma, blur, None if w is None else w[b:b + 1], dtype, device, chunk,
                                w_skips_near, True) for b in range(verts.shape[0])]
        cat = {k: torch.cat([o[k] for o in outs]) for k in outs[0] if torch.is_tensor(outs[0][k])}
        cat["gap"] = min(o["gap"] for o in outs)
        return cat
    verts, cam = verts.detach().to(device=device, dtype=dtype), cam.detach().to(device=device, dtype=dtype)
    faces = torch.as_tensor(faces).long().to(device)
    B = verts.shape[0]

    def project(vv):
        X, Y, Z = vv[..., 0], vv[..., 1], vv[..., 2]
        fx, fy, px, py = (cam[:, k].unsqueeze(1) for k in range(4))
        return torch.stack([(X * fx + Z * px) / Z, (Y * fy + Z * py) / Z], -1), Z

    S = torch.zeros(B, H, H, dtype=dtype, device=device)
    gap = float("inf")
    near = torch.zeros(B, H, H, dtype=torch.int32, device=device)
    hit = torch.zeros(B, dtype=torch.int64, device=device)
    with torch.no_grad():
        ndc, z = project(verts)
        for f0 in range(0, faces.shape[0], chunk):
            y0, y1, x0, x1 = win = _window(ndc, faces[f0:f0 + chunk], H, blur) if windowed else (0, H, 0, H)
            if y1 <= y0 or x1 <= x0:
                continue
            terms, dist, inside, valid, part = _chunk_terms(ndc, z, faces[f0:f0 + chunk], H, sigma, blur, win)
            S[:, y0:y1, x0:x1] += terms.sum(1)
            hit += part.flatten(2).any(-1).sum(1)
            sel = valid & ~inside
            if blur > 0 and bool(sel.any()):
                rel = (dist - blur).abs() / blur
                gap = min(gap, float(rel[sel].min()))
                near[:, y0:y1, x0:x1] += (sel & (rel < GAP)).sum(1).to(torch.int32)
    out = {"alpha": 1.0 - torch.exp(-S), "S": S, "gap": gap, "near": near, "faces_hit": hit}
    if w is not None:
        w = w.to(device=device, dtype=dtype)
        if w_skips_near:
            w = torch.where(near > 0, torch.zeros((), dtype=dtype, device=device), w)
        out["w"] = w
        up = w * torch.exp(-S)                                                               # d loss / d S
        vg = verts.clone().requires_grad_(True)
        for f0 in range(0, faces.shape[0], chunk):
            ndc, z = project(vg)
            y0, y1, x0, x1 = win = _window(ndc, faces[f0:f0 + chunk], H, blur) if windowed else (0, H, 0, H)
            if y1 <= y0 or x1 <= x0:
                continue
            terms = _chunk_terms(ndc, z, faces[f0:f0 + chunk], H, sigma, blur, win)[0]
            (terms.sum(1) * up[:, y0:y1, x0:x1]).sum().backward()
        out["gverts"] = vg.grad if vg.grad is not None else torch.zeros_like(verts)
    return out


def losses(alpha, mask, lam_sil, lam_iou):
    """(lam_sil * F.l1_loss(alpha, mask), lam_iou * hifihr_amd.losses.iou(mask, alpha)) in float64; alpha may require grad."""
    A, M = alpha.double().flatten(1), mask.double().flatten(1)
    inter = (A * M).sum(1)
    union = (A + M).sum(1) - inter
    return torch.stack([lam_sil * (A - M).abs().mean(), lam_iou * (1.0 - (inter / union).mean())])
