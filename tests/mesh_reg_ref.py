"""Restatement of the two mesh regularisers (include/hifihr.h "Mesh regularisers": `triangle` = the uniform Laplacian of PyTorch3D's
mesh_laplacian_smoothing, `normal_consistency` = its mesh_normal_consistency, both [recalled]) in plain torch: an index-add Laplacian,
torch.cross and F.cosine_similarity(eps=1e-8); the gradients come from autograd.  float64 is the reference of the tests, the same code
in float32 is their yardstick.  The topology is counted here in Python, independently of the library's host code."""
import numpy as np
import torch
import torch.nn.functional as F


def topology(faces, V):
    """faces [F, 3] -> dict(edges [E, 2], quads [Q, 4], deg [V]) as int64 numpy arrays, by the rules of the header: unique unordered
    pairs; per edge (v0 < v1) the opposite vertices in ascending face order, one record (v0, v1, a, b) per unordered pair of them."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    opposite = {}
    for f in faces:                                                  # ascending face order
        assert len(set(f.tolist())) == 3 and f.min() >= 0 and f.max() < V, f
        for k in range(3):
            i, j, o = int(f[k]), int(f[(k + 1) % 3]), int(f[(k + 2) % 3])
            opposite.setdefault((min(i, j), max(i, j)), []).append(o)
    edges = sorted(opposite)
    quads = [(v0, v1, opp[i], opp[j]) for (v0, v1) in edges for opp in [opposite[(v0, v1)]] for i in range(len(opp)) for j in range(i + 1, len(opp))]
    deg = np.zeros(V, dtype=np.int64)
    for v0, v1 in edges:
        deg[v0] += 1
        deg[v1] += 1
    return dict(edges=np.asarray(edges, dtype=np.int64).reshape(-1, 2), quads=np.asarray(quads, dtype=np.int64).reshape(-1, 4), deg=deg,
                boundary=sum(1 for e in edges if len(opposite[e]) == 1))


def laplacian_d(verts, topo):
    """d_i = mean of the neighbours - v_i ([B, V, 3]); a vertex without a neighbour has d = -v."""
    e = torch.as_tensor(topo["edges"])
    s = torch.zeros_like(verts).index_add(1, e[:, 0], verts[:, e[:, 1]]).index_add(1, e[:, 1], verts[:, e[:, 0]])
    deg = torch.as_tensor(topo["deg"]).to(verts.dtype).clamp(min=1.0)
    return s / deg[None, :, None] - verts


def terms(verts, topo):
    """-> (lap, nc) unweighted, 0-d tensors of verts' dtype."""
    lap = torch.norm(laplacian_d(verts, topo), dim=-1).mean()        # torch.norm: the subgradient at 0 is 0
    q = torch.as_tensor(topo["quads"])
    if q.shape[0] == 0:
        return lap, torch.zeros((), dtype=verts.dtype)
    v0, v1, a, b = (verts[:, q[:, k]] for k in range(4))
    e = v1 - v0
    n0 = torch.cross(e, a - v0, dim=-1)
    n1 = -torch.cross(e, b - v0, dim=-1)
    return lap, (1.0 - F.cosine_similarity(n0, n1, dim=-1, eps=1e-8)).mean()


def mesh_regularizers(verts, faces, lam_lap, lam_nc, gout=None, dtype=torch.float64, topo=None):
    """verts [B, V, 3] (their float32 values are what every precision sees) -> dict(out [2], unit [B, V, 3], gverts or None); a weight of
    exactly 0 gives that term as 0 without a gradient.  lam_* are rounded to float32 first, as the C ABI takes them."""
    topo = topology(faces, verts.shape[1]) if topo is None else topo
    v = verts.detach().float().to(dtype).requires_grad_(True)
    lap, nc = terms(v, topo)
    lam = [float(np.float32(lam_lap)), float(np.float32(lam_nc))]
    out = torch.stack([lam[0] * lap if lam[0] != 0.0 else torch.zeros((), dtype=dtype), lam[1] * nc if lam[1] != 0.0 else torch.zeros((), dtype=dtype)])
    res = dict(out=out.detach(), gverts=None, topo=topo)
    with torch.no_grad():
        d = laplacian_d(v.detach(), topo)
        n = torch.norm(d, dim=-1, keepdim=True)
        res["unit"] = torch.where(n > 0, d / n.clamp(min=torch.finfo(dtype).tiny), torch.zeros_like(d)) if lam[0] != 0.0 else torch.zeros_like(d)
    if gout is not None:
        g = torch.as_tensor(gout).to(dtype)
        if out.requires_grad:
            (out * g).sum().backward()
            res["gverts"] = v.grad.detach()
        else:
            res["gverts"] = torch.zeros_like(v.detach())
    return res
