"""Shared bodies of the point-to-mesh tests (hifihr_point_mesh_fwd / _bwd, csrc/point_mesh.hip): tests/test_hostsim_point_mesh.py runs them on
the emulator (device='cpu'), tests/test_gpu_point_mesh.py on the MI355X (device='cuda').  The reference is the float64 restatement of
tests/point_mesh_ref.py.  Parity with PyTorch3D's point_mesh_face_distance is unpinned.

Bounds (include/hifihr.h "Point-to-mesh distance"; the kernels and the restatement evaluate ONE fp64 expression without contraction):
    idx_*, min_*, bary_*   on the emulator: equal as integers / as float64 bits.  On the GPU the same equality is expected and the number of
             differing elements is printed; fp64 division is the one operation whose device rounding this repository had not pinned, so a
             differing element is EXCUSED only where the restatement's own d2 at the kernel's choice lies within DELTA = 1e-12 extent^2 of
             the restatement's minimum (extent: the largest coordinate span of the case; fp64 epsilon 2.2e-16 times an expression depth of a
             few tens, with two orders of margin).  An excused element compares the CLOSEST POINT instead of the weights: the kernel's
             weights are >= 0 and sum to 1 within 1e-15, and the point they give on the kernel's face has, in float64 on the host, a squared
             distance within DELTA of the restatement's minimum, as has the kernel's min.  (Two faces tied at a distance need not share a
             closest point, so the points themselves are not compared.)  The exact-arithmetic cases (known answers, ties) admit no excuse.
             Every soup case first asserts on the restatement alone that no query's best and second-best d2 are closer than DELTA, so there
             the excuse cannot fire: it can only fire on the shared edges and vertices of the MANO-topology case.
    sums_d   within 1e-12 relative: an fp64 sum of a few thousand non-negative terms in any order stays inside that
    out_d    within 2^-23 |ref|: one fp32 rounding of an fp64 value
    gp, gv   every component within 2^-23 |ref| + 1e-10 max |ref over the tensor|: accumulated in fp64, rounded once
(Qp, Tf) = points per workgroup and face records per LDS pass of the points -> faces search, (Qf, Tp) = faces per workgroup and points per
LDS pass of the faces -> points search, from hifihr_point_mesh_geometry; the four waves of a workgroup scan consecutive quarters of a pass.
The cases are built from them."""
import ctypes

import numpy as np
import torch

import kernel_cases as kc
import point_mesh_ref as pr

EINVAL = -1
W = (0.7, 1.3)                     # unequal weights: a mix-up of the two directions shows
GOUT = -1.7
KERNELS = {"point_mesh_search_kernel", "point_mesh_finish_kernel", "point_mesh_bwd_points_kernel", "point_mesh_bwd_corners_kernel",
           "point_mesh_bwd_verts_kernel"}
EPS32 = 2.0 ** -23
_PAD = 64                          # guard elements on each side of every output
_CANARY = {torch.int32: -7, torch.float64: -1234.5, torch.float32: -1234.5}
_FILL = {torch.int32: -1, torch.float64: float("nan"), torch.float32: float("nan")}
_DIR_KEYS = {0: ("idx_pf", "bary_pf", "min_pf"), 1: ("idx_fp", "bary_fp", "min_fp")}


def geometry(lib):
    qp, tf, qf, tp = lib.point_mesh_geometry()
    assert qp >= 64 and qp % 64 == 0 and qf >= 64 and qf % 64 == 0 and tf >= 4 and tf % 4 == 0 and tp >= 4 and tp % 4 == 0, (qp, tf, qf, tp)
    return qp, tf, qf, tp


def boundary_sizes(lib, direction):
    """-> (the five N, the five F) round the boundaries of one direction: queries {1, Q-1, Q, Q+1, 2Q+3}, searched {1, T-1, T, T+1, 2T+5}"""
    qp, tf, qf, tp = geometry(lib)
    five = lambda q, t: ([1, q - 1, q, q + 1, 2 * q + 3], [1, t - 1, t, t + 1, 2 * t + 5])
    if direction == 0:
        return five(qp, tf)
    fs, ns = five(qf, tp)
    return ns, fs


def seeded_soup(B, N, V, F, seed):
    """A triangle soup in general position: seeded vertices and points uniform in a 20 cm box (float32, metres), seeded faces with three
    distinct indices.  No two faces share a vertex (V >= 3 F): a point whose closest point is a shared vertex would be an exact tie between
    the faces round it, and the soups are the cases that must have none (assert_general_position)."""
    assert V >= 3 * F
    g = torch.Generator().manual_seed(seed)
    p = ((torch.rand(B, N, 3, generator=g) - 0.5) * 0.2).numpy()
    v = ((torch.rand(B, V, 3, generator=g) - 0.5) * 0.2).numpy()
    faces = torch.randperm(V, generator=g)[:3 * F].reshape(F, 3).numpy().astype(np.int32)
    return p, v, faces


def soup_verts(F):
    """The vertex count of the soups: three per face and two that no face uses (their gradient is 0)"""
    return 3 * F + 2


class _Outs:
    """Outputs inside larger allocations: _PAD canary elements on each side, which must come back unchanged."""

    def __init__(self, device):
        self.device, self.items = device, []

    def new(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        whole = torch.full((_PAD + n + _PAD,), _CANARY[dtype], dtype=dtype, device=self.device)
        view = whole[_PAD:_PAD + n].view(*shape)
        view.fill_(_FILL[dtype] if fill is None else fill)
        self.items.append((whole, n, _CANARY[dtype]))
        return view

    def intact(self):
        for whole, n, canary in self.items:
            assert bool((whole[:_PAD] == canary).all()) and bool((whole[_PAD + n:] == canary).all()), "wrote outside an output (guard band changed)"


def _bits(t):
    return t.view(torch.int64) if t.element_size() == 8 else t.view(torch.int32)


def _untouched(t):
    return bool((t == -1).all()) if t.dtype == torch.int32 else bool(torch.isnan(t).all())


def device_tables(faces, V, device):
    off, corner = pr.vertex_corner_table(faces, V)
    return torch.as_tensor(off).to(device), torch.as_tensor(corner).to(device)


def run_kernels(lib, device, p, v, faces, w_pf, w_fp, gout=GOUT, grads="both"):
    """-> dict of CPU numpy arrays (idx_pf, bary_pf, min_pf, idx_fp, bary_fp, min_fp, sums, out, gp, gv).  Every output starts as a value
    the kernels cannot produce (index -1, NaN), inside guard bands, and must come back fully written with the bands untouched -- except the
    arrays of a direction of weight exactly 0, which must come back UNTOUCHED; forward and backward run twice: the same bits both times.
    grads: "both", "p" (gv_d NULL) or "v" (gp_d NULL)."""
    p = torch.as_tensor(np.asarray(p, np.float32)).to(device).contiguous()
    v = torch.as_tensor(np.asarray(v, np.float32)).to(device).contiguous()
    faces_t = torch.as_tensor(np.asarray(faces, np.int32)).to(device).contiguous()
    B, N, V, F = p.shape[0], p.shape[1], v.shape[1], faces_t.shape[0]
    off, corner = device_tables(faces, V, device)
    go = torch.tensor([gout], dtype=torch.float32, device=device)
    o = _Outs(device)
    runs = []
    for _ in range(2):
        r = dict(idx_pf=o.new((B, N), torch.int32), bary_pf=o.new((B, N, 3), torch.float64), min_pf=o.new((B, N), torch.float64),
                 idx_fp=o.new((B, F), torch.int32), bary_fp=o.new((B, F, 3), torch.float64), min_fp=o.new((B, F), torch.float64),
                 sums=o.new((B, 2), torch.float64), out=o.new((1,), torch.float32))
        ws = o.new((lib.point_mesh_workspace_bytes(B, N, V, F) // 8,), torch.float64)
        r["gp"] = o.new((B, N, 3), torch.float32) if grads in ("both", "p") else None
        r["gv"] = o.new((B, V, 3), torch.float32) if grads in ("both", "v") else None
        lib.point_mesh_fwd(p, v, faces_t, w_pf, w_fp, r["idx_pf"], r["bary_pf"], r["min_pf"], r["idx_fp"], r["bary_fp"], r["min_fp"], r["sums"],
                           r["out"], ws)
        lib.point_mesh_bwd(p, v, faces_t, r["idx_pf"], r["bary_pf"], r["idx_fp"], r["bary_fp"], go, off, corner, w_pf, w_fp, r["gp"], r["gv"], ws)
        runs.append(r)
    skipped = set(_DIR_KEYS[0] if float(np.float32(w_pf)) == 0.0 else ()) | set(_DIR_KEYS[1] if float(np.float32(w_fp)) == 0.0 else ())
    for k, a in runs[0].items():
        if a is None:
            continue
        if k in skipped:
            assert _untouched(a) and _untouched(runs[1][k]), f"{k}: a direction of weight 0 was written"
            continue
        if a.dtype == torch.int32:
            assert int(a.min()) >= 0, f"{k}: an element was not written"
        else:
            assert not bool(torch.isnan(a).any()), f"{k}: an element was not written"
        assert torch.equal(_bits(a), _bits(runs[1][k])), f"{k}: two calls differ in their bits"
    o.intact()
    res = {k: (None if a is None else a.cpu().numpy()) for k, a in runs[0].items()}
    res["skipped"] = skipped
    return res


def extent_of(p, v):
    both = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3), np.asarray(v, np.float64).reshape(-1, 3)])
    return float((both.max(0) - both.min(0)).max())


def _compare_direction(tag, d, got, ref, p, v, faces, device, exact, delta):
    ki, kb, km = _DIR_KEYS[d]
    differ = (got[ki] != ref[ki]) | (got[km].view(np.int64) != ref[km].view(np.int64)) | (got[kb].view(np.int64) != ref[kb].view(np.int64)).any(-1)
    n_idx, n_min = int((got[ki] != ref[ki]).sum()), int((got[km].view(np.int64) != ref[km].view(np.int64)).sum())
    n_bary = int((got[kb].view(np.int64) != ref[kb].view(np.int64)).any(-1).sum())
    print(f"[point_mesh] {tag}: {ki}: {n_idx} of {got[ki].size} indices differ; {km}: {n_min} minima and {kb}: {n_bary} weight triples differ "
          f"in their bits")
    if device == "cpu" or exact:
        assert not differ.any(), (tag, ki, np.argwhere(differ)[:4].tolist())
        return
    fc = np.clip(np.asarray(faces, np.int64), 0, np.asarray(v).shape[1] - 1)
    for b, q in np.argwhere(differ):
        k = int(got[ki][b, q])
        pi, fi = ([q], [k]) if d == 0 else ([k], [q])
        d2k, _ = pr.d2_at(p[b], v[b], faces, pi, fi)
        w = got[kb][b, q]
        vd, pd = np.asarray(v[b], np.float32).astype(np.float64), np.asarray(p[b], np.float32).astype(np.float64)
        cp = (vd[fc[fi[0]]] * w[:, None]).sum(0)
        dk = float(((pd[pi[0]] - cp) ** 2).sum())
        print(f"[point_mesh] {tag}: {ki}[{b}, {q}] = {k} (restatement {int(ref[ki][b, q])}): restatement d2 there {float(d2k[0]):.17e}, minimum "
              f"{float(ref[km][b, q]):.17e}, kernel min {float(got[km][b, q]):.17e}, d2 of the kernel's closest point {dk:.17e}, DELTA {delta:.3e}")
        assert float(d2k[0]) - float(ref[km][b, q]) <= delta, (tag, ki, int(b), int(q), "differs and is no tie within DELTA")
        assert (w >= 0).all() and abs(float(w.sum()) - 1.0) <= 1e-15, (tag, kb, w.tolist())
        assert abs(dk - float(ref[km][b, q])) <= delta + 1e-15 * float(ref[km][b, q]) and abs(float(got[km][b, q]) - float(ref[km][b, q])) <= delta


def compare(tag, got, ref, p, v, faces, device, exact=False):
    """The module docstring's bounds; prints each figure before it asserts."""
    delta = 1e-12 * extent_of(p, v) ** 2
    for d in (0, 1):
        if _DIR_KEYS[d][0] not in got["skipped"]:
            _compare_direction(tag, d, got, ref, np.asarray(p), np.asarray(v), faces, device, exact, delta)
    want = ref["sums"].copy()
    for d in (0, 1):
        if _DIR_KEYS[d][0] in got["skipped"]:
            want[:, d] = 0.0                              # the column of a direction that was not searched is written as 0
    es = float(np.max(np.abs(got["sums"] - want) / np.maximum(np.abs(want), 1e-300)))
    eo = abs(float(got["out"][0]) - ref["value"])
    print(f"[point_mesh] {tag}: sums relative error {es:.2e} (bound 1e-12); out {float(got['out'][0]):.9e} ref {ref['value']:.9e} "
          f"error {eo:.2e} (bound {EPS32 * abs(ref['value']):.2e})")
    assert es <= 1e-12, (tag, es)
    assert eo <= EPS32 * abs(ref["value"]), (tag, eo, ref["value"])
    for k in ("gp", "gv"):
        if got.get(k) is None:
            continue
        r = ref[k]
        bound = EPS32 * np.abs(r) + 1e-10 * float(np.abs(r).max())
        err = np.abs(got[k].astype(np.float64) - r)
        print(f"[point_mesh] {tag}: {k}: max error {float(err.max()):.2e}, max |ref| {float(np.abs(r).max()):.3e}, worst error / bound "
              f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (tag, k, float(err.max()))


def assert_general_position(tag, ref, p, v):
    """On the restatement alone: no query's best and second-best d2 are closer than DELTA, so the GPU excuse cannot fire on this case."""
    delta = 1e-12 * extent_of(p, v) ** 2
    g0, g1 = float(ref["gap_pf"].min()), float(ref["gap_fp"].min())
    print(f"[point_mesh] {tag}: smallest gap between best and second-best d2: points {g0:.3e}, faces {g1:.3e} (DELTA {delta:.3e})")
    assert g0 >= delta and g1 >= delta, (tag, g0, g1, delta)


def check(tag, lib, device, p, v, faces, w=W, gout=GOUT, exact=False, soup=False, grads="both"):
    ref = pr.point_mesh(p, v, faces, w[0], w[1], gout, second=soup)
    if soup:
        assert_general_position(tag, ref, p, v)
    got = run_kernels(lib, device, p, v, faces, w[0], w[1], gout, grads=grads)
    compare(tag, got, ref, p, v, faces, device, exact=exact)
    return got, ref


# ---- known answers in exact arithmetic --------------------------------------------------------------------------------------------------
TRI = [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]]
# one point in each of the seven regions of TRI (two in the interior), and by hand: d2, the weights, r = p - cp
SEVEN = [  # point,            d2,   weights,             r                     region
    ([-1.0, -2.0, 2.0],        9.0, [1.0, 0.0, 0.0],     [-1.0, -2.0, 2.0]),    # vertex a
    ([6.0, -1.0, 2.0],         9.0, [0.0, 1.0, 0.0],     [2.0, -1.0, 2.0]),     # vertex b
    ([1.0, -2.0, 2.0],         8.0, [0.75, 0.25, 0.0],   [0.0, -2.0, 2.0]),     # edge ab: cp (1, 0, 0)
    ([-1.0, 6.0, 2.0],         9.0, [0.0, 0.0, 1.0],     [-1.0, 2.0, 2.0]),     # vertex c
    ([-2.0, 1.0, 2.0],         8.0, [0.75, 0.0, 0.25],   [-2.0, 0.0, 2.0]),     # edge ac: cp (0, 1, 0)
    ([3.0, 3.0, 2.0],          6.0, [0.0, 0.5, 0.5],     [1.0, 1.0, 2.0]),      # edge bc: cp (2, 2, 0)
    ([1.0, 1.0, 3.0],          9.0, [0.5, 0.25, 0.25],   [0.0, 0.0, 3.0]),      # interior: cp (1, 1, 0)
    ([2.0, 1.0, -1.0],         1.0, [0.25, 0.5, 0.25],   [0.0, 0.0, -1.0]),     # interior: cp (2, 1, 0), the face's own closest point
]


def grid_mesh(n):
    """n x n integer vertices in the plane z = 0 (index = ix n + iy), two triangles per cell"""
    g = np.arange(n, dtype=np.float32)
    verts = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((n, n), np.float32)], -1).reshape(1, n * n, 3).copy()
    faces = []
    for ix in range(n - 1):
        for iy in range(n - 1):
            a, b, c, d = ix * n + iy, (ix + 1) * n + iy, ix * n + iy + 1, (ix + 1) * n + iy + 1
            faces += [[a, b, c], [b, d, c]]
    return verts, np.asarray(faces, np.int32)


def known_answers_case(lib, device):
    # the seven regions: N = 8, F = 1, B = 1, weights (1, 0.5), gout 2: c_pf = 2 / 8 = 0.25, c_fp = 0.5 * 2 / 1 = 1
    pts = np.asarray([[s[0] for s in SEVEN]], np.float32)
    got, _ = check("seven regions", lib, device, pts, [TRI], [[0, 1, 2]], w=(1.0, 0.5), gout=2.0, exact=True)
    assert got["min_pf"].tolist() == [[s[1] for s in SEVEN]] and got["bary_pf"].tolist() == [[s[2] for s in SEVEN]]
    assert got["idx_pf"].tolist() == [[0] * 8] and got["idx_fp"].tolist() == [[7]] and got["min_fp"].tolist() == [[1.0]]
    assert got["bary_fp"].tolist() == [[[0.25, 0.5, 0.25]]] and got["sums"].tolist() == [[59.0, 1.0]]
    assert float(got["out"][0]) == 59.0 / 8.0 + 0.5                                        # 7.875
    # gp[i] = gout c_pf r_i = 0.5 r_i; the point the face chose adds gout c_fp r_7: 2.5 r_7
    assert got["gp"].tolist() == [[[0.5 * x for x in s[3]] for s in SEVEN[:7]] + [[0.0, 0.0, -2.5]]], got["gp"]
    # slab[k] = -(0.25 sum_i w_k(i) r_i + w_k(7) r_7), gv = 2 slab:
    #   sum_i w_0 r_i = (-2.5, -3.5, 6.25), w_1: (2.5, -1, 3.75), w_2: (-1, 2.5, 4); own terms (0, 0, -0.25), (0, 0, -0.5), (0, 0, -0.25)
    assert got["gv"].tolist() == [[[1.25, 1.75, -2.625], [-1.25, 0.5, -0.875], [0.5, -1.25, -1.5]]], got["gv"]
    # degenerate faces, one per sample (the face table is (0, 1, 2) for all): the distance to the segment or point, finite
    verts = np.asarray([[[0, 0, 0], [4, 0, 0], [2, 0, 0]],      # collinear, c between a and b: the segment a .. b
                        [[0, 0, 0], [2, 0, 0], [4, 0, 0]],      # collinear, b between a and c: the segment a .. c
                        [[0, 0, 0], [0, 0, 0], [0, 4, 0]],      # a == b by coordinate: the segment a .. c
                        [[0, 0, 0], [4, 0, 0], [4, 0, 0]],      # b == c: the segment a .. b
                        [[1, 1, 1], [1, 1, 1], [1, 1, 1]]], np.float32)                    # a point
    pts = np.asarray([[[1, 2, 0], [6, 0, 3], [-1, 1, 1]],       # (1, 0, 0): 4; b: 4 + 9; a: 3
                      [[3, 1, 0], [5, 0, 2], [-2, 0, 0]],       # (3, 0, 0): 1; c: 1 + 4; a: 4
                      [[1, 1, 0], [2, -1, 0], [0, 6, 1]],       # (0, 1, 0): 1; a: 5; c: 4 + 1
                      [[1, 2, 0], [6, 1, 0], [-1, 0, 0]],       # (1, 0, 0): 4; b: 4 + 1; a: 1
                      [[1, 1, 3], [0, 1, 1], [3, 3, 2]]], np.float32)                      # 4; 1; 4 + 4 + 1
    got, _ = check("degenerate faces", lib, device, pts, verts, [[0, 1, 2]], w=(1.0, 1.0), gout=1.0, exact=True)
    assert got["min_pf"].tolist() == [[4.0, 13.0, 3.0], [1.0, 5.0, 4.0], [1.0, 5.0, 5.0], [4.0, 5.0, 1.0], [4.0, 1.0, 9.0]], got["min_pf"]
    assert got["min_fp"].tolist() == [[3.0], [1.0], [1.0], [1.0], [1.0]] and got["idx_fp"].tolist() == [[2], [0], [0], [2], [1]]
    assert np.isfinite(got["gp"]).all() and np.isfinite(got["gv"]).all() and np.isfinite(got["bary_pf"]).all()
    assert (got["bary_pf"] >= 0).all() and (got["bary_pf"].sum(-1) == 1.0).all()
    # a planar integer grid (169 vertices, 288 faces: more than one pass) against points ON it -- its vertices and its cell centres (313
    # points: more than one workgroup): value 0, no gradient; every tie goes to the lowest index (compared with the restatement)
    verts, faces = grid_mesh(13)
    centres = (verts[0].reshape(13, 13, 3)[:12, :12] + np.asarray([0.5, 0.5, 0.0], np.float32)).reshape(-1, 3)
    pts = np.concatenate([verts[0], centres])[None]
    got, _ = check("points on a planar grid", lib, device, pts, verts, faces, w=(1.0, 1.0), exact=True)
    assert float(got["out"][0]) == 0.0 and not got["sums"].any() and not got["gp"].any() and not got["gv"].any()
    assert not got["min_pf"].any() and not got["min_fp"].any()


# ---- the boundaries of a workgroup's queries and of an LDS pass -----------------------------------------------------------------------
def boundary_case(lib, device, N, F, B=2):
    """A seeded soup at one (N, F) of boundary_sizes.  Indices, weights, minima, values and gradients."""
    p, v, faces = seeded_soup(B, N, soup_verts(F), F, seed=1000 * N + F)
    check(f"boundary B={B} N={N} F={F}", lib, device, p, v, faces, soup=True)


# ---- ties across passes and waves ------------------------------------------------------------------------------------------------------
def tie_layouts(t):
    """(name, positions of the duplicated element in the searched set) for a pass of t elements: across passes, at a pass boundary, and
    inside one pass at the first and last element of two different waves' shares."""
    s = t // 4
    return [("0, T-1, T, 2T+1", [0, t - 1, t, 2 * t + 1]), ("T, T+3", [t, t + 3]), ("T-1, T", [t - 1, t]),
            ("first of share 1, last of share 2", [s, 3 * s - 1]), ("last of share 0, first of share 2", [s - 1, 2 * s]),
            ("last of share 1, first of share 3, second pass", [t + 2 * s - 1, t + 3 * s]), ("first of share 0, last of share 3", [0, t - 1])]


def tie_case(lib, device):
    """Points -> faces: the table lists ONE face (the same three vertex indices) at several positions, the points are nearest to it: every
    point reports the LOWEST position.  Faces -> points: the set holds one point several times, the faces are nearest to it.  The
    duplicates have identical records, so their d2 have identical bits on any machine: no excuse."""
    qp, tf, qf, tp = geometry(lib)
    g = torch.Generator().manual_seed(5)
    # points -> faces
    n_f, n_q = 2 * tf + 5, qp + 1
    far = (torch.rand(1, 3 * n_f, 3, generator=g) + 2.0).numpy()                        # the other faces: in the box [2, 3]^3
    near = np.asarray([[0.25, -0.5, 0.125], [0.375, -0.5, 0.25], [0.25, -0.375, 0.0]], np.float32)
    verts = np.concatenate([far, near[None]], 1)
    queries = (near.mean(0) + 0.05 * (torch.rand(1, n_q, 3, generator=g).numpy() - 0.5)).astype(np.float32)
    for name, pos in tie_layouts(tf):
        faces = np.arange(3 * n_f, dtype=np.int32).reshape(n_f, 3)
        faces[pos] = [3 * n_f, 3 * n_f + 1, 3 * n_f + 2]
        got, _ = check(f"one face at {name}", lib, device, queries, verts, faces, exact=True)
        assert (got["idx_pf"] == min(pos)).all(), (name, np.unique(got["idx_pf"]).tolist(), min(pos))
    # faces -> points
    n_p, n_q = 2 * tp + 5, qf + 1
    farp = (torch.rand(1, n_p, 3, generator=g) + 2.0).numpy()
    dup = np.asarray([0.25, -0.5, 0.125], np.float32)
    verts = (dup + 0.05 * (torch.rand(1, 3 * n_q, 3, generator=g).numpy() - 0.5)).astype(np.float32)
    faces = np.arange(3 * n_q, dtype=np.int32).reshape(n_q, 3)
    for name, pos in tie_layouts(tp):
        pts = farp.copy()
        pts[0, pos] = dup
        got, _ = check(f"one point at {name}", lib, device, pts, verts, faces, exact=True)
        assert (got["idx_fp"] == min(pos)).all(), (name, np.unique(got["idx_fp"]).tolist(), min(pos))


# ---- the sizes of the product -------------------------------------------------------------------------------------------------------------
_MANO = {}


def mano_inputs(B):
    """The MANO topology (778 vertices, 1538 faces of synthetic_mano_tables): the template, per sample a little larger and moved by seeded
    millimetres; 778 points: the template's vertices moved by other seeded millimetres."""
    if B not in _MANO:
        from hifihr_amd.mano_tables import synthetic_mano_tables
        t = synthetic_mano_tables(0)
        vt = np.asarray(t.v_template, np.float32)
        g = torch.Generator().manual_seed(778)
        v = (vt[None] * 1.02 + 0.002 * torch.randn(B, 778, 3, generator=g).numpy()).astype(np.float32)
        p = (vt[None] + 0.003 * torch.randn(B, 778, 3, generator=g).numpy()).astype(np.float32)
        _MANO[B] = (p, v, np.asarray(t.faces, np.int32))
    return _MANO[B]


def mano_case(lib, device, B):
    p, v, faces = mano_inputs(B)
    assert p.shape == (B, 778, 3) and v.shape == (B, 778, 3) and faces.shape == (1538, 3)
    check(f"MANO topology B={B}", lib, device, p, v, faces)


def soup_product_case(lib, device, B, N, F):
    p, v, faces = seeded_soup(B, N, soup_verts(F), F, seed=N + F)
    check(f"soup B={B} N={N} F={F}", lib, device, p, v, faces, soup=True)


# ---- weights of exactly zero, NULL gradients ----------------------------------------------------------------------------------------------
def _small_soup(lib, seed):
    qp, tf, qf, tp = geometry(lib)
    return seeded_soup(2, qp + 1, soup_verts(qf + 1), qf + 1, seed=seed)


def zero_weight_case(lib, device):
    """Each direction with a weight of exactly 0: its arrays keep their canaries (run_kernels), value and gradients are the restatement's,
    and the other direction has the bits it has when both are searched."""
    p, v, faces = _small_soup(lib, 11)
    full = run_kernels(lib, device, p, v, faces, *W)
    for w, kept in (((0.0, W[1]), 1), ((W[0], 0.0), 0)):
        got, _ = check(f"weights {w}", lib, device, p, v, faces, w=w, soup=True)
        assert set(_DIR_KEYS[1 - kept]) == got["skipped"]
        for k in _DIR_KEYS[kept]:
            assert (got[k].view(np.int64 if got[k].dtype == np.float64 else np.int32) ==
                    full[k].view(np.int64 if full[k].dtype == np.float64 else np.int32)).all(), (w, k)
        assert (got["sums"][:, kept] == full["sums"][:, kept]).all() and not got["sums"][:, 1 - kept].any()
    got = run_kernels(lib, device, p, v, faces, 0.0, 0.0)
    assert float(got["out"][0]) == 0.0 and not got["gp"].any() and not got["gv"].any() and not got["sums"].any()
    assert got["skipped"] == set(_DIR_KEYS[0]) | set(_DIR_KEYS[1])


def null_gradient_case(lib, device):
    """gv_d NULL, then gp_d NULL: the other gradient has the bits of the run with both."""
    p, v, faces = _small_soup(lib, 12)
    both = run_kernels(lib, device, p, v, faces, *W)
    only_p, only_v = run_kernels(lib, device, p, v, faces, *W, grads="p"), run_kernels(lib, device, p, v, faces, *W, grads="v")
    assert only_p["gv"] is None and only_v["gp"] is None
    assert (only_p["gp"].view(np.int32) == both["gp"].view(np.int32)).all() and (only_v["gv"].view(np.int32) == both["gv"].view(np.int32)).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
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
        assert torch.equal(_bits(o), _bits(b)), f"{name}: {what}: refused but wrote an output"


def refusal_case(lib, device):
    from hifihr_amd._lib import _fp as fp, _ip as ip
    cf, vp = ctypes.c_float, lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    B, N, V, F = 2, 5, 23, 7
    ps, vs, fs = seeded_soup(B, N, V, F, seed=3)
    p, v, faces = torch.as_tensor(ps).to(device), torch.as_tensor(vs).to(device), torch.as_tensor(fs).to(device)
    off, corner = device_tables(fs, V, device)
    # the workspace size: 0 for what is refused, never decreasing with B
    sizes = [lib.point_mesh_workspace_bytes(b, N, V, F) for b in range(6)]
    assert sizes[0] == 0 and sizes[1] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    for bad in ((-1, N, V, F), (B, 0, V, F), (B, N, 0, F), (B, N, V, 0)):
        assert lib.point_mesh_workspace_bytes(*bad) == 0, bad
    sent = lambda shape, dtype: torch.full(shape, _CANARY[dtype], dtype=dtype, device=device)
    i_pf, i_fp = sent((B, N), torch.int32), sent((B, F), torch.int32)
    b_pf, b_fp, m_pf, m_fp = sent((B, N, 3), torch.float64), sent((B, F, 3), torch.float64), sent((B, N), torch.float64), sent((B, F), torch.float64)
    sums, out, ws = sent((B, 2), torch.float64), sent((1,), torch.float32), sent((sizes[B] // 8,), torch.float64)
    gp, gv = sent((B, N, 3), torch.float32), sent((B, V, 3), torch.float32)
    good_pf, good_fp = torch.zeros(B, N, dtype=torch.int32, device=device), torch.zeros(B, F, dtype=torch.int32, device=device)
    good_bpf, good_bfp = torch.zeros(B, N, 3, dtype=torch.float64, device=device), torch.zeros(B, F, 3, dtype=torch.float64, device=device)
    gout = torch.ones(1, device=device)
    big = 1 << 30                                                   # N = F = 1: one chunk each, 2 B chunks = 2^31 > 2^31 - 1
    bad = [("B < 0", dict(B=-1)), ("N < 1", dict(N=0)), ("V < 1", dict(V=0)), ("F < 1", dict(F=0)), ("N < 0", dict(N=-3)),
           ("grid past 2^31 - 1", dict(B=big, N=1, V=1, F=1)), ("w_pf NaN", dict(wp=float("nan"))), ("w_pf inf", dict(wp=float("inf"))),
           ("w_fp NaN", dict(wf=float("nan"))), ("w_fp -inf", dict(wf=float("-inf")))]
    outs_f = (i_pf, b_pf, m_pf, i_fp, b_fp, m_fp, sums, out, ws)
    base = dict(p=fp(p), v=fp(v), faces=ip(faces), B=B, N=N, V=V, F=F, wp=0.7, wf=1.3, ipf=ip(i_pf), bpf=vp(b_pf), mpf=vp(m_pf), ifp=ip(i_fp),
                bfp=vp(b_fp), mfp=vp(m_fp), sums=vp(sums), out=fp(out), ws=vp(ws))
    nulls = ("p", "v", "faces", "ipf", "bpf", "mpf", "ifp", "bfp", "mfp", "sums", "out", "ws")
    for what, change in [(f"{k} NULL", {k: None}) for k in nulls] + bad:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_point_mesh_fwd", (a["p"], a["v"], a["faces"], a["B"], a["N"], a["V"], a["F"], cf(a["wp"]), cf(a["wf"]),
                                                         a["ipf"], a["bpf"], a["mpf"], a["ifp"], a["bfp"], a["mfp"], a["sums"], a["out"], a["ws"],
                                                         None), outs_f, what)
    base = dict(p=fp(p), v=fp(v), faces=ip(faces), ipf=ip(good_pf), bpf=vp(good_bpf), ifp=ip(good_fp), bfp=vp(good_bfp), gout=fp(gout), off=ip(off),
                corner=ip(corner), B=B, N=N, V=V, F=F, wp=0.7, wf=1.3, gp=fp(gp), gv=fp(gv), ws=vp(ws))
    bwd_args = lambda a: (a["p"], a["v"], a["faces"], a["ipf"], a["bpf"], a["ifp"], a["bfp"], a["gout"], a["off"], a["corner"], a["B"], a["N"],
                          a["V"], a["F"], cf(a["wp"]), cf(a["wf"]), a["gp"], a["gv"], a["ws"], None)
    nulls = ("p", "v", "faces", "ipf", "bpf", "ifp", "bfp", "gout", "off", "corner", "ws")
    for what, change in [(f"{k} NULL", {k: None}) for k in nulls] + bad:
        _refused(lib, device, "hifihr_point_mesh_bwd", bwd_args(dict(base, **change)), (gp, gv, ws), what)
    # accepted no-ops: B == 0, and a backward without a gradient to write: nothing launched, nothing written
    if device == "cpu":
        kc.launch_log(lib)
    assert lib.c.hifihr_point_mesh_fwd(fp(p), fp(v), ip(faces), 0, N, V, F, cf(0.7), cf(1.3), ip(i_pf), vp(b_pf), vp(m_pf), ip(i_fp), vp(b_fp),
                                       vp(m_fp), vp(sums), fp(out), vp(ws), None) == 0
    assert lib.c.hifihr_point_mesh_bwd(*bwd_args(dict(base, B=0))) == 0
    assert lib.c.hifihr_point_mesh_bwd(*bwd_args(dict(base, gp=None, gv=None))) == 0
    if device == "cpu":
        assert not kc.launch_log(lib)
    else:
        torch.cuda.synchronize()
    for t in outs_f + (gp, gv):
        assert bool((t == _CANARY[t.dtype]).all())
    null = ctypes.POINTER(ctypes.c_int32)()
    lib.c.hifihr_point_mesh_geometry(null, null, null, null)        # any pointer may be NULL
