"""Shared bodies of the mesh-regulariser tests (hifihr_mesh_topology_* / hifihr_mesh_reg_fwd / _bwd, csrc/mesh_reg.hip):
tests/test_hostsim_mesh_reg.py runs them on the emulator (device='cpu'), tests/test_gpu_mesh_reg.py on the MI355X (device='cuda').
The reference is the float64 restatement of tests/mesh_reg_ref.py on the float32 inputs.

Tolerance.  The yardstick of a case is the error of the SAME restatement run by torch in float32 on the CPU, against float64.  The kernel
does the same arithmetic in another summation order, so it may be at most KERNEL_OVER_F32 = 4 times that, with a floor of FLOOR = 1e-6 of
the largest reference magnitude of what is compared (the float32 run is sometimes exact): per case
    max |out - ref| <= max(4 max |out32 - ref|, 1e-6 max |ref|),    max |gverts - gref| <= max(4 max |g32 - gref|, 1e-6 max |gref|),
and the same for each of the two terms of out by itself (the smaller term must not hide behind the larger one's floor).
PRECISION collects (tag, float32 error, kernel error, both relative to the largest reference magnitude) per case;
tools/mesh_reg_precision.py writes them to profiles/mesh_reg_precision.txt."""
import ctypes
import math

import numpy as np
import torch

import kernel_cases as kc
import mesh_reg_ref as mr

EINVAL = -1
KERNEL_OVER_F32, FLOOR = 4.0, 1e-6
LAM = (0.1, 0.01)                  # lambda_laplacian, lambda_normal_consistency of hifihr_amd/options.py
GOUT = (0.7, -1.3)                 # unequal and of opposite sign: a mix-up of the two terms shows
KERNELS = {"mesh_reg_fwd_kernel", "mesh_reg_finish_kernel", "mesh_reg_bwd_kernel"}
PRECISION = []

# (B, n, m): jittered n x m grids.  (1, 2, 2) = 4 vertices and one quad; (2, 20, 15) = 300 vertices: two workgroups, a ragged tail
RANDOM_CASES = [(1, 2, 2), (3, 5, 7), (2, 20, 15)]


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def grid_faces(n, m):
    """n x m vertices (row-major), every cell split along the same diagonal."""
    f = []
    for i in range(n - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, i * m + j + 1, (i + 1) * m + j, (i + 1) * m + j + 1
            f += [(a, b, d), (a, d, c)]
    return np.asarray(f, dtype=np.int32)


def grid_verts(n, m, B=1, jitter=0.0, seed=0):
    """Unit spacing, centred at the origin; jitter uniform in +-jitter per coordinate, z included."""
    ii, jj = torch.meshgrid(torch.arange(n, dtype=torch.float32), torch.arange(m, dtype=torch.float32), indexing="ij")
    base = torch.stack([jj - (m - 1) / 2.0, ii - (n - 1) / 2.0, torch.zeros_like(ii)], -1).reshape(1, n * m, 3).repeat(B, 1, 1)
    if jitter:
        base = base + (torch.rand(B, n * m, 3, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0) * jitter
    return base.contiguous()


TETRA_VERTS = [(1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0)]
TETRA_FACES = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
BOOK_FACES = [(0, 1, 2), (0, 1, 3), (1, 0, 4)]                          # three triangles on the edge (0, 1)


def fan_faces(n=70):
    """An open fan of n triangles round vertex 0 over the rim 1 .. n + 1: the hub has degree n + 1."""
    return np.asarray([(0, 1 + k, 2 + k) for k in range(n)], dtype=np.int32)


def hinge(phi, flip=None):
    """Two triangles on the shared edge (0, 1), the second folded by phi out of the first one's plane (0 = flat)."""
    verts = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.5, -math.cos(phi), math.sin(phi)]]], dtype=torch.float32)
    faces = [[0, 1, 2], [1, 0, 3]]
    if flip is not None:
        faces[flip] = faces[flip][::-1]
    return verts, np.asarray(faces, dtype=np.int32)


# ---- driving the C ABI ----------------------------------------------------------------------------------------------------------------
class Topology:
    def __init__(self, lib, faces, V):
        self.lib, self.V = lib, int(V)
        self.h = lib.mesh_topology_create(np.ascontiguousarray(np.asarray(faces), dtype=np.int32), V)

    def counts(self):
        return self.lib.mesh_topology_counts(self.h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.mesh_topology_destroy(self.h)


def run_kernels(lib, device, topo, verts, lam_lap, lam_nc, gout=GOUT):
    """-> (out [2], unit [B,V,3], gverts [B,V,3]) as float64 CPU tensors.  Every output starts as NaN inside guard bands and must come
    back fully written with the bands untouched; forward and backward run twice: the same bits both times."""
    B, V = verts.shape[0], verts.shape[1]
    g = kc.Guards(device)
    v, go = g.inp(verts.float()), g.inp(torch.tensor(gout, dtype=torch.float32))
    runs = []
    for _ in range(2):
        out, unit = g.out(2, fill=float("nan")), g.out(B, V, 3, fill=float("nan"))
        partial = g.out(lib.mesh_reg_partial_floats(topo.h, B), fill=float("nan"))
        gverts = g.out(B, V, 3, fill=float("nan"))
        lib.mesh_reg_fwd(topo.h, v, lam_lap, lam_nc, unit, partial, out)
        lib.mesh_reg_bwd(topo.h, v, unit, go, lam_lap, lam_nc, gverts)
        runs.append((out, unit, gverts))
    for a, b, name in zip(runs[0], runs[1], ("out", "unit", "gverts")):
        assert not bool(torch.isnan(a).any()), f"{name}: an element was not written"
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two calls differ in their bits"
    g.intact("mesh regularisers")
    return tuple(t.double().cpu() for t in runs[0])


def _bound(err32, ref):
    return max(KERNEL_OVER_F32 * err32, FLOOR * float(ref.abs().max()))


def check_against_restatement(tag, lib, device, verts, faces, lam=LAM, gout=GOUT):
    """out and gverts of the kernels against the float64 restatement, bounded by the float32 restatement's own error (module docstring);
    then each weight set to 0 in turn: the zeroed term is exactly 0 and the gradient is the other term's alone."""
    V = verts.shape[1]
    topo = mr.topology(faces, V)
    ref = mr.mesh_regularizers(verts, faces, lam[0], lam[1], gout=gout, topo=topo)
    r32 = mr.mesh_regularizers(verts, faces, lam[0], lam[1], gout=gout, topo=topo, dtype=torch.float32)
    with Topology(lib, faces, V) as t:
        assert t.counts() == (V, len(topo["edges"]), len(topo["quads"])), (t.counts(), V, len(topo["edges"]), len(topo["quads"]))
        out, unit, gverts = run_kernels(lib, device, t, verts, lam[0], lam[1], gout)
        halves = [run_kernels(lib, device, t, verts, lam[0], 0.0, gout), run_kernels(lib, device, t, verts, 0.0, lam[1], gout)]
    omax, gmax = float(ref["out"].abs().max()), float(ref["gverts"].abs().max())
    e32_o, e32_g = float((r32["out"].double() - ref["out"]).abs().max()), float((r32["gverts"].double() - ref["gverts"]).abs().max())
    ek_o, ek_g = float((out - ref["out"]).abs().max()), float((gverts - ref["gverts"]).abs().max())
    rel = lambda e, m: e / m if m > 0 else e
    PRECISION.append((tag, device, rel(e32_o, omax), rel(ek_o, omax), rel(e32_g, gmax), rel(ek_g, gmax)))
    print(f"[mesh_reg] {tag}: out {out.tolist()} error float32 {rel(e32_o, omax):.2e} kernel {rel(ek_o, omax):.2e} of max|ref|; "
          f"gradient error float32 {rel(e32_g, gmax):.2e} kernel {rel(ek_g, gmax):.2e} of max|gref| = {gmax:.3e}")
    assert ek_o <= _bound(e32_o, ref["out"]), (tag, ek_o, e32_o, omax)
    for k in range(2):                                              # ... and each term by itself, so that the larger one hides nothing
        ek, e32 = abs(float(out[k] - ref["out"][k])), abs(float(r32["out"][k].double() - ref["out"][k]))
        print(f"[mesh_reg] {tag}: term {k}: float32 {e32:.2e} kernel {ek:.2e} reference {float(ref['out'][k]):.6e}")
        assert ek <= _bound(e32, ref["out"][k]), (tag, k, ek, e32)
    assert ek_g <= _bound(e32_g, ref["gverts"]), (tag, ek_g, e32_g, gmax)
    assert bool(torch.isfinite(gverts).all())
    # a weight of exactly 0: that term is exactly 0, the other one has the bits it had, and the gradient is the other term's alone
    for k, (o, u, gv) in enumerate(halves):                         # k = the index of the term that is KEPT
        lam_k = (lam[0], 0.0) if k == 0 else (0.0, lam[1])
        rk = mr.mesh_regularizers(verts, faces, lam_k[0], lam_k[1], gout=gout, topo=topo)
        r32k = mr.mesh_regularizers(verts, faces, lam_k[0], lam_k[1], gout=gout, topo=topo, dtype=torch.float32)
        assert float(o[1 - k]) == 0.0 and float(o[k]) == float(out[k]), (tag, k, o.tolist(), out.tolist())
        e32 = float((r32k["gverts"].double() - rk["gverts"]).abs().max())
        assert float((gv - rk["gverts"]).abs().max()) <= _bound(e32, rk["gverts"]), (tag, k)
        if k == 1:
            assert not bool(u.any()), "unit_d is written as zeros when lam_lap == 0"
    return ref, out, unit, gverts


def random_case(lib, device, B, n, m):
    verts, faces = grid_verts(n, m, B, jitter=0.25, seed=100 * n + m), grid_faces(n, m)
    ref, *_ = check_against_restatement(f"grid B={B} {n}x{m}", lib, device, verts, faces)
    assert float(mr.laplacian_d(verts.double(), ref["topo"]).norm(dim=-1).min()) > 1e-3, "a zero d: the case is meant to have none"


def mano_case(lib, device, tables, B=2):
    """The MANO template with 2 mm of noise: 778 vertices, E = 2315, Q = 2299 (four workgroups of vertices, nine of quads)."""
    faces = np.asarray(tables.faces, dtype=np.int32)
    v0 = torch.as_tensor(np.asarray(tables.v_template), dtype=torch.float32)
    verts = (v0[None] + 0.002 * torch.randn(B, 778, 3, generator=torch.Generator().manual_seed(0))).contiguous()
    ref, *_ = check_against_restatement(f"mano B={B}", lib, device, verts, faces)
    t = ref["topo"]
    assert (len(t["edges"]), len(t["quads"]), int(t["deg"].min()), int(t["deg"].max()), t["boundary"]) == (2315, 2299, 4, 7, 16)


# ---- known answers --------------------------------------------------------------------------------------------------------------------
def known_answers_case(lib, device):
    """Closed forms.  The kernel is held to them to 1e-6 (its inputs are float32 roundings of the closed form's)."""
    # regular tetrahedron: every vertex has the three others as neighbours, d = -(4/3) v, |d| = 4 / sqrt(3); the normals of two faces meet
    # at the dihedral angle acos(1/3) and the two n of a record point to opposite sides: cos = -1/3
    verts = torch.tensor([TETRA_VERTS], dtype=torch.float32)
    with Topology(lib, TETRA_FACES, 4) as t:
        assert t.counts() == (4, 6, 6)
        out, _, g = run_kernels(lib, device, t, verts, 1.0, 1.0)
    assert abs(float(out[0]) - 4.0 / math.sqrt(3.0)) <= 1e-6 * 4.0 / math.sqrt(3.0) and abs(float(out[1]) - 4.0 / 3.0) <= 1e-6 * 4.0 / 3.0, out.tolist()
    rt = mr.mesh_regularizers(verts, TETRA_FACES, 1.0, 1.0, gout=GOUT)
    assert float((g - rt["gverts"]).abs().max()) <= 1e-6 * float(rt["gverts"].abs().max())
    # two triangles hinged on an edge: nc = 1 - cos(phi), whatever the winding of either
    for phi in (0.0, math.pi / 3, math.pi / 2):
        for flip in (None, 0, 1):
            verts, faces = hinge(phi, flip)
            with Topology(lib, faces, 4) as t:
                assert t.counts() == (4, 5, 1)
                out, _, _ = run_kernels(lib, device, t, verts, 1.0, 1.0)
            assert abs(float(out[1]) - (1.0 - math.cos(phi))) <= 1e-6, (phi, flip, float(out[1]))
    # flat 4 x 4 grid, unit spacing (float32 is exact on it: integer normals of length 1, cos = 1; the mean of an interior vertex's six
    # neighbours is a correctly rounded division of six times its own coordinates)
    verts, faces = grid_verts(4, 4), grid_faces(4, 4)
    ref = mr.mesh_regularizers(verts, faces, 1.0, 1.0, gout=GOUT)
    with Topology(lib, faces, 16) as t:
        assert t.counts() == (16, 33, 21)
        out, unit, g = run_kernels(lib, device, t, verts, 1.0, 1.0)
    assert float(out[1]) == 0.0 and float(ref["out"][1]) == 0.0
    assert abs(float(out[0]) - float(ref["out"][0])) <= 1e-6 * float(ref["out"][0]) and float(ref["out"][0]) > 0.1
    interior = [5, 6, 9, 10]
    assert not bool(unit[0, interior].any()) and not bool(ref["unit"][0, interior].any()), "d = 0 exactly at the four interior vertices"
    assert bool(torch.isfinite(g).all()) and float((g - ref["gverts"]).abs().max()) <= 1e-6 * float(ref["gverts"].abs().max())


# ---- topology -------------------------------------------------------------------------------------------------------------------------
def topology_case(lib, device, tables):
    """hifihr_mesh_topology_counts against the Python count of mesh_reg_ref.topology."""
    meshes = [(f"grid {n}x{m}", grid_faces(n, m), n * m) for _, n, m in RANDOM_CASES] + [("grid 4x4", grid_faces(4, 4), 16)]
    meshes += [("mano", np.asarray(tables.faces, dtype=np.int32), 778), ("book", np.asarray(BOOK_FACES, dtype=np.int32), 5),
               ("fan", fan_faces(70), 72)]
    for name, faces, V in meshes:
        ref = mr.topology(faces, V)
        with Topology(lib, faces, V) as t:
            assert t.counts() == (V, len(ref["edges"]), len(ref["quads"])), (name, t.counts())
    assert len(mr.topology(BOOK_FACES, 5)["quads"]) == 3
    assert int(mr.topology(meshes[-1][1], 72)["deg"][0]) == 71
    assert (len(mr.topology(grid_faces(4, 4), 16)["edges"]), len(mr.topology(grid_faces(4, 4), 16)["quads"])) == (33, 21)
    m = mr.topology(meshes[4][1], 778)
    assert (len(m["edges"]), len(m["quads"])) == (2315, 2299)


def fan_case(lib, device):
    """A hub of degree 71 with 69 quad roles (well past any fixed unroll), and the book: an edge with three faces."""
    gen = torch.Generator().manual_seed(7)
    ang = torch.arange(71, dtype=torch.float32) * (1.6 * math.pi / 70)
    rim = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros(71)], -1)
    verts = torch.cat([torch.tensor([[0.0, 0.0, 0.4]]), rim])[None].repeat(2, 1, 1)
    verts = (verts + 0.02 * (torch.rand(2, 72, 3, generator=gen) * 2.0 - 1.0)).contiguous()
    ref, *_ = check_against_restatement("fan of 70", lib, device, verts, fan_faces(70))
    assert int(ref["topo"]["deg"][0]) == 71 and len(ref["topo"]["quads"]) == 69
    bv = (torch.rand(1, 5, 3, generator=gen) * 2.0 - 1.0).contiguous()
    ref, *_ = check_against_restatement("book", lib, device, bv, np.asarray(BOOK_FACES, dtype=np.int32))
    assert len(ref["topo"]["quads"]) == 3


def isolated_vertex_case(lib, device):
    """A vertex that no face references: deg = 0, d = -v, its gradient is -u (1 / (B V)) and it is in no quad."""
    n, m = 3, 4
    faces = grid_faces(n, m)
    faces = np.where(faces >= 5, faces + 1, faces).astype(np.int32)                # vertex 5 is left out
    verts = torch.cat([grid_verts(n, m, 2, jitter=0.25, seed=3), torch.tensor([[[0.3, -0.2, 0.5]], [[-0.1, 0.4, 0.2]]])], 1)
    verts = verts[:, [0, 1, 2, 3, 4, 12, 5, 6, 7, 8, 9, 10, 11]].contiguous()
    ref, _, unit, gverts = check_against_restatement("isolated vertex", lib, device, verts, faces)
    assert int(ref["topo"]["deg"][5]) == 0
    want = -verts[:, 5].double() / verts[:, 5].double().norm(dim=-1, keepdim=True)
    assert float((unit[:, 5] - want).abs().max()) <= 1e-6
    assert float((gverts[:, 5] - (-want) * GOUT[0] * float(np.float32(LAM[0])) / (2 * 13)).abs().max()) <= 1e-6 * float(gverts.abs().max())


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
        assert torch.equal(o.view(torch.int32), b.view(torch.int32)), f"{name}: {what}: refused but wrote an output"


def refusal_case(lib, device):
    from hifihr_amd._lib import HifihrError, _c_int_p, _fp as fp
    cf = ctypes.c_float
    # creation
    good = np.asarray([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(_c_int_p)
    create = lib.c.hifihr_mesh_topology_create
    assert not create(None, 2, 4) and not create(ip(good), 0, 4) and not create(ip(good), -1, 4) and not create(ip(good), 2, 0)
    assert not create(ip(good), 2, 3), "index 3 with V = 3"
    for bad in ([[0, 1, 2], [0, -1, 3]], [[0, 1, 1], [0, 2, 3]], [[0, 1, 2], [3, 2, 3]]):
        b = np.asarray(bad, dtype=np.int32)
        assert not create(ip(b), 2, 4), bad
        try:
            lib.mesh_topology_create(b, 4)
        except HifihrError as e:
            assert "hifihr_mesh_topology_create" in str(e)
        else:
            raise AssertionError(f"{bad}: the binding did not raise")
    assert lib.c.hifihr_mesh_topology_destroy(None) == 0
    assert lib.c.hifihr_mesh_topology_counts(None, None, None, None) == EINVAL
    # compute entries
    B, n, m = 2, 3, 4
    V = n * m
    verts = grid_verts(n, m, B, jitter=0.25, seed=1).to(device)
    with Topology(lib, grid_faces(n, m), V) as t:
        assert lib.c.hifihr_mesh_topology_counts(t.h, None, None, None) == 0
        sizes = [lib.mesh_reg_partial_floats(t.h, b) for b in range(5)]
        assert sizes[0] == 0 and sizes[1] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert lib.mesh_reg_partial_floats(None, 2) == 0 and lib.mesh_reg_partial_floats(t.h, -1) == 0
        nan = lambda *s: torch.full(s, float("nan"), device=device)
        out, unit, partial, gverts = nan(2), nan(B, V, 3), nan(sizes[B]), nan(B, V, 3)
        good_unit, gout = torch.zeros(B, V, 3, device=device), torch.ones(2, device=device)
        big = (1 << 31) // (3 * V) + 1                                # the smallest B with B V 3 >= 2^31
        assert (big - 1) * V * 3 < (1 << 31) <= big * V * 3
        bad = [("B < 0", dict(B=-1)), ("B V 3 >= 2^31", dict(B=big)), ("lam_lap NaN", dict(ll=float("nan"))), ("lam_lap inf", dict(ll=float("inf"))),
               ("lam_nc NaN", dict(ln=float("nan"))), ("lam_nc -inf", dict(ln=float("-inf")))]
        base = dict(h=t.h, verts=fp(verts), B=B, ll=0.1, ln=0.01, unit=fp(unit), partial=fp(partial), out=fp(out))
        for what, change in [(f"{k} NULL", {k: None}) for k in ("h", "verts", "unit", "partial", "out")] + bad:
            a = dict(base, **change)
            _refused(lib, device, "hifihr_mesh_reg_fwd", (a["h"], a["verts"], a["B"], cf(a["ll"]), cf(a["ln"]), a["unit"], a["partial"], a["out"], None),
                     (out, unit, partial), what)
        base = dict(h=t.h, verts=fp(verts), unit=fp(good_unit), gout=fp(gout), B=B, ll=0.1, ln=0.01, gverts=fp(gverts))
        for what, change in [(f"{k} NULL", {k: None}) for k in ("h", "verts", "unit", "gout", "gverts")] + bad:
            a = dict(base, **change)
            _refused(lib, device, "hifihr_mesh_reg_bwd", (a["h"], a["verts"], a["unit"], a["gout"], a["B"], cf(a["ll"]), cf(a["ln"]), a["gverts"], None),
                     (gverts,), what)
        # B == 0: accepted, nothing launched, nothing written
        if device == "cpu":
            kc.launch_log(lib)
        assert lib.c.hifihr_mesh_reg_fwd(t.h, fp(verts), 0, cf(0.1), cf(0.01), fp(unit), fp(partial), fp(out), None) == 0
        assert lib.c.hifihr_mesh_reg_bwd(t.h, fp(verts), fp(good_unit), fp(gout), 0, cf(0.1), cf(0.01), fp(gverts), None) == 0
        if device == "cpu":
            assert not kc.launch_log(lib)
        else:
            torch.cuda.synchronize()
        assert all(bool(torch.isnan(x).all()) for x in (out, unit, partial, gverts))
