"""Shared bodies of the Chamfer-distance tests (hifihr_chamfer_fwd / _bwd, csrc/chamfer.hip): tests/test_hostsim_chamfer.py runs them on
the emulator (device='cpu'), tests/test_gpu_chamfer.py on the MI355X (device='cuda').  The reference is the float64 restatement of
tests/chamfer_ref.py; tests/golden/chamfer.npz pins the restatement's value to the reference's own ChamferLoss.

Bounds (include/hifihr.h "Chamfer distance"; the kernels and the restatement evaluate ONE fp64 expression without contraction):
    idx_*    equal as integers;            min_*   equal as float64 bits
    sums_d   within 1e-12 relative: an fp64 sum of at most 5990 non-negative terms in any order stays inside that
    out_d    within 2^-23 |ref|: one fp32 rounding of an fp64 value
    gx, gy   every component within 2^-23 |ref| + 1e-10 max |ref over the tensor|: accumulated in fp64, rounded once; the second term leaves
             more than two orders of magnitude over the fp64 noise of a 5990-term sum
Q (queries per workgroup) and T (searched points per LDS pass) come from hifihr_chamfer_geometry; the four waves of a workgroup scan
consecutive quarters of a pass.  The cases are built from them."""
import ctypes

import numpy as np
import torch

import chamfer_ref as cr
import kernel_cases as kc

EINVAL = -1
W = (0.7, 1.3)                     # unequal weights: a mix-up of the two directions shows
GOUT = -1.7
KERNELS = {"chamfer_search_kernel", "chamfer_finish_kernel", "chamfer_bwd_kernel"}
EPS32 = 2.0 ** -23
_PAD = 64                          # guard elements on each side of every output
_CANARY = {torch.int32: -7, torch.float64: -1234.5, torch.float32: -1234.5}


def geometry(lib):
    q, t = lib.chamfer_geometry()
    assert q >= 64 and q % 64 == 0 and t >= 4 and t % 4 == 0, (q, t)
    return q, t


def boundary_sizes(lib):
    q, t = geometry(lib)
    return [1, q - 1, q, q + 1, 2 * q + 3], [1, t - 1, t, t + 1, 2 * t + 5]


def seeded_points(B, N, M, seed):
    """Uniform in a 20 cm box, float32: hand-sized sets in metres."""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, N, 3, generator=g) - 0.5) * 0.2).numpy(), ((torch.rand(B, M, 3, generator=g) - 0.5) * 0.2 + 0.01).numpy()


class _Outs:
    """Outputs inside larger allocations: _PAD canary elements on each side, which must come back unchanged."""

    def __init__(self, device):
        self.device, self.items = device, []

    def new(self, shape, dtype, fill):
        n = int(np.prod(shape))
        whole = torch.full((_PAD + n + _PAD,), _CANARY[dtype], dtype=dtype, device=self.device)
        view = whole[_PAD:_PAD + n].view(*shape)
        view.fill_(fill)
        self.items.append((whole, n, _CANARY[dtype]))
        return view

    def intact(self):
        for whole, n, canary in self.items:
            assert bool((whole[:_PAD] == canary).all()) and bool((whole[_PAD + n:] == canary).all()), "wrote outside an output (guard band changed)"


def _bits(t):
    return t.view(torch.int64) if t.element_size() == 8 else t.view(torch.int32)


def run_kernels(lib, device, x, y, w_xy, w_yx, gout=GOUT, grads="both"):
    """-> dict of CPU numpy arrays (idx_xy, idx_yx, min_xy, min_yx, sums, out, gx, gy).  Every output starts as a value the kernels cannot
    produce, inside guard bands, and must come back fully written with the bands untouched; forward and backward run twice: the same
    bits both times.  grads: "both", "x" (gy_d NULL) or "y" (gx_d NULL)."""
    x, y = torch.as_tensor(np.asarray(x, np.float32)).to(device).contiguous(), torch.as_tensor(np.asarray(y, np.float32)).to(device).contiguous()
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    go = torch.tensor([gout], dtype=torch.float32, device=device)
    o = _Outs(device)
    runs = []
    for _ in range(2):
        r = dict(idx_xy=o.new((B, N), torch.int32, -1), idx_yx=o.new((B, M), torch.int32, -1),
                 min_xy=o.new((B, N), torch.float64, float("nan")), min_yx=o.new((B, M), torch.float64, float("nan")),
                 sums=o.new((B, 2), torch.float64, float("nan")), out=o.new((1,), torch.float32, float("nan")))
        ws = o.new((lib.chamfer_workspace_bytes(B, N, M) // 8,), torch.float64, float("nan"))
        r["gx"] = o.new((B, N, 3), torch.float32, float("nan")) if grads in ("both", "x") else None
        r["gy"] = o.new((B, M, 3), torch.float32, float("nan")) if grads in ("both", "y") else None
        lib.chamfer_fwd(x, y, w_xy, w_yx, r["idx_xy"], r["idx_yx"], r["min_xy"], r["min_yx"], r["sums"], r["out"], ws)
        lib.chamfer_bwd(x, y, r["idx_xy"], r["idx_yx"], go, w_xy, w_yx, r["gx"], r["gy"])
        runs.append(r)
    for k, a in runs[0].items():
        if a is None:
            continue
        if a.dtype == torch.int32:
            assert int(a.min()) >= 0, f"{k}: an element was not written"
        else:
            assert not bool(torch.isnan(a).any()), f"{k}: an element was not written"
        assert torch.equal(_bits(a), _bits(runs[1][k])), f"{k}: two calls differ in their bits"
    o.intact()
    return {k: (None if a is None else a.cpu().numpy()) for k, a in runs[0].items()}


def compare(tag, got, ref):
    """The module docstring's bounds; prints each figure before it asserts."""
    for k in ("idx_xy", "idx_yx"):
        bad = int((got[k] != ref[k]).sum())
        print(f"[chamfer] {tag}: {k}: {bad} of {got[k].size} indices differ")
        assert bad == 0, (tag, k, np.argwhere(got[k] != ref[k])[:4].tolist())
    for k in ("min_xy", "min_yx"):
        bad = int((got[k].view(np.int64) != ref[k].view(np.int64)).sum())
        print(f"[chamfer] {tag}: {k}: {bad} of {got[k].size} minima differ in their bits")
        assert bad == 0, (tag, k)
    es = float(np.max(np.abs(got["sums"] - ref["sums"]) / np.maximum(np.abs(ref["sums"]), 1e-300)))
    eo = abs(float(got["out"][0]) - ref["value"])
    print(f"[chamfer] {tag}: sums relative error {es:.2e} (bound 1e-12); out {float(got['out'][0]):.9e} ref {ref['value']:.9e} "
          f"error {eo:.2e} (bound {EPS32 * abs(ref['value']):.2e})")
    assert es <= 1e-12, (tag, es)
    assert eo <= EPS32 * abs(ref["value"]), (tag, eo, ref["value"])
    for k in ("gx", "gy"):
        if got.get(k) is None:
            continue
        r = ref[k]
        bound = EPS32 * np.abs(r) + 1e-10 * float(np.abs(r).max())
        err = np.abs(got[k].astype(np.float64) - r)
        print(f"[chamfer] {tag}: {k}: max error {float(err.max()):.2e}, max |ref| {float(np.abs(r).max()):.3e}, worst error / bound "
              f"{float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), (tag, k, float(err.max()))


def check(tag, lib, device, x, y, w=W, gout=GOUT):
    ref = cr.chamfer(x, y, w[0], w[1], gout)
    got = run_kernels(lib, device, x, y, w[0], w[1], gout)
    compare(tag, got, ref)
    return got, ref


# ---- known answers in exact arithmetic --------------------------------------------------------------------------------------------------
def lattice(n):
    """n^3 integer points, index = (ix n + iy) n + iz"""
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, n ** 3, 3).copy()


def known_answers_case(lib, device):
    # one point each: d2 = 1 + 4 + 4 = 9 both ways; value 18 at unit weights; gx = -gy = gout (2 (x - y) + 2 (x - y)) = 4 (-1, -2, -2) gout
    got = run_kernels(lib, device, [[[0.0, 0.0, 0.0]]], [[[1.0, 2.0, 2.0]]], 1.0, 1.0, gout=0.75)
    assert got["sums"].tolist() == [[9.0, 9.0]] and float(got["out"][0]) == 18.0 and got["min_xy"].tolist() == [[9.0]]
    assert got["idx_xy"].tolist() == [[0]] and got["idx_yx"].tolist() == [[0]]
    assert got["gx"].tolist() == [[[-3.0, -6.0, -6.0]]] and got["gy"].tolist() == [[[3.0, 6.0, 6.0]]], (got["gx"], got["gy"])
    # an integer lattice against itself (729 points: more than one workgroup of queries, more than one pass): value 0, a[i] = i, no gradient
    L = lattice(9)
    n = L.shape[1]
    got = run_kernels(lib, device, L, L, 1.0, 1.0)
    assert float(got["out"][0]) == 0.0 and not got["sums"].any() and not got["gx"].any() and not got["gy"].any()
    assert (got["idx_xy"][0] == np.arange(n)).all() and (got["idx_yx"][0] == np.arange(n)).all()
    # ... against a copy shifted by half a cell along x: x[i] has the partners (ix - 1, .) and (ix, .) at 0.25, 81 indices apart -- the LOWER
    # one, ix - 1, unless ix = 0; y[j] has (jx, .) and (jx + 1, .): the lower one is j itself.  All of it is exact
    S = L + np.asarray([0.5, 0.0, 0.0], np.float32)
    got, ref = check("lattice against its half-cell shift", lib, device, L, S, w=(1.0, 1.0))
    i = np.arange(n)
    assert (got["idx_xy"][0] == np.where(i >= 81, i - 81, i)).all() and (got["idx_yx"][0] == i).all()
    assert (got["min_xy"] == 0.25).all() and (got["min_yx"] == 0.25).all() and float(got["out"][0]) == 0.5


# ---- the boundaries of a workgroup's queries and of an LDS pass -----------------------------------------------------------------------
def boundary_case(lib, device, N, M, B=2):
    """Seeded points at one (N, M) of boundary_sizes: one direction always has surplus chunks.  Indices, minima, values and gradients."""
    x, y = seeded_points(B, N, M, seed=1000 * N + M)
    check(f"boundary B={B} N={N} M={M}", lib, device, x, y)


# ---- ties across passes and waves ------------------------------------------------------------------------------------------------------
def tie_layouts(lib):
    """(name, positions of the duplicated point in the searched set): across passes, at a pass boundary, and inside one pass at the first
    and last element of two different waves' shares."""
    _, t = geometry(lib)
    s = t // 4
    return [("0, T-1, T, 2T+1", [0, t - 1, t, 2 * t + 1]), ("T, T+3", [t, t + 3]), ("T-1, T", [t - 1, t]),
            ("first of share 1, last of share 2", [s, 3 * s - 1]), ("last of share 0, first of share 2", [s - 1, 2 * s]),
            ("last of share 1, first of share 3, second pass", [t + 2 * s - 1, t + 3 * s]), ("first of share 0, last of share 3", [0, t - 1])]


def tie_case(lib, device):
    """The searched set holds one point several times, the queries are nearest to it: every query reports the LOWEST of the positions, from
    whichever pass or wave the others come.  Both directions: the set is searched once as y (idx_xy) and once as x (idx_yx)."""
    q, t = geometry(lib)
    n_s, n_q = 2 * t + 5, q + 1
    g = torch.Generator().manual_seed(5)
    far = (torch.rand(1, n_s, 3, generator=g) + 2.0).numpy()                       # the rest of the searched set: the box [2, 3]^3
    p = np.asarray([0.25, -0.5, 0.125], np.float32)
    queries = (p + 0.01 * (torch.rand(1, n_q, 3, generator=g).numpy() - 0.5)).astype(np.float32)
    for name, pos in tie_layouts(lib):
        searched = far.copy()
        searched[0, pos] = p
        for tag, x, y, key in (("x searches y", queries, searched, "idx_xy"), ("y searches x", searched, queries, "idx_yx")):
            got, _ = check(f"ties at {name}, {tag}", lib, device, x, y)
            assert (got[key] == min(pos)).all(), (name, tag, np.unique(got[key]).tolist(), min(pos))


# ---- the sizes of the product -------------------------------------------------------------------------------------------------------------
def product_case(lib, device, B, N, M):
    x, y = seeded_points(B, N, M, seed=N + M)
    check(f"product B={B} N={N} M={M}", lib, device, x, y)


# ---- weights of exactly zero, NULL gradients ----------------------------------------------------------------------------------------------
def zero_weight_case(lib, device):
    q, t = geometry(lib)
    x, y = seeded_points(2, q + 1, t + 1, seed=11)
    full = run_kernels(lib, device, x, y, *W)
    for w in ((0.0, W[1]), (W[0], 0.0)):
        got, ref = check(f"weights {w}", lib, device, x, y, w=w)              # its index and min arrays are still written, and equal
        for k in ("idx_xy", "idx_yx", "min_xy", "min_yx", "sums"):
            assert (got[k] == full[k]).all(), (w, k)
    got = run_kernels(lib, device, x, y, 0.0, 0.0)
    assert float(got["out"][0]) == 0.0 and not got["gx"].any() and not got["gy"].any()
    assert (got["idx_xy"] == full["idx_xy"]).all() and (got["sums"] == full["sums"]).all()
    # one weight 0: the value is the other direction's alone -- the fp32 rounding of w times the mean of the sums the kernel itself wrote
    for k, w in ((1, (0.0, W[1])), (0, (W[0], 0.0))):
        o = float(run_kernels(lib, device, x, y, *w)["out"][0])
        want = float(np.float32(w[k])) * float(np.mean(full["sums"][:, k] / (x.shape[1] if k == 0 else y.shape[1])))
        assert abs(o - want) <= EPS32 * abs(want), (w, o, want)


def null_gradient_case(lib, device):
    """gx_d NULL, then gy_d NULL: the other gradient has the bits of the run with both."""
    q, t = geometry(lib)
    x, y = seeded_points(2, q + 1, t + 1, seed=12)
    both = run_kernels(lib, device, x, y, *W)
    only_x, only_y = run_kernels(lib, device, x, y, *W, grads="x"), run_kernels(lib, device, x, y, *W, grads="y")
    assert only_x["gy"] is None and only_y["gx"] is None
    assert (only_x["gx"].view(np.int32) == both["gx"].view(np.int32)).all() and (only_y["gy"].view(np.int32) == both["gy"].view(np.int32)).all()


# ---- the reference's own class ------------------------------------------------------------------------------------------------------------
def golden_case(lib, device, golden_dir):
    """tests/golden/chamfer.npz (tools/make_chamfer_golden.py): the reference's ChamferLoss()(preds = x, gts = y) in float64 on seeded
    sets, x [3, 37, 3], y [3, 53, 3].  sums_d / N = loss_1, sums_d / M = loss_2 within 1e-12 max(|x|^2, |y|^2): the reference expands
    |x|^2 + |y|^2 - 2 x.y, whose float64 cancellation error is a few ulp of that magnitude; the bound is three orders above it."""
    import os
    z = np.load(os.path.join(golden_dir, "chamfer.npz"))
    x, y = z["x"], z["y"]
    assert x.dtype == np.float32 and x.shape == (3, 37, 3) and y.shape == (3, 53, 3)
    got, _ = check("golden", lib, device, x, y, w=(1.0, 1.0))
    bound = 1e-12 * max(float((x.astype(np.float64) ** 2).sum(-1).max()), float((y.astype(np.float64) ** 2).sum(-1).max()))
    e1, e2 = np.abs(got["sums"][:, 0] / 37 - z["loss_1"]).max(), np.abs(got["sums"][:, 1] / 53 - z["loss_2"]).max()
    print(f"[chamfer] golden: loss_1 error {e1:.2e}, loss_2 error {e2:.2e}, bound {bound:.2e}")
    assert e1 <= bound and e2 <= bound, (e1, e2, bound)
    want = float(z["loss_1"].mean() + z["loss_2"].mean())
    assert abs(float(got["out"][0]) - want) <= EPS32 * abs(want) + bound


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
    B, N, M = 2, 5, 7
    xs, ys = seeded_points(B, N, M, seed=3)
    x, y = torch.as_tensor(xs).to(device), torch.as_tensor(ys).to(device)
    # the workspace size: 0 for what is refused, never decreasing with B
    sizes = [lib.chamfer_workspace_bytes(b, N, M) for b in range(6)]
    assert sizes[0] == 0 and sizes[1] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.chamfer_workspace_bytes(-1, N, M) == 0 and lib.chamfer_workspace_bytes(B, 0, M) == 0 and lib.chamfer_workspace_bytes(B, N, 0) == 0
    q, _ = geometry(lib)
    assert lib.chamfer_workspace_bytes(B, 2 * q + 1, 1) == B * 2 * 3 * 8
    sent = lambda shape, dtype: torch.full(shape, _CANARY[dtype], dtype=dtype, device=device)
    idx_xy, idx_yx = sent((B, N), torch.int32), sent((B, M), torch.int32)
    min_xy, min_yx, sums = sent((B, N), torch.float64), sent((B, M), torch.float64), sent((B, 2), torch.float64)
    out, ws = sent((1,), torch.float32), sent((sizes[B] // 8,), torch.float64)
    gx, gy = sent((B, N, 3), torch.float32), sent((B, M, 3), torch.float32)
    good_xy, good_yx = torch.zeros(B, N, dtype=torch.int32, device=device), torch.zeros(B, M, dtype=torch.int32, device=device)
    gout = torch.ones(1, device=device)
    big = 1 << 30                                                   # N = M = 1: one chunk, 2 B chunks = 2^31 > 2^31 - 1
    bad = [("B < 0", dict(B=-1)), ("N < 1", dict(N=0)), ("M < 1", dict(M=0)), ("N < 0", dict(N=-3)), ("grid past 2^31 - 1", dict(B=big, N=1, M=1)),
           ("w_xy NaN", dict(wx=float("nan"))), ("w_xy inf", dict(wx=float("inf"))), ("w_yx NaN", dict(wy=float("nan"))),
           ("w_yx -inf", dict(wy=float("-inf")))]
    outs_f = (idx_xy, idx_yx, min_xy, min_yx, sums, out, ws)
    base = dict(x=fp(x), y=fp(y), B=B, N=N, M=M, wx=0.7, wy=1.3, ixy=ip(idx_xy), iyx=ip(idx_yx), mxy=vp(min_xy), myx=vp(min_yx), sums=vp(sums),
                out=fp(out), ws=vp(ws))
    for what, change in [(f"{k} NULL", {k: None}) for k in ("x", "y", "ixy", "iyx", "mxy", "myx", "sums", "out", "ws")] + bad:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_chamfer_fwd", (a["x"], a["y"], a["B"], a["N"], a["M"], cf(a["wx"]), cf(a["wy"]), a["ixy"], a["iyx"], a["mxy"],
                                                      a["myx"], a["sums"], a["out"], a["ws"], None), outs_f, what)
    base = dict(x=fp(x), y=fp(y), ixy=ip(good_xy), iyx=ip(good_yx), gout=fp(gout), B=B, N=N, M=M, wx=0.7, wy=1.3, gx=fp(gx), gy=fp(gy))
    for what, change in [(f"{k} NULL", {k: None}) for k in ("x", "y", "ixy", "iyx", "gout")] + bad:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_chamfer_bwd", (a["x"], a["y"], a["ixy"], a["iyx"], a["gout"], a["B"], a["N"], a["M"], cf(a["wx"]), cf(a["wy"]),
                                                      a["gx"], a["gy"], None), (gx, gy), what)
    # accepted no-ops: B == 0, and a backward without a gradient to write: nothing launched, nothing written
    if device == "cpu":
        kc.launch_log(lib)
    b = base
    assert lib.c.hifihr_chamfer_fwd(fp(x), fp(y), 0, N, M, cf(0.7), cf(1.3), ip(idx_xy), ip(idx_yx), vp(min_xy), vp(min_yx), vp(sums), fp(out),
                                    vp(ws), None) == 0
    assert lib.c.hifihr_chamfer_bwd(b["x"], b["y"], b["ixy"], b["iyx"], b["gout"], 0, N, M, cf(0.7), cf(1.3), b["gx"], b["gy"], None) == 0
    assert lib.c.hifihr_chamfer_bwd(b["x"], b["y"], b["ixy"], b["iyx"], b["gout"], B, N, M, cf(0.7), cf(1.3), None, None, None) == 0
    if device == "cpu":
        assert not kc.launch_log(lib)
    else:
        torch.cuda.synchronize()
    for t in outs_f + (gx, gy):
        assert bool((t == _CANARY[t.dtype]).all())
    null = ctypes.POINTER(ctypes.c_int32)()
    lib.c.hifihr_chamfer_geometry(null, null)                       # either pointer may be NULL
