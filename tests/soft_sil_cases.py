"""Shared bodies of the soft-silhouette tests (hifihr_soft_sil_fwd / _bwd, hifihr_soft_sil_loss_fwd / _bwd, csrc/soft_sil.hip):
tests/test_hostsim_soft_silhouette.py runs them on the emulator (device='cpu'), tests/test_gpu_soft_silhouette.py on the MI355X
(device='cuda').  The reference is the float64 restatement of tests/soft_sil_ref.py on the fp32-rounded inputs.

Conditions on the inputs, asserted from the restatement alone:
  * participation gap: every (pixel, face) pair that is not inside has |dist - blur| >= 5e-5 blur, so fp32 and fp64 agree on which faces
    participate (a flip moves S by softplus(-blur / sigma), 1.0e-4 at the default blur: twice the bound on alpha).  A seed that fails it
    is replaced, the gap is never relaxed.  No condition on nearest-edge ties: the value is continuous there and the gradient bounds are
    norm-wise.
  * admission (the renderer contract's RENDER_ADMIT = 0.5 rule): the restatement evaluated in plain float32 stays within HALF of every
    bound, so a bound never passes on luck; a case that breaks it is changed, not the bound.
Bounds (about ten times the float32 restatement's own error -- the kernel rounds in another order, in the same precision):
  alpha 5e-5 absolute; neglog 5e-5 max(1, S_ref); gradients 1e-4 max|g_ref| element-wise and 1e-4 relative L2."""
import ctypes
import math

import numpy as np
import torch

import kernel_cases as kc
import soft_sil_ref as sr

EINVAL = -1
ALPHA_ATOL, NEGLOG_RTOL, GRAD_TOL, ADMIT = 5e-5, 5e-5, 1e-4, 0.5
TILE = 16
LIST = 256          # kSoftList of csrc/soft_sil.hip: the faces the tile's LDS list holds (= the faces tested per pass)
CAM = (-4.5, -4.5, 0.05, -0.03)

# (H, B, F, sigma, kind, seed).  H around the tile edge 16, F around the 256-face chunk, both sigma.  kind: "mesh" = the generator of the
# issue (V = 40, faces = random vertex triples); "soup" = F small triangles with vertices of their own (plus unreferenced ones), so that
# hundreds of faces leave partial coverage; "shift" = mesh with the principal point moved by one NDC unit: half of it off screen;
# "zero_tile" = mesh with galpha zero on the whole tile (0, 0); "stack" = LIST + 1 faces over the ONE tile of a 16-pixel image.
# The seeds are the first ones that meet the two conditions above and leave the case neither empty nor saturated: searched on the CPU with
# the restatement alone, before the kernel ran on them.
RANDOM_CASES = [
    (1, 1, 1, 1e-4, "mesh", 8), (15, 3, 60, 1e-3, "mesh", 1), (16, 1, 256, 1e-4, "soup", 0), (17, 3, 257, 1e-3, "soup", 1),
    (33, 1, 600, 1e-4, "soup", 0), (33, 3, 60, 1e-4, "mesh", 0), (32, 2, 60, 1e-3, "mesh", 1), (33, 2, 60, 1e-3, "shift", 0),
    (33, 2, 60, 1e-4, "zero_tile", 0), (16, 1, LIST + 1, 1e-3, "stack", 1),
]
MANO_SEED = {64: 0}          # make_render_inputs seeds whose B = 2 hands meet the gap at that size


def f32(x):
    return float(np.float32(x))


def make_inputs(H, B, F, kind, seed):
    torch.manual_seed(seed)
    cam = torch.tensor([CAM]).repeat(B, 1)
    if kind in ("soup", "stack"):
        spread, size, extra = (0.03, 0.02, 3) if kind == "stack" else (0.08, 0.015, 5)
        centre = spread * torch.randn(B, F, 1, 2)
        tri = torch.cat([centre + size * torch.randn(B, F, 3, 2), 0.6 + 0.05 * torch.randn(B, F, 3, 1)], -1).reshape(B, 3 * F, 3)
        verts = torch.cat([tri, torch.cat([0.08 * torch.randn(B, extra, 2), 0.6 + 0.05 * torch.randn(B, extra, 1)], -1)], 1)
        perm = torch.randperm(3 * F + extra)                      # vertex v of the soup is stored at row perm[v]
        stored = torch.empty_like(verts)
        stored[:, perm] = verts
        faces = perm[torch.arange(3 * F).view(F, 3)]
        verts = stored
    else:
        V = 40
        verts = torch.cat([0.08 * torch.randn(B, V, 2), 0.6 + 0.05 * torch.randn(B, V, 1)], -1)
        faces = torch.stack([torch.randperm(V)[:3] for _ in range(F)])
        if kind == "shift":
            cam[:, 2] += 1.0
    w = torch.randn(B, H, H)
    if kind == "zero_tile":
        w[:, :TILE, :TILE] = 0.0
    return verts.contiguous(), faces.contiguous(), cam, w


class Renderer:
    """A renderer handle for (faces, V, H): the soft-silhouette entries reuse its device-side faces, V, F and image_size."""

    def __init__(self, lib, faces, V, H):
        self.lib, self.H, self.V = lib, H, V
        self.h = lib.renderer_create(np.ascontiguousarray(torch.as_tensor(faces).numpy(), dtype=np.int32), V, image_size=H, aa=1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.renderer_destroy(self.h)


def run_kernels(lib, device, r, verts, cam, sigma, blur, galpha=None):
    """-> (alpha [B,H,H], neglog [B,H,H], gverts [B,V,3] or None) as float64 CPU tensors.  Every output starts as NaN inside guard bands
    and must come back fully written with the bands untouched; the forward runs twice: the same bits both times."""
    B, H, V = verts.shape[0], r.H, r.V
    g = kc.Guards(device)
    v, c = g.inp(verts), g.inp(cam)
    ws = g.out(lib.soft_sil_workspace_bytes(r.h, B), dtype=torch.uint8)
    outs = []
    for _ in range(2):
        alpha, neglog = g.out(B, H, H, fill=float("nan")), g.out(B, H, H, fill=float("nan"))
        lib.soft_sil_fwd(r.h, v, c, sigma, blur, alpha, neglog, ws)
        outs.append((alpha, neglog))
    for a, b, name in ((outs[0][0], outs[1][0], "alpha"), (outs[0][1], outs[1][1], "neglog")):
        assert not bool(torch.isnan(a).any()), f"{name}: an element was not written"
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: two calls differ in their bits"
    gverts = None
    if galpha is not None:
        gverts = g.out(B, V, 3, fill=float("nan"))
        lib.soft_sil_bwd(r.h, v, c, outs[0][1], g.inp(galpha.float()), sigma, blur, gverts, ws)
        assert not bool(torch.isnan(gverts).any()), "gverts: an element was not overwritten"
    g.intact("soft silhouette")
    return outs[0][0].double().cpu(), outs[0][1].double().cpu(), None if gverts is None else gverts.double().cpu()


def errors(alpha, neglog, gverts, ref):
    """The four figures the bounds are on, each as observed / bound."""
    e = {"alpha": float((alpha - ref["alpha"]).abs().max()) / ALPHA_ATOL,
         "neglog": float(((neglog - ref["S"]).abs() / ref["S"].clamp(min=1.0)).max()) / NEGLOG_RTOL}
    if gverts is not None:
        gr = ref["gverts"]
        gmax, gnorm = float(gr.abs().max()), float(gr.norm())
        e["grad_max"] = (float((gverts - gr).abs().max()) / gmax if gmax > 0 else float(gverts.abs().max())) / GRAD_TOL
        e["grad_l2"] = (float((gverts - gr).norm()) / gnorm if gnorm > 0 else float(gverts.norm())) / GRAD_TOL
    return e


def check_against_restatement(tag, lib, device, verts, faces, cam, w, H, sigma, ref_device="cpu", strict_gap=True, windowed=False):
    """ref_device: where the float64 restatement runs.  The float32 restatement of the admission rule ALWAYS runs on the CPU: torch's
    float32 on the GPU is a worse yardstick (its division is not correctly rounded, exp / log1p are approximations) -- on the 224-pixel
    MANO case it uses 0.52 .. 0.77 of the neglog bound where the CPU's float32 uses 0.29 .. 0.37."""
    sigma32, blur32 = f32(sigma), f32(sr.default_blur(sigma))
    ref = sr.soft_silhouette(verts, faces, cam, H, sigma32, blur32, w=w, device=ref_device, w_skips_near=not strict_gap, windowed=windowed)
    r32 = sr.soft_silhouette(verts, faces, cam, H, sigma32, blur32, w=ref["w"], dtype=torch.float32, device="cpu", windowed=windowed)
    ref = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ref.items()}
    n_near = int((ref["near"] > 0).sum())
    print(f"[soft_sil] {tag}: gap {ref['gap']:.3e}, pixels with a near pair {n_near}, coverage {float(ref['alpha'].mean()):.3f}, "
          f"max|g_ref| {float(ref['gverts'].abs().max()):.3e}")
    if strict_gap:
        assert ref["gap"] >= sr.GAP, f"{tag}: a distance sits within {sr.GAP} of blur_radius ({ref['gap']:.3e}): take another seed"
    keep = ref["near"] == 0                                    # all of them under strict_gap
    if not strict_gap:
        # see mano_case: such a pixel may flip one face per near pair, each worth softplus(-blur (1 - GAP) / sigma); its galpha is zero
        assert n_near <= 1e-3 * keep.numel(), (n_near, keep.numel())
    admit = errors(torch.where(keep, r32["alpha"].double().cpu(), ref["alpha"]), torch.where(keep, r32["S"].double().cpu(), ref["S"]),
                   r32["gverts"].double().cpu(), ref)
    print(f"[soft_sil] {tag}: float32 restatement / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in admit.items()))
    assert max(admit.values()) <= ADMIT, f"{tag}: the float32 restatement uses more than half of a bound {admit}: change the case"
    with Renderer(lib, faces, verts.shape[1], H) as r:
        alpha, neglog, gverts = run_kernels(lib, device, r, verts, cam, sigma, sr.default_blur(sigma), galpha=ref["w"])
    got = errors(torch.where(keep, alpha, ref["alpha"]), torch.where(keep, neglog, ref["S"]), gverts, ref)
    print(f"[soft_sil] {tag}: kernel / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in got.items()))
    assert got["alpha"] <= 1.0 and got["neglog"] <= 1.0 and got["grad_max"] <= 1.0 and got["grad_l2"] <= 1.0, (tag, got)
    if not strict_gap and n_near:
        flip = math.log1p(math.exp(-blur32 * (1.0 - sr.GAP) / sigma32))
        slack = ALPHA_ATOL + ref["near"].double() * flip
        assert bool(((alpha - ref["alpha"]).abs() <= slack).all()) and bool(((neglog - ref["S"]).abs() <= slack * ref["S"].clamp(min=1.0)).all())
    assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    used = torch.zeros(verts.shape[1], dtype=torch.bool)
    used[torch.as_tensor(faces).reshape(-1).long()] = True
    assert not bool(gverts[:, ~used].any()), "an unreferenced vertex has a gradient"
    return ref, alpha, gverts


def random_case(lib, device, H, B, F, sigma, kind, seed):
    verts, faces, cam, w = make_inputs(H, B, F, kind, seed)
    ref, alpha, gverts = check_against_restatement(f"{kind} H={H} B={B} F={F} sigma={sigma:g} seed={seed}", lib, device, verts, faces, cam, w, H, sigma)
    assert float(ref["alpha"].max()) > 0.0, "the case covers no pixel"
    if H > 1:
        assert 0.02 < float(ref["alpha"].mean()) < 0.98 and float(ref["gverts"].abs().max()) > 0.0, "the case is all or nothing: it would not see a wrong face"
    if kind in ("soup", "stack"):
        assert verts.shape[1] > 3 * F                              # rows of unreferenced vertices exist (checked to be 0 above)
    if kind == "stack":
        assert int(ref["faces_hit"].min()) >= LIST + 1, "fewer faces over the one tile than its list holds, plus one"
    if kind == "shift":
        ndc_x = (verts[..., 0] * cam[:, :1] + verts[..., 2] * cam[:, 2:3]) / verts[..., 2]
        assert 0.25 < float((ndc_x.abs() > 1).float().mean()) < 0.75, "about half of the mesh is meant to be off screen"


def mano_case(lib, device, tables, H, B=2, seed=0, ref_device="cpu"):
    """The MANO topology (778 vertices, 1538 faces: seven passes of the list) posed in front of a FreiHAND-like camera, B = 2, the default
    sigma = 1e-4 and blur radius.
    H = 64: seed 0 meets the participation gap on every pair.
    H = 224 (the GPU only; the size and sigma the model runs at): no seed can.  A hand has about 1.4e5 (pixel, face) pairs per unit of
    relative distance at the blur radius (the gaps of 20 seeds lie between 5e-7 and 2e-5), so a seed passes 5e-5 with probability exp(-7).
    The gap itself is not relaxed: the pixels that own a pair inside it are named from the float64 restatement alone (about ten of
    100 352, at most 0.1 % is asserted), get galpha = 0, are left out of the alpha / neglog bounds and are held instead to the bound plus
    one face flip, softplus(-blur (1 - 5e-5) / sigma), per near pair; every other pixel and the whole gradient are held to the bounds as
    everywhere else.  The restatements walk each chunk of faces on the pixel window it can reach (soft_sil_ref `windowed`); admission of
    seed 0 (float32 on the CPU): neglog 0.36, alpha 0.14, gradient 0.10 of their bounds."""
    strict = H in MANO_SEED
    assert not strict or seed == MANO_SEED[H]
    verts, _, cam, _, _ = kc.make_render_inputs(tables, B, seed, H)
    faces = torch.as_tensor(np.asarray(tables.faces)).long()
    w = torch.randn(B, H, H, generator=torch.Generator().manual_seed(seed + 100))
    ref, alpha, _ = check_against_restatement(f"mano H={H} B={B} seed={seed}", lib, device, verts.contiguous(), faces, cam.contiguous(), w, H, 1e-4,
                                              ref_device=ref_device, strict_gap=strict, windowed=not strict)
    assert 0.02 < float(ref["alpha"].mean()) < 0.5 and int(ref["faces_hit"].min()) > 300


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def _pixel_of(c, H):
    """(yi, xi) of the pixel whose centre is NDC (cx, cy): centre = pix_to_ndc(H - 1 - index, H)."""
    i = [(v + 1.0) * H / 2.0 - 0.5 for v in c]
    assert all(abs(v - round(v)) < 1e-12 for v in i)
    return H - 1 - int(round(i[1])), H - 1 - int(round(i[0]))


def _sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x))


def known_answers_case(lib, device):
    """Z = 1, cam = (1, 1, 0, 0) (NDC = X, Y), H = 4 (centres at +-0.25, +-0.75), dyadic coordinates: every expected value is the closed
    form in float64.  Triangle T1 = (-0.5, -0.625), (0.875, -0.625), (-0.5, 0.75) (hypotenuse x + y = 0.25) in both windings."""
    H, sigma = 4, 0.05
    cam = torch.tensor([[1.0, 1.0, 0.0, 0.0]])
    T1 = [(-0.5, -0.625), (0.875, -0.625), (-0.5, 0.75)]
    T2 = [(-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0)]                # hypotenuse x + y = 0
    tri = lambda pts, z=(1.0, 1.0, 1.0): [[x * zz, y * zz, zz] for (x, y), zz in zip(pts, z)]

    def alpha_of(vert_rows, faces, blur, galpha=None):
        verts = torch.tensor([vert_rows], dtype=torch.float32)
        with Renderer(lib, torch.tensor(faces), verts.shape[1], H) as r:
            return run_kernels(lib, device, r, verts, cam, sigma, blur, galpha=galpha)

    inside, edge, vertex, far = _pixel_of((-0.25, -0.25), H), _pixel_of((-0.75, -0.25), H), _pixel_of((-0.75, -0.75), H), _pixel_of((0.75, 0.75), H)
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):
        a, s, _ = alpha_of(tri(T1), faces, 0.1)
        # inside, 0.25 from the nearest edge x = -0.5 (0.375 from y = -0.625, 0.53 from the hypotenuse): sigmoid(h^2 / sigma)
        assert abs(float(a[0][inside]) - _sigmoid(0.0625 / sigma)) <= ALPHA_ATOL
        assert abs(float(s[0][inside]) - math.log1p(math.exp(0.0625 / sigma))) <= NEGLOG_RTOL * math.log1p(math.exp(0.0625 / sigma))
        # outside, nearest to the interior of the edge x = -0.5 at (-0.5, -0.25): dist = 0.0625 < blur
        assert abs(float(a[0][edge]) - _sigmoid(-0.0625 / sigma)) <= ALPHA_ATOL
        # outside, nearest to the vertex (-0.5, -0.625): dist = 0.0625 + 0.015625 < blur
        assert abs(float(a[0][vertex]) - _sigmoid(-0.078125 / sigma)) <= ALPHA_ATOL
        # beyond the blur radius (1.25^2 / 2 from the hypotenuse): exactly 0
        assert float(a[0][far]) == 0.0 and float(s[0][far]) == 0.0
        # blur_radius = 0: inside faces only
        a0, _, _ = alpha_of(tri(T1), faces, 0.0)
        assert abs(float(a0[0][inside]) - _sigmoid(0.0625 / sigma)) <= ALPHA_ATOL
        assert float(a0[0][edge]) == 0.0 and float(a0[0][vertex]) == 0.0 and float(a0[0][far]) == 0.0
        ref0 = sr.soft_silhouette(torch.tensor([tri(T1)]), faces, cam, H, sigma, 0.0)
        assert float((a0 - ref0["alpha"]).abs().max()) <= ALPHA_ATOL and int((a0 > 0).sum()) == int((ref0["alpha"] > 0).sum())
    # two overlapping triangles: 1 - (1 - p1)(1 - p2); the centre is 0.5 / sqrt(2) from T2's hypotenuse, 0.75 from its legs
    a, _, _ = alpha_of(tri(T1) + tri(T2), [[0, 1, 2], [3, 4, 5]], 0.1)
    p1, p2 = _sigmoid(0.0625 / sigma), _sigmoid(0.125 / sigma)
    assert abs(float(a[0][inside]) - (1.0 - (1.0 - p1) * (1.0 - p2))) <= ALPHA_ATOL
    # a zero-area face (three collinear dyadic points: the area is exactly 0): exactly 0 everywhere
    a, s, g = alpha_of(tri([(-0.5, -0.5), (0.0, 0.0), (0.5, 0.5)]), [[0, 1, 2]], 0.1, galpha=torch.ones(1, H, H))
    assert not bool(a.any()) and not bool(s.any()) and not bool(g.any())
    # a face with one vertex behind the camera plane: exactly 0 everywhere, zero gradient
    a, s, g = alpha_of(tri(T1, z=(1.0, -1.0, 1.0)), [[0, 1, 2]], 0.1, galpha=torch.ones(1, H, H))
    assert not bool(a.any()) and not bool(s.any()) and not bool(g.any())
    # ... and it does not disturb the face next to it
    a, _, g = alpha_of(tri(T1, z=(1.0, -1.0, 1.0)) + tri(T1), [[0, 1, 2], [3, 4, 5]], 0.1, galpha=torch.ones(1, H, H))
    assert abs(float(a[0][inside]) - p1) <= ALPHA_ATOL and not bool(g[0, :3].any()) and bool(g[0, 3:].any())


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def buffers_case(lib, device):
    """What run_kernels asserts on every call (NaN-prefilled outputs fully written, guard bands around outputs and workspace untouched,
    two forwards bit-identical, gverts overwritten), on a case with unreferenced vertices and a ragged last tile; plus: the backward needs
    nothing the forward left in the workspace (a fresh, poisoned one gives the same gradient to rounding)."""
    H, B, F, sigma = 17, 2, 70, 1e-3
    verts, faces, cam, w = make_inputs(H, B, F, "soup", 3)
    blur = sr.default_blur(sigma)
    with Renderer(lib, faces, verts.shape[1], H) as r:
        alpha, neglog, g1 = run_kernels(lib, device, r, verts, cam, sigma, blur, galpha=w)
        g = kc.Guards(device)
        ws = g.out(lib.soft_sil_workspace_bytes(r.h, B), dtype=torch.uint8, fill=0xFF)
        g2 = g.out(B, verts.shape[1], 3, fill=float("nan"))
        lib.soft_sil_bwd(r.h, verts.to(device), cam.to(device), neglog.float().to(device), w.to(device), sigma, blur, g2, ws)
        g.intact("soft_sil_bwd on a fresh workspace")
    assert float((g2.double().cpu() - g1).abs().max()) <= 1e-5 * float(g1.abs().max()) and float(g1.abs().max()) > 0
    used = torch.zeros(verts.shape[1], dtype=torch.bool)
    used[faces.reshape(-1)] = True
    assert int((~used).sum()) == 5 and not bool(g1[:, ~used].any()) and not bool(g2.cpu()[:, ~used].any())


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
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
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    cf = ctypes.c_float
    H, B, F, sigma = 5, 2, 4, 1e-3
    blur = sr.default_blur(sigma)
    verts, faces, cam, w = make_inputs(H, B, F, "mesh", 0)
    V = verts.shape[1]
    verts, cam, w = verts.to(device), cam.to(device), w.to(device)
    bad_params = [("sigma = 0", dict(sigma=0.0)), ("sigma < 0", dict(sigma=-1e-4)), ("sigma NaN", dict(sigma=float("nan"))),
                  ("sigma inf", dict(sigma=float("inf"))), ("blur < 0", dict(blur=-1e-6)), ("blur NaN", dict(blur=float("nan"))),
                  ("blur inf", dict(blur=float("inf"))), ("B < 0", dict(B=-1))]
    with Renderer(lib, faces, V, H) as r:
        n = [lib.soft_sil_workspace_bytes(r.h, b) for b in range(5)]
        assert n[0] == 0 and all(a <= b for a, b in zip(n, n[1:])) and n[1] > 0, n               # never decreases with B
        assert lib.soft_sil_workspace_bytes(None, 2) == 0 and lib.soft_sil_workspace_bytes(r.h, -1) == 0
        fill = lambda *s: torch.full(s, -1234.5, device=device)
        alpha, neglog, gverts = fill(B, H, H), fill(B, H, H), fill(B, V, 3)
        ws = torch.full((n[B],), 0xA5, dtype=torch.uint8, device=device)
        good_s = fill(B, H, H).fill_(0.3)
        base = dict(h=r.h, verts=fp(verts), cam=fp(cam), B=B, sigma=sigma, blur=blur, alpha=fp(alpha), neglog=fp(neglog), ws=vp(ws))
        cases = [(f"{k} NULL", {k: None}) for k in ("h", "verts", "cam", "alpha", "neglog", "ws")] + bad_params
        for what, change in cases:
            a = dict(base, **change)
            _refused(lib, device, "hifihr_soft_sil_fwd", (a["h"], a["verts"], a["cam"], a["B"], cf(a["sigma"]), cf(a["blur"]), a["alpha"], a["neglog"],
                                                          a["ws"], None), (alpha, neglog, ws), what)
        base = dict(h=r.h, verts=fp(verts), cam=fp(cam), neglog=fp(good_s), galpha=fp(w), B=B, sigma=sigma, blur=blur, gverts=fp(gverts), ws=vp(ws))
        cases = [(f"{k} NULL", {k: None}) for k in ("h", "verts", "cam", "neglog", "galpha", "gverts", "ws")] + bad_params
        for what, change in cases:
            a = dict(base, **change)
            _refused(lib, device, "hifihr_soft_sil_bwd", (a["h"], a["verts"], a["cam"], a["neglog"], a["galpha"], a["B"], cf(a["sigma"]), cf(a["blur"]),
                                                          a["gverts"], a["ws"], None), (gverts, ws), what)
        # B == 0: accepted, nothing launched, nothing written
        before = [t.clone() for t in (alpha, neglog, gverts, ws)]
        if device == "cpu":
            kc.launch_log(lib)
        assert lib.c.hifihr_soft_sil_fwd(r.h, fp(verts), fp(cam), 0, cf(sigma), cf(blur), fp(alpha), fp(neglog), vp(ws), None) == 0
        assert lib.c.hifihr_soft_sil_bwd(r.h, fp(verts), fp(cam), fp(good_s), fp(w), 0, cf(sigma), cf(blur), fp(gverts), vp(ws), None) == 0
        if device == "cpu":
            assert not kc.launch_log(lib)
        else:
            torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((alpha, neglog, gverts, ws), before))
        lib.soft_sil_fwd(r.h, verts, cam, sigma, 0.0, alpha, neglog, ws)                           # blur_radius = 0 itself is accepted
    # the loss pair
    HW = H * H
    A, M = torch.rand(B, HW, device=device), (torch.rand(B, HW, device=device) > 0.5).float()
    sums = torch.full((B, 3), -3e300, dtype=torch.float64, device=device)
    out, gA, gout = torch.full((2,), -1234.5, device=device), torch.full((B, HW), -1234.5, device=device), torch.ones(2, device=device)
    base = dict(A=fp(A), M=vp(M), kind=0, B=B, HW=HW, sums=vp(sums), out=fp(out))
    cases = [(f"{k} NULL", {k: None}) for k in ("A", "M", "sums", "out")] + [("B < 0", dict(B=-1)), ("HW = 0", dict(HW=0)), ("HW < 0", dict(HW=-3)),
                                                                              ("mask kind 2", dict(kind=2)), ("mask kind -1", dict(kind=-1))]
    for what, change in cases:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_soft_sil_loss_fwd", (a["A"], a["M"], a["kind"], a["B"], a["HW"], cf(1.0), cf(1.0), a["sums"], a["out"], None), (sums, out), what)
    good_sums = torch.ones(B, 3, dtype=torch.float64, device=device)
    base = dict(A=fp(A), M=vp(M), kind=0, sums=vp(good_sums), gout=fp(gout), B=B, HW=HW, gA=fp(gA))
    cases = [(f"{k} NULL", {k: None}) for k in ("A", "M", "sums", "gout", "gA")] + [("B < 0", dict(B=-1)), ("B = 65536", dict(B=65536)), ("HW = 0", dict(HW=0)),
                                                                                     ("mask kind 2", dict(kind=2))]
    for what, change in cases:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_soft_sil_loss_bwd", (a["A"], a["M"], a["kind"], a["sums"], a["gout"], a["B"], a["HW"], cf(1.0), cf(1.0), a["gA"], None),
                 (gA,), what)
    if device == "cpu":
        kc.launch_log(lib)
    assert lib.c.hifihr_soft_sil_loss_fwd(fp(A), vp(M), 0, 0, HW, cf(1.0), cf(1.0), vp(sums), fp(out), None) == 0
    assert lib.c.hifihr_soft_sil_loss_bwd(fp(A), vp(M), 0, vp(good_sums), fp(gout), 0, HW, cf(1.0), cf(1.0), fp(gA), None) == 0
    if device == "cpu":
        assert not kc.launch_log(lib)
    else:
        torch.cuda.synchronize()
    assert bool((out == -1234.5).all()) and bool((gA == -1234.5).all()) and bool((sums == -3e300).all())


# ---- losses -------------------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = [(1, 16), (3, 16), (1, 33), (3, 33)]          # (B, H)


def _run_losses(lib, device, A, M, lam_s, lam_i, gout):
    """-> (out [2], sums [B,3], gA) on the CPU; the forward runs twice on garbage-filled outputs: the same bits."""
    B = A.shape[0]
    a, m = A.to(device).contiguous(), M.to(device).contiguous()
    res = []
    for fill in (-3e300, 7e200):
        sums = torch.full((B, 3), fill, dtype=torch.float64, device=device)
        out = torch.full((2,), float("nan"), device=device)
        lib.soft_sil_loss_fwd(a, m, lam_s, lam_i, sums, out)
        res.append((out, sums))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) or bool(torch.isnan(res[0][0]).any()), "out: two calls differ in their bits"
    assert torch.equal(res[0][1].view(torch.int64), res[1][1].view(torch.int64)), "sums: two calls differ in their bits"
    gA = torch.full_like(a, float("nan"))
    lib.soft_sil_loss_bwd(a, m, res[0][1], gout.to(device), lam_s, lam_i, gA)
    return res[0][0].cpu(), res[0][1].cpu(), gA.cpu()


def losses_case(lib, device, B, H, mask_dtype=torch.int64):
    """Forward and backward against the float64 formulas, to 1e-6 relative (the sums are fp64; the outputs round once to fp32, 6e-8).
    The gradient is compared against the norm of its reference: an element near a sign change of its two parts has no relative digits."""
    gen = torch.Generator().manual_seed(10 * B + H)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
    M = torch.stack([((yy - H * (0.4 + 0.1 * b)) ** 2 + (xx - H * 0.5) ** 2 < (0.3 * H) ** 2) for b in range(B)]).to(mask_dtype)
    A = (0.8 * M.float() * torch.rand(B, H, H, generator=gen) + 0.3 * torch.rand(B, H, H, generator=gen)).clamp(0, 1)
    A[:, 0, 0] = M[:, 0, 0].float()                                # |A - M| has gradient 0 where they are equal
    A = A.view(B, 1, H, H).contiguous()
    lam_s, lam_i = 0.005, 1e-3
    gout = torch.tensor([0.7, -1.3])
    out, sums, gA = _run_losses(lib, device, A, M, lam_s, lam_i, gout)
    Ar = A.double().requires_grad_(True)
    ref = sr.losses(Ar, M, f32(lam_s), f32(lam_i))
    (ref * gout.double()).sum().backward()
    rel = ((out.double() - ref.detach()).abs() / ref.detach().abs()).tolist()
    gerr = float((gA.double() - Ar.grad).abs().max()) / float(Ar.grad.abs().max())
    print(f"[soft_sil] losses B={B} H={H}: out {out.tolist()} relative error {rel}, gradient error / max|g| {gerr:.2e}")
    assert max(rel) <= 1e-6 and gerr <= 1e-6
    # a term with weight 0 is exactly 0 and contributes no gradient; the other is unchanged
    o2, _, g2 = _run_losses(lib, device, A, M, lam_s, 0.0, gout)
    assert float(o2[1]) == 0.0 and torch.equal(o2[0], out[0])
    o3, _, g3 = _run_losses(lib, device, A, M, 0.0, lam_i, gout)
    assert float(o3[0]) == 0.0 and torch.equal(o3[1], out[1])
    assert float((g2 + g3 - gA).abs().max()) <= 1e-6 * float(gA.abs().max())
    assert torch.equal(gA[:, 0, 0, 0], g3[:, 0, 0, 0]) and not bool(g2[:, 0, 0, 0].any())       # A == M there: no L1 part


def losses_nan_case(lib, device):
    """An image with an empty mask and zero alpha: U_b = 0 and the IoU term is NaN, exactly as hifihr_amd.losses.iou gives it."""
    from hifihr_amd.losses import iou
    B, H = 2, 16
    A, M = torch.rand(B, 1, H, H), (torch.rand(B, H, H) > 0.5).float()
    A[1], M[1] = 0.0, 0.0
    assert bool(torch.isnan(iou(M.unsqueeze(1), A)))
    out, _, _ = _run_losses(lib, device, A, M, 0.005, 1e-3, torch.ones(2))
    assert bool(torch.isnan(out[1])) and abs(float(out[0]) - 0.005 * float((A.double() - M.unsqueeze(1).double()).abs().mean())) <= 1e-6 * float(out[0])


KERNELS = {"soft_sil_vertex_kernel", "soft_sil_fwd_kernel", "soft_sil_bwd_kernel", "soft_sil_proj_bwd_kernel", "soft_sil_loss_sums_kernel",
           "soft_sil_loss_finish_kernel", "soft_sil_loss_bwd_kernel"}
