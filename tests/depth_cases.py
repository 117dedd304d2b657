"""Shared bodies of the depth-map tests (hifihr_render_depth_fwd / _bwd, hifihr_depth_loss_fwd / _bwd, csrc/depth.hip):
tests/test_hostsim_depth.py runs them on the emulator (device='cpu'), tests/test_gpu_depth.py on the MI355X (device='cuda').
The references are the restatements of tests/depth_ref.py and oracle/raster_oracle.c.

Sizes: image_size 8 (exactly one 8-pixel tile of the backward), 9 and 17 (a ragged last tile), 16 (two full tiles), aa = 1, 2, 3; B <= 2.
Bounds:
  * forward: bit for bit (aa = 1 against the C rasteriser's zbuf, aa > 1 against the float32 restatement with the same summation order);
  * gradient: GRAD_FACTOR times the error of the float32 restatement (autograd, CPU) on the same case, both against float64.  The factor is
    8 over the worst kernel / float32-restatement ratio measured by tools/depth_precision.py (profiles/depth_precision.txt): the 8 covers
    the summation-order freedom of the atomics, which one run does not sample.  The yardstick is the float32 restatement, never the kernel.
  * loss: sums bit for bit against the ordered float64 restatement, out to 1 ulp of fp32, gdepth exact by formula."""
import ctypes
import json
import os

import numpy as np
import torch

import depth_ref as dr
import kernel_cases as kc

EINVAL = -1
# worst kernel / float32-restatement ratio of the gradient error over GRAD_CASES, measured on an MI355X (profiles/depth_precision.txt: 1.573,
# the 8 x 8, aa = 1 case), and the factor of 8 over it
GRAD_WORST_RATIO = 1.573
GRAD_FACTOR = 8.0 * GRAD_WORST_RATIO
SIZES = [(H, aa) for H in (8, 9, 16, 17) for aa in (1, 2, 3)]
KINDS = ["single", "tie", "straddle", "behind", "zero_area"]
UNIT_CAM = (1.0, 1.0, 0.0, 0.0)         # NDC = (X / Z, Y / Z)


def _golden(name):
    cases = json.load(open(os.path.join(kc.REPO, "tests", "golden", "raster_known.json")))["cases"]
    return next(c for c in cases if c["name"] == name)


def scene(kind):
    """-> (verts [1,V,3] float32, faces [F,3], cam [1,4]).  The degenerate geometries are those of tests/golden/raster_known.json."""
    cam = torch.tensor([UNIT_CAM])
    if kind == "single":                         # non-dyadic corners, a depth gradient across the face
        pts, z = [(-0.71, -0.63), (0.83, -0.37), (-0.29, 0.77)], (0.53, 0.91, 0.67)
        verts, faces = [[x * zz, y * zz, zz] for (x, y), zz in zip(pts, z)], [[0, 1, 2]]
    elif kind == "tie":                          # two overlapping faces in the plane Z = 1 (every sample of the overlap ties: the lower index wins)
        c = _golden("equal_depth_lower_index_wins")
        verts, faces = c["verts_cam"], c["faces"]
    elif kind == "straddle":                     # one vertex behind the camera plane: rasterised per sample (pz >= 0)
        c = _golden("straddling_face_opposite_wedge")
        verts, faces = c["verts_cam"], c["faces"]
    elif kind == "behind":                       # a face wholly behind the camera (dropped) next to a visible one
        c = _golden("two_vertices_behind_camera")
        back = [[0.3, 0.2, -1.0], [-0.4, 0.1, -0.8], [0.1, -0.5, -1.2]]
        front = [[-0.6 * 0.7, -0.5 * 0.7, 0.7], [0.7 * 0.9, -0.4 * 0.9, 0.9], [0.1 * 0.8, 0.6 * 0.8, 0.8]]
        verts, faces = back + c["verts_cam"] + front, [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    elif kind == "zero_area":
        c = _golden("zero_area_face_skipped")
        verts, faces = c["verts_cam"], c["faces"]
    else:
        raise KeyError(kind)
    return torch.tensor([verts], dtype=torch.float32), np.asarray(faces, dtype=np.int32), cam


class Renderer:
    def __init__(self, lib, faces, V, H, aa):
        self.lib, self.H, self.aa, self.V = lib, H, aa, V
        self.faces = np.ascontiguousarray(torch.as_tensor(faces).numpy(), dtype=np.int32)
        self.h = lib.renderer_create(self.faces, V, image_size=H, aa=aa)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.renderer_destroy(self.h)


def oracle_raster(verts, cam, faces, S):
    from oracle import render_oracle as ro
    p2f, zbuf, _ = ro.rasterize(ro.project_ndc(verts, cam), torch.as_tensor(np.asarray(faces)).long(), S)
    return p2f, zbuf


def kernel_face_id(lib, device, r, verts, cam):
    """face_id of the library's own hard render (hifihr_render_fwd) for these vertices."""
    B, S = verts.shape[0], r.H * r.aa
    d = lambda t: t.to(device).contiguous()
    rgba = torch.empty(B, 4, r.H, r.H, device=device)
    fid = torch.full((B, S, S), -7, dtype=torch.int32, device=device)
    ws = torch.empty(lib.render_workspace_bytes(r.h, B), dtype=torch.uint8, device=device)
    lib.render_fwd(r.h, d(verts), torch.ones(r.V, 3, device=device), d(cam), torch.zeros(B, 3, device=device),
                   torch.tensor([[0.0, 0.0, -1.0]], device=device).repeat(B, 1).contiguous(), rgba, fid, ws)
    return fid


def run_depth(lib, device, r, verts, cam, face_id, gdepth=None):
    """-> (depth float32 [B,H,H], hits int32 [B,H,H], gverts float32 [B,V,3] or None) on the CPU.  Outputs start as canaries inside guard
    bands and must come back fully written with the bands untouched; the forward runs twice: the same bits both times."""
    B, H, V = verts.shape[0], r.H, r.V
    g = kc.Guards(device)
    v, c, f = g.inp(verts), g.inp(cam), g.inp(torch.as_tensor(face_id, dtype=torch.int32))
    outs = []
    for _ in range(2):
        depth, hits = g.out(B, 1, H, H, fill=float("nan")), g.out(B, H, H, dtype=torch.int32, fill=-99)
        lib.render_depth_fwd(r.h, v, c, f, depth, hits)
        outs.append((depth, hits))
    assert not bool(torch.isnan(outs[0][0]).any()) and not bool((outs[0][1] == -99).any()), "depth / hits: an element was not written"
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)), "depth: two calls differ in their bits"
    assert torch.equal(outs[0][1], outs[1][1]), "hits: two calls differ"
    gverts = None
    if gdepth is not None:
        ws = g.out(lib.render_depth_workspace_bytes(r.h, B), dtype=torch.uint8, fill=0xFF)
        gverts = g.out(B, V, 3, fill=float("nan"))
        lib.render_depth_bwd(r.h, v, c, f, g.inp(gdepth.float().reshape(B, 1, H, H)), outs[0][1], gverts, ws)
        assert not bool(torch.isnan(gverts).any()), "gverts: an element was not overwritten"
        gverts = gverts.cpu()
    g.intact("depth map")
    return outs[0][0].cpu().reshape(B, H, H), outs[0][1].cpu(), gverts


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def ulp_distance(a, b):
    """Largest distance in units of the last place between two float32 arrays of finite, same-signed values."""
    return int(np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64)).max()) if a.size else 0


def check_forward_bits(tag, lib, device, verts, cam, faces, H, aa, face_id=None):
    """The kernel's depth against the C rasteriser's zbuf (aa = 1) and the float32 restatement (every aa), bit for bit; hits exact."""
    S = H * aa
    p2f, zbuf = oracle_raster(verts, cam, faces, S)
    with Renderer(lib, faces, verts.shape[1], H, aa) as r:
        if face_id is None:
            face_id = p2f
        else:
            np.testing.assert_array_equal(np.asarray(face_id), p2f, err_msg=f"{tag}: the renderer's face_id is not the oracle's")
        depth, hits, _ = run_depth(lib, device, r, verts, cam, torch.as_tensor(np.asarray(face_id)))
    want, want_hits, _ = dr.depth_f32(verts.numpy(), cam.numpy(), faces, p2f, H, aa)
    depth, hits = depth.numpy(), hits.numpy()
    np.testing.assert_array_equal(hits, want_hits, err_msg=f"{tag}: hits")
    np.testing.assert_array_equal(want_hits, (p2f >= 0).reshape(-1, H, aa, H, aa).sum(axis=(2, 4)))
    assert not depth[hits == 0].any(), f"{tag}: a pixel without a covered sample is not exactly 0"
    if aa == 1:
        z = np.where(p2f >= 0, zbuf, np.float32(0.0)).astype(np.float32)
        assert np.array_equal(_bits(want), _bits(z)), f"{tag}: the float32 restatement is not the oracle's zbuf"       # the restatement itself
        diff = _bits(depth) != _bits(z)
        assert not diff.any(), f"{tag}: depth != zbuf in {int(diff.sum())} elements, largest distance {ulp_distance(depth[diff], z[diff])} ulp"
    diff = _bits(depth) != _bits(want)
    assert not diff.any(), (f"{tag}: depth differs from the float32 restatement in {int(diff.sum())} elements, "
                            f"largest distance {ulp_distance(depth[diff], want[diff])} ulp")
    return depth, hits, p2f


def bit_equality_case(lib, device, kind):
    verts, faces, cam = scene(kind)
    covered = 0
    for H, aa in SIZES:
        _, hits, _ = check_forward_bits(f"{kind} H={H} aa={aa}", lib, device, verts, cam, faces, H, aa)
        covered += int(hits.sum())
    assert covered > 0, f"{kind}: nothing is covered at any size"


def mano_bits_case(lib, device, tables, H=32, B=2, seed=0):
    """The MANO topology, B = 2, image_size 32, aa = 1, 2, 3, on the face_id of the library's own render."""
    verts, _, cam, _, _ = kc.make_render_inputs(tables, B, seed, H)
    verts, cam = verts.contiguous(), cam.contiguous()
    for aa in (1, 2, 3):
        with Renderer(lib, tables.faces, 778, H, aa) as r:
            fid = kernel_face_id(lib, device, r, verts, cam).cpu().numpy()
        _, hits, _ = check_forward_bits(f"mano H={H} aa={aa}", lib, device, verts, cam, np.asarray(tables.faces), H, aa, face_id=fid)
        assert 0.02 < float((hits > 0).mean()) < 0.9


def known_answers_case(lib, device):
    """tests/golden/raster_known.json stores an exactly derived zbuf per listed sample.  With image_size = the file's sample grid and
    aa = 1 every sample is a pixel: depth equals the stored value within the file's own bound (rtol 2e-6, as tests/test_raster_known.py),
    hits is 1 there, and depth is 0 with hits 0 where the file says miss."""
    cases = json.load(open(os.path.join(kc.REPO, "tests", "golden", "raster_known.json")))["cases"]
    listed = 0
    for c in cases:
        verts = torch.tensor([c["verts_cam"]], dtype=torch.float32)
        S = c["image_size"] * c["aa"]
        fid = np.asarray(c["pix_to_face"], dtype=np.int32).reshape(1, S, S)
        with Renderer(lib, c["faces"], verts.shape[1], S, 1) as r:
            depth, hits, _ = run_depth(lib, device, r, verts, torch.tensor([UNIT_CAM]), torch.as_tensor(fid))
        np.testing.assert_array_equal(hits[0].numpy(), (fid[0] >= 0).astype(np.int32), err_msg=c["name"])
        assert not bool(depth[0][torch.as_tensor(fid[0] < 0)].any()), c["name"]
        for s in c["samples"]:
            yi, xi = s["yi"], s["xi"]
            listed += 1
            if s["face"] >= 0:
                assert int(hits[0, yi, xi]) == 1
                np.testing.assert_allclose(float(depth[0, yi, xi]), s["zbuf"], rtol=2e-6, err_msg=c["name"])
            else:
                assert int(hits[0, yi, xi]) == 0 and float(depth[0, yi, xi]) == 0.0, (c["name"], s)
    assert listed >= 15


# ---- gradient -----------------------------------------------------------------------------------------------------------------------
# (H, aa, B, F, seed): F small triangles with vertices of their own plus unreferenced ones, Z in [0.3, 1.0], edges of 0.2 .. 0.6 NDC units
GRAD_CASES = [(8, 1, 1, 6, 0), (8, 3, 2, 6, 1), (9, 2, 2, 12, 2), (16, 3, 1, 12, 3), (17, 1, 2, 20, 4), (17, 3, 2, 20, 5)]
GRAD_EXTRA = 4          # unreferenced vertices per case


def grad_inputs(H, aa, B, F, seed):
    gen = torch.Generator().manual_seed(1000 + seed)
    centre = 1.2 * torch.rand(B, F, 1, 2, generator=gen) - 0.6
    ang = 2 * np.pi * (torch.rand(B, F, 1, generator=gen) + torch.tensor([0.0, 1 / 3, 2 / 3]).view(1, 1, 3) +
                       0.1 * (torch.rand(B, F, 3, generator=gen) - 0.5))
    rad = 0.2 + 0.25 * torch.rand(B, F, 3, generator=gen)
    ndc = centre + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], -1)            # [B,F,3,2]
    z = 0.3 + 0.7 * torch.rand(B, F, 3, 1, generator=gen)
    tri = torch.cat([ndc * z, z], -1).reshape(B, 3 * F, 3)
    extra = torch.cat([torch.rand(B, GRAD_EXTRA, 2, generator=gen) - 0.5, 0.3 + 0.7 * torch.rand(B, GRAD_EXTRA, 1, generator=gen)], -1)
    verts = torch.cat([tri, extra], 1)
    perm = torch.randperm(3 * F + GRAD_EXTRA, generator=gen)
    stored = torch.empty_like(verts)
    stored[:, perm] = verts
    faces = perm[torch.arange(3 * F).view(F, 3)]
    cam = torch.tensor([[1.05, 0.95, 0.03, -0.02]]).repeat(B, 1)
    w = torch.randn(B, H, H, generator=gen)
    return stored.contiguous(), faces.contiguous(), cam, w


def grad_errors(lib, device, H, aa, B, F, seed):
    """-> dict(kernel, f32, ratio, ...): the kernel's and the float32 restatement's gradient error against float64 autograd, each as max-abs
    over max-abs-ref, with the library's own face_id and the kernel's hits as constants."""
    verts, faces, cam, w = grad_inputs(H, aa, B, F, seed)
    V = verts.shape[1]
    with Renderer(lib, faces, V, H, aa) as r:
        fid = kernel_face_id(lib, device, r, verts, cam).cpu()
        depth, hits, gverts = run_depth(lib, device, r, verts, cam, fid, gdepth=w)
    want, want_hits, clamped = dr.depth_f32(verts.numpy(), cam.numpy(), faces.numpy(), fid.numpy(), H, aa)
    assert clamped == 0, "a covered sample sits on the denominator clamp: the case is meant to stay off it"
    np.testing.assert_array_equal(hits.numpy(), want_hits)
    grads = {}
    for dt in (torch.float64, torch.float32):
        v = verts.to(dt).requires_grad_(True)
        d = dr.depth_torch(v, cam, faces, fid, hits, H, aa, dtype=dt)
        (d * w.to(dt)).sum().backward()
        grads[dt] = v.grad.double()
        if dt == torch.float64:
            assert float((d.detach() - torch.as_tensor(want).double()).abs().max()) <= 1e-5, "float64 and float32 restatements disagree"
    ref = grads[torch.float64]
    scale = float(ref.abs().max())
    assert scale > 0 and float((hits > 0).float().mean()) > 0.05, "the case covers too little to see a wrong gradient"
    e_k = float((gverts.double() - ref).abs().max()) / scale
    e_32 = float((grads[torch.float32] - ref).abs().max()) / scale
    used = torch.zeros(V, dtype=torch.bool)
    used[faces.reshape(-1)] = True
    assert int((~used).sum()) == GRAD_EXTRA and not bool(gverts[:, ~used].any()), "an unreferenced vertex has a gradient"
    return dict(kernel=e_k, f32=e_32, ratio=e_k / e_32 if e_32 > 0 else float("inf"), scale=scale, coverage=float((hits > 0).float().mean()))


def gradient_case(lib, device, H, aa, B, F, seed):
    e = grad_errors(lib, device, H, aa, B, F, seed)
    bound = GRAD_FACTOR * e["f32"]
    print(f"[depth] gradient H={H} aa={aa} B={B} F={F} seed={seed}: kernel {e['kernel']:.3e}, float32 restatement {e['f32']:.3e}, "
          f"ratio {e['ratio']:.3f}, bound {bound:.3e}, coverage {e['coverage']:.2f}")
    assert e["kernel"] <= bound, e
    return bound


def clamp_case(lib, device):
    """One face at Z = 5e-5: t0 + t1 + t2 ~ 1e-10 sits under the 1e-8 clamp of the denominator.  The restatement confirms that covered
    samples are clamped; the gradients only have to be finite (and exactly 0 on the unreferenced vertex)."""
    H, aa, z = 9, 2, 5e-5
    pts = [(-0.7, -0.6), (0.8, -0.5), (-0.1, 0.75)]
    verts = torch.tensor([[[x * z, y * z, z] for x, y in pts] + [[0.0, 0.0, 0.5]]], dtype=torch.float32)
    faces, cam = np.asarray([[0, 1, 2]], dtype=np.int32), torch.tensor([UNIT_CAM])
    p2f, _ = oracle_raster(verts, cam, faces, H * aa)
    _, hits_ref, clamped = dr.depth_f32(verts.numpy(), cam.numpy(), faces, p2f, H, aa)
    assert clamped > 0 and clamped == int((p2f >= 0).sum()), "the case is meant to put every covered sample on the clamp"
    with Renderer(lib, faces, 4, H, aa) as r:
        depth, hits, gverts = run_depth(lib, device, r, verts, cam, torch.as_tensor(p2f), gdepth=torch.ones(1, H, H))
    np.testing.assert_array_equal(hits.numpy(), hits_ref)
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(gverts).all()) and bool(gverts[0, :3].any()) and not bool(gverts[0, 3].any())


# ---- loss pair ----------------------------------------------------------------------------------------------------------------------
def loss_inputs(B, HW, kind, seed=0):
    """d, hits, D, mask (int64, or None), trunc.  kind "mixed": every sort of pixel; "empty": no valid pixel; "one": HW = 1."""
    gen = torch.Generator().manual_seed(77 + seed)
    d = 0.3 + 0.6 * torch.rand(B, HW, generator=gen)
    D = (d + 0.05 * torch.randn(B, HW, generator=gen)).clamp(min=0.05)
    hits = torch.randint(1, 10, (B, HW), generator=gen, dtype=torch.int32)
    mask = torch.ones(B, HW, dtype=torch.int64)
    if kind == "empty":
        hits[0], D[1:] = 0, 0.0
        return d, hits, D, mask, 0.0
    if kind == "one":
        return d, hits, D, mask, 0.0
    assert HW >= 12
    for b in range(B):
        o = b % 3
        hits[b, o] = 0; d[b, o] = 0.0                      # the mesh does not cover it
        D[b, o + 1] = 0.0                                  # no measurement
        D[b, o + 2] = -1.0                                 # (a negative target is no measurement either)
        mask[b, o + 3] = 0                                 # masked out
        D[b, o + 4] = d[b, o + 4]                          # d == D: valid, gradient 0
        D[b, o + 5] = d[b, o + 5] + 0.5                    # far behind: cut by trunc when it is on
        D[b, o + 6] = (d[b, o + 6] - 0.4).clamp(min=0.01)  # far in front: cut by trunc when it is on
        D[b, o + 7] = d[b, o + 7] + 0.01                   # near, d < D
        D[b, o + 8] = d[b, o + 8] - 0.01                   # near, d > D
    return d, hits, D, mask, 0.1


LOSS_SHAPES = [(1, 12), (2, 17 * 17), (3, 300)]           # (B, HW): below one pass of 256 lanes, above it, B = 3


def run_loss(lib, device, d, hits, D, mask, lam, trunc, gout):
    """-> (out float32 scalar, sums float64 [B,2], gdepth float32 [B,HW]) on the CPU; the forward runs twice on garbage-filled outputs."""
    B = d.shape[0]
    dv, hv, Dv = d.to(device).contiguous(), hits.to(device).contiguous(), D.to(device).contiguous()
    mv = None if mask is None else mask.to(device).contiguous()
    res = []
    for fill in (-3e300, 7e200):
        sums = torch.full((B, 2), fill, dtype=torch.float64, device=device)
        out = torch.full((1,), float("nan"), device=device)
        lib.depth_loss_fwd(dv, hv, Dv, mv, lam, trunc, sums, out)
        res.append((out, sums))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)), "out: two calls differ in their bits"
    assert torch.equal(res[0][1].view(torch.int64), res[1][1].view(torch.int64)), "sums: two calls differ in their bits"
    g = torch.full_like(dv, float("nan"))
    lib.depth_loss_bwd(dv, hv, Dv, mv, res[0][1], torch.tensor([gout], device=device), lam, trunc, g)
    return res[0][0].cpu().numpy()[0], res[0][1].cpu().numpy(), g.cpu().numpy()


def check_loss(tag, lib, device, d, hits, D, mask, lam, trunc, gout=0.7):
    out, sums, g = run_loss(lib, device, d, hits, D, mask, lam, trunc, gout)
    m = None if mask is None else mask.numpy()
    want_sums = dr.loss_sums_ordered(d.numpy(), hits.numpy(), D.numpy(), m, trunc)
    assert np.array_equal(sums.view(np.int64), want_sums.view(np.int64)), (tag, sums, want_sums)
    want = dr.loss_value(want_sums, lam)
    assert ulp_distance(np.asarray([out]), np.asarray([want])) <= 1, (tag, out, want)
    ok, e = dr.loss_valid(d.numpy(), hits.numpy(), D.numpy(), m, trunc)
    exact = float(np.float32(lam)) * (np.abs(e[ok]).sum() / max(int(ok.sum()), 1))                     # any order: the same to 1e-12
    assert abs(float(out) - exact) <= 1e-6 * max(abs(exact), 1e-30) + 1e-45, (tag, out, exact)
    want_g = dr.loss_grad(d.numpy(), hits.numpy(), D.numpy(), m, trunc, want_sums, gout, lam)
    assert np.array_equal(_bits(g), _bits(want_g)), f"{tag}: gdepth is not the formula's, in {int((_bits(g) != _bits(want_g)).sum())} elements"
    return out, sums, g, ok, e


def loss_case(lib, device, B, HW):
    d, hits, D, mask, trunc = loss_inputs(B, HW, "mixed")
    lam = 0.37
    for t in (0.0, trunc):
        ok, e = dr.loss_valid(d.numpy(), hits.numpy(), D.numpy(), mask.numpy(), t)
        # the condition on a mixed case: one valid pixel and one invalid pixel of every kind, asserted on the restatement
        h, Dn, mn = hits.numpy(), D.numpy(), mask.numpy()
        assert ok.any() and (h == 0).any() and (Dn == 0).any() and (Dn < 0).any() and (mn == 0).any() and (e[ok] == 0).any()
        assert (e[ok] > 0).any() and (e[ok] < 0).any()
        if t > 0:
            cut = (h > 0) & (Dn > 0) & (mn != 0) & (np.abs(e) > t)
            assert (cut & (e > 0)).any() and (cut & (e < 0)).any() and not (ok & cut).any(), "trunc needs a pixel on each side"
        for mk, name in ((mask, "int64"), (mask.float(), "float32")):
            out, sums, g, ok2, e2 = check_loss(f"loss B={B} HW={HW} trunc={t} mask {name}", lib, device, d, hits, D, mk, lam, t)
            assert not g[~ok2].any() and not g[ok2 & (e2 == 0)].any() and np.all(g[ok2 & (e2 != 0)] != 0)
        # mask NULL: the masked-out pixels count
        o3, s3, _, ok3, _ = check_loss(f"loss B={B} HW={HW} trunc={t} no mask", lib, device, d, hits, D, None, lam, t)
        assert int(s3[:, 1].sum()) == int(sums[:, 1].sum()) + int(((mn == 0) & ok3).sum()) and ((mn == 0) & ok3).any()
    print(f"[depth] loss B={B} HW={HW}: out {float(out):.6e}, valid {int(sums[:, 1].sum())} of {B * HW}")


def loss_edge_cases(lib, device):
    # a batch without a valid pixel: exactly 0 and an all-zero gradient
    d, hits, D, mask, _ = loss_inputs(2, 40, "empty")
    out, sums, g, ok, _ = check_loss("loss without a valid pixel", lib, device, d, hits, D, mask, 1.0, 0.0)
    assert not ok.any() and float(out) == 0.0 and not sums.any() and not g.any()
    # HW = 1, valid and invalid
    d, hits, D, mask, _ = loss_inputs(1, 1, "one")
    out, sums, g, ok, _ = check_loss("loss HW=1", lib, device, d, hits, D, None, 2.0, 0.0)
    assert ok.all() and float(sums[0, 1]) == 1.0 and float(g[0, 0]) != 0.0
    out, _, g, _, _ = check_loss("loss HW=1 uncovered", lib, device, d, torch.zeros_like(hits), D, None, 2.0, 0.0)
    assert float(out) == 0.0 and float(g[0, 0]) == 0.0


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
    from hifihr_amd._lib import _fp as fp, _ip as ip
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    cf = ctypes.c_float
    H, aa, B = 5, 2, 2
    verts, faces, cam, w = grad_inputs(H, aa, B, 4, 9)
    V, S = verts.shape[1], H * aa
    verts, cam, w = verts.to(device), cam.to(device), w.to(device).contiguous()
    with Renderer(lib, faces, V, H, aa) as r:
        n = [lib.render_depth_workspace_bytes(r.h, b) for b in range(5)]
        assert n[0] == 0 and all(a <= b for a, b in zip(n, n[1:])) and n[1] >= 12 * V, n
        assert lib.render_depth_workspace_bytes(None, 2) == 0 and lib.render_depth_workspace_bytes(r.h, -1) == 0
        fid = kernel_face_id(lib, device, r, verts, cam)
        depth, gverts = torch.full((B, 1, H, H), -1234.5, device=device), torch.full((B, V, 3), -1234.5, device=device)
        hits = torch.full((B, H, H), -77, dtype=torch.int32, device=device)
        good_hits = torch.ones(B, H, H, dtype=torch.int32, device=device)
        ws = torch.full((n[B],), 0xA5, dtype=torch.uint8, device=device)
        base = dict(h=r.h, verts=fp(verts), cam=fp(cam), fid=ip(fid), B=B, depth=fp(depth), hits=ip(hits))
        for what, change in [(f"{k} NULL", {k: None}) for k in ("h", "verts", "cam", "fid", "depth", "hits")] + [("B < 0", dict(B=-1))]:
            a = dict(base, **change)
            _refused(lib, device, "hifihr_render_depth_fwd", (a["h"], a["verts"], a["cam"], a["fid"], a["B"], a["depth"], a["hits"], None),
                     (depth, hits), what)
        base = dict(h=r.h, verts=fp(verts), cam=fp(cam), fid=ip(fid), g=fp(w), hits=ip(good_hits), B=B, gverts=fp(gverts), ws=vp(ws))
        for what, change in [(f"{k} NULL", {k: None}) for k in ("h", "verts", "cam", "fid", "g", "hits", "gverts", "ws")] + [("B < 0", dict(B=-1))]:
            a = dict(base, **change)
            _refused(lib, device, "hifihr_render_depth_bwd", (a["h"], a["verts"], a["cam"], a["fid"], a["g"], a["hits"], a["B"], a["gverts"],
                                                              a["ws"], None), (gverts, ws), what)
        # B == 0: accepted, nothing launched, nothing written
        before = [t.clone() for t in (depth, hits, gverts, ws)]
        if device == "cpu":
            kc.launch_log(lib)
        assert lib.c.hifihr_render_depth_fwd(r.h, fp(verts), fp(cam), ip(fid), 0, fp(depth), ip(hits), None) == 0
        assert lib.c.hifihr_render_depth_bwd(r.h, fp(verts), fp(cam), ip(fid), fp(w), ip(good_hits), 0, fp(gverts), vp(ws), None) == 0
        if device == "cpu":
            assert not kc.launch_log(lib)
        else:
            torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((depth, hits, gverts, ws), before))
    # the loss pair
    HW = H * H
    d, D = torch.rand(B, HW, device=device) + 0.2, torch.rand(B, HW, device=device) + 0.2
    hh = torch.ones(B, HW, dtype=torch.int32, device=device)
    M = (torch.rand(B, HW, device=device) > 0.5).float()
    sums = torch.full((B, 2), -3e300, dtype=torch.float64, device=device)
    out, g, gout = torch.full((1,), -1234.5, device=device), torch.full((B, HW), -1234.5, device=device), torch.ones(1, device=device)
    bad = [("B < 0", dict(B=-1)), ("HW = 0", dict(HW=0)), ("HW < 0", dict(HW=-3)), ("mask kind 2", dict(kind=2)), ("mask kind -1", dict(kind=-1)),
           ("trunc < 0", dict(trunc=-1e-3)), ("trunc NaN", dict(trunc=float("nan"))), ("trunc inf", dict(trunc=float("inf"))),
           ("lam NaN", dict(lam=float("nan"))), ("lam inf", dict(lam=float("-inf")))]
    base = dict(d=fp(d), hits=ip(hh), D=fp(D), M=vp(M), kind=0, B=B, HW=HW, lam=1.0, trunc=0.0, sums=vp(sums), out=fp(out))
    for what, change in [(f"{k} NULL", {k: None}) for k in ("d", "hits", "D", "sums", "out")] + bad:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_depth_loss_fwd", (a["d"], a["hits"], a["D"], a["M"], a["kind"], a["B"], a["HW"], cf(a["lam"]), cf(a["trunc"]),
                                                        a["sums"], a["out"], None), (sums, out), what)
    good_sums = torch.ones(B, 2, dtype=torch.float64, device=device)
    base = dict(d=fp(d), hits=ip(hh), D=fp(D), M=vp(M), kind=0, sums=vp(good_sums), gout=fp(gout), B=B, HW=HW, lam=1.0, trunc=0.0, g=fp(g))
    for what, change in [(f"{k} NULL", {k: None}) for k in ("d", "hits", "D", "sums", "gout", "g")] + bad + [("B = 65536", dict(B=65536))]:
        a = dict(base, **change)
        _refused(lib, device, "hifihr_depth_loss_bwd", (a["d"], a["hits"], a["D"], a["M"], a["kind"], a["sums"], a["gout"], a["B"], a["HW"],
                                                        cf(a["lam"]), cf(a["trunc"]), a["g"], None), (g,), what)
    if device == "cpu":
        kc.launch_log(lib)
    assert lib.c.hifihr_depth_loss_fwd(fp(d), ip(hh), fp(D), None, 0, 0, HW, cf(1.0), cf(0.0), vp(sums), fp(out), None) == 0
    assert lib.c.hifihr_depth_loss_bwd(fp(d), ip(hh), fp(D), None, 0, vp(good_sums), fp(gout), 0, HW, cf(1.0), cf(0.0), fp(g), None) == 0
    if device == "cpu":
        assert not kc.launch_log(lib)
    else:
        torch.cuda.synchronize()
    assert bool((out == -1234.5).all()) and bool((g == -1234.5).all()) and bool((sums == -3e300).all())
    # a NULL mask itself is accepted
    lib.depth_loss_fwd(d, hh, D, None, 1.0, 0.0, sums, out)
    assert float(out.cpu()) > 0


KERNELS = {"render_depth_fwd_kernel", "render_depth_bwd_kernel", "render_depth_proj_bwd_kernel", "depth_loss_sums_kernel",
           "depth_loss_finish_kernel", "depth_loss_bwd_kernel"}


def launched_kernels(log):
    """Kernel names of a launch log without their template arguments."""
    return {k.split("<")[0] for k in log}
