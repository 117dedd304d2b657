"""Kernel-level parity cases shared by the hostsim (CPU, `not gpu`) and HIP (`gpu`) test modules.

Each case drives the C ABI through hifihr_amd._lib.HifihrLib with tensors on `device` and compares with the
oracle.  `lib` is either the product library (device='cuda') or tests/hostsim's emulator build (device='cpu').
"""
import os
import subprocess

import numpy as np
import torch

from hifihr_amd._lib import HifihrLib
from oracle import mano_oracle as mo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM_DIR = os.path.join(REPO, "tests", "hostsim")
HOSTSIM_LIB = os.path.join(HOSTSIM_DIR, "libhifihr_hostsim.so")


def bn_slots(stats, C, slots=32):
    """[slots][2][C] partial (sum, sum of squares) view of a batch-norm FORWARD statistics buffer: float64 since round 3
    (include/hifihr.h: hifihr_bn_stats_floats; csrc/hifihr_internal.h "FORWARD statistics")."""
    return stats[:slots * 2 * C * 2].view(torch.float64).view(slots, 2, C)


def build_hostsim() -> HifihrLib:
    subprocess.run(["make", "-s", "-C", HOSTSIM_DIR, "-j8"], check=True)
    return HifihrLib(HOSTSIM_LIB)


def launch_log(lib):
    """The kernels the emulator library launched since the last call, as their launch sites spell them (tests/hostsim/hostsim.cpp:
    template arguments are symbolic where the launch site is itself a template); the log is cleared."""
    import ctypes
    lib.c.hostsim_launch_log.restype = ctypes.c_char_p
    return lib.c.hostsim_launch_log().decode().splitlines()


def _dev(x, device):
    return torch.as_tensor(x).to(device).contiguous()


def mano_fwd_bwd_case(lib, tables, g, device, atol_v=5e-6, gtol=3e-4):
    """g: golden dict with pose, beta, wv, wj, verts, jtr, gpose, gbeta (reference ManoLayer outputs)."""
    h = lib.mano_create(tables)
    try:
        pose, beta = _dev(g["pose"], device), _dev(g["beta"], device)
        B = pose.shape[0]
        verts = torch.empty(B, 778, 3, device=device)
        jtr = torch.empty(B, 21, 3, device=device)
        saved = torch.empty(B, 778, 3, device=device)
        lib.mano_lbs_fwd(h, pose, beta, verts, jtr, saved)
        np.testing.assert_allclose(verts.cpu().numpy(), g["verts"], atol=atol_v, rtol=0)
        np.testing.assert_allclose(jtr.cpu().numpy(), g["jtr"], atol=atol_v, rtol=0)
        gpose = torch.empty(B, 48, device=device)
        gbeta = torch.empty(B, 10, device=device)
        lib.mano_lbs_bwd(h, pose, beta, saved, _dev(g["wv"], device), _dev(g["wj"], device), gpose, gbeta)
        scale_p = np.abs(g["gpose"]).max()
        scale_b = np.abs(g["gbeta"]).max()
        np.testing.assert_allclose(gpose.cpu().numpy(), g["gpose"], atol=gtol * scale_p, rtol=1e-4)
        np.testing.assert_allclose(gbeta.cpu().numpy(), g["gbeta"], atol=gtol * scale_b, rtol=1e-4)
    finally:
        lib.mano_destroy(h)


def mano_random_vs_oracle_case(lib, tables, device, B, seed):
    gen = torch.Generator().manual_seed(seed)
    pose = (0.6 * torch.randn(B, 48, generator=gen)).requires_grad_(True)
    beta = (0.7 * torch.randn(B, 10, generator=gen)).requires_grad_(True)
    wv = torch.randn(B, 778, 3, generator=gen)
    wj = torch.randn(B, 21, 3, generator=gen)
    verts, jtr, _ = mo.mano_forward(tables, pose, beta)
    ((verts * wv).sum() + (jtr * wj).sum()).backward()
    g = dict(pose=pose.detach().numpy(), beta=beta.detach().numpy(), wv=wv.numpy(), wj=wj.numpy(),
             verts=verts.detach().numpy(), jtr=jtr.detach().numpy(), gpose=pose.grad.numpy(), gbeta=beta.grad.numpy())
    mano_fwd_bwd_case(lib, tables, g, device)


def mano_joints_case(lib, tables, device, B, seed, root_id=9):
    gen = torch.Generator().manual_seed(seed)
    verts = (0.1 * torch.randn(B, 778, 3, generator=gen)).requires_grad_(True)
    j = mo.xyz_from_vertice(tables, verts)
    if root_id >= 0:
        jr, vr, root = mo.root_relative(j, verts, root_id)
    else:
        jr, vr, root = j, verts, torch.zeros(B, 1, 3)
    wj = torch.randn(B, 21, 3, generator=gen)
    wv = torch.randn(B, 778, 3, generator=gen)
    wr = torch.randn(B, 3, generator=gen)
    ((jr * wj).sum() + (vr * wv).sum() + (root.reshape(B, 3) * wr).sum()).backward()
    h = lib.mano_create(tables)
    try:
        vd = _dev(verts.detach(), device)
        o_j = torch.empty(B, 21, 3, device=device)
        o_v = torch.empty(B, 778, 3, device=device)
        o_r = torch.empty(B, 3, device=device)
        lib.mano_joints_fwd(h, vd, root_id, o_j, o_v, o_r)
        np.testing.assert_allclose(o_j.cpu().numpy(), jr.detach().numpy(), atol=2e-6)
        np.testing.assert_allclose(o_v.cpu().numpy(), vr.detach().numpy(), atol=2e-6)
        np.testing.assert_allclose(o_r.cpu().numpy(), root.detach().reshape(B, 3).numpy(), atol=2e-6)
        gv = torch.empty(B, 778, 3, device=device)
        lib.mano_joints_bwd(h, _dev(wj, device), _dev(wv, device), _dev(wr, device) if root_id >= 0 else None, root_id, gv)
        np.testing.assert_allclose(gv.cpu().numpy(), verts.grad.numpy(), atol=2e-4, rtol=1e-4)
    finally:
        lib.mano_destroy(h)


def mano_full_case(lib, tables, device, B, seed, root_id=9, with_cam=True):
    """hifihr_mano_full_fwd / _bwd (layer + joint regression + root-relative step + camera-space offset; the backward in one launch)
    against the ORACLE chain (oracle/mano_oracle.py: mano_forward -> xyz_from_vertice -> root_relative -> + root_xyz) and, bit for bit in
    the forward direction, against the two-call form of the same library."""
    gen = torch.Generator().manual_seed(seed)
    pose = (0.6 * torch.randn(B, 48, generator=gen)).requires_grad_(True)
    beta = (0.7 * torch.randn(B, 10, generator=gen)).requires_grad_(True)
    root_xyz = torch.randn(B, 3, generator=gen) * 0.3
    verts, _, _ = mo.mano_forward(tables, pose, beta)
    j = mo.xyz_from_vertice(tables, verts)
    if root_id >= 0:
        jr, vr, root = mo.root_relative(j, verts, root_id)
    else:
        jr, vr, root = j, verts, torch.zeros(B, 1, 3)
    vc = vr + root_xyz.unsqueeze(1)
    wj, wv, wc, wr = (torch.randn(B, 21, 3, generator=gen), torch.randn(B, 778, 3, generator=gen), torch.randn(B, 778, 3, generator=gen),
                      torch.randn(B, 3, generator=gen))
    tot = (jr * wj).sum() + (vr * wv).sum() + (root.reshape(B, 3) * wr).sum()
    if with_cam:
        tot = tot + (vc * wc).sum()
    tot.backward()
    h = lib.mano_create(tables)
    try:
        f = lambda *shape: torch.empty(*shape, device=device)
        pd, bd = _dev(pose.detach(), device), _dev(beta.detach(), device)
        o_verts, o_j, o_v, o_c, o_r, saved = f(B, 778, 3), f(B, 21, 3), f(B, 778, 3), f(B, 778, 3), f(B, 3), f(B, 778, 3)
        lib.mano_full_fwd(h, pd, bd, root_id, _dev(root_xyz, device), o_verts, o_j, o_v, o_c, o_r, saved)
        np.testing.assert_allclose(o_j.cpu().numpy(), jr.detach().numpy(), atol=5e-6)
        np.testing.assert_allclose(o_v.cpu().numpy(), vr.detach().numpy(), atol=5e-6)
        np.testing.assert_allclose(o_c.cpu().numpy(), vc.detach().numpy(), atol=5e-6)
        np.testing.assert_allclose(o_r.cpu().numpy(), root.detach().reshape(B, 3).numpy(), atol=5e-6)
        # the two-call form of the same library: identical bits
        t_verts, t_jtr, t_saved, t_j, t_v, t_r = f(B, 778, 3), f(B, 21, 3), f(B, 778, 3), f(B, 21, 3), f(B, 778, 3), f(B, 3)
        lib.mano_lbs_fwd(h, pd, bd, t_verts, t_jtr, t_saved)
        lib.mano_joints_fwd(h, t_verts, root_id, t_j, t_v, t_r)
        assert torch.equal(t_verts, o_verts) and torch.equal(t_saved, saved) and torch.equal(t_j, o_j) and torch.equal(t_v, o_v) and torch.equal(t_r, o_r)
        gp, gb = f(B, 48), f(B, 10)
        lib.mano_full_bwd(h, pd, bd, saved, _dev(wj, device), _dev(wv, device), _dev(wc, device) if with_cam else None,
                          _dev(wr, device) if root_id >= 0 else None, root_id, gp, gb)
        eg = float(np.abs(gp.cpu().numpy() - pose.grad.numpy()).max() / np.abs(pose.grad.numpy()).max())
        eb = float(np.abs(gb.cpu().numpy() - beta.grad.numpy()).max() / np.abs(beta.grad.numpy()).max())
        assert eg <= 3e-4 and eb <= 3e-4, (eg, eb)
        gp2, gb2 = f(B, 48), f(B, 10)                         # deterministic: no float atomics
        lib.mano_full_bwd(h, pd, bd, saved, _dev(wj, device), _dev(wv, device), _dev(wc, device) if with_cam else None,
                          _dev(wr, device) if root_id >= 0 else None, root_id, gp2, gb2)
        assert torch.equal(gp, gp2) and torch.equal(gb, gb2)
        # gradients that reach pose / beta through their other consumer are added inside the launch
        ap, ab = torch.randn(B, 48, generator=gen), torch.randn(B, 10, generator=gen)
        lib.mano_full_bwd(h, pd, bd, saved, _dev(wj, device), _dev(wv, device), _dev(wc, device) if with_cam else None,
                          _dev(wr, device) if root_id >= 0 else None, root_id, gp2, gb2, gpose_add=_dev(ap, device), gbeta_add=_dev(ab, device))
        assert torch.equal(gp2.cpu(), gp.cpu() + ap) and torch.equal(gb2.cpu(), gb.cpu() + ab)
    finally:
        lib.mano_destroy(h)


# ------------------------------------------------------------------------------------------------
# renderer
# ------------------------------------------------------------------------------------------------
def make_render_inputs(tables, B, seed, image_size, z=0.6):
    """Posed synthetic hands in front of a FreiHAND-like camera (scaled to `image_size`)."""
    from oracle import render_oracle as ro
    gen = torch.Generator().manual_seed(seed)
    pose = 0.4 * torch.randn(B, 48, generator=gen)
    pose[:, :3] = torch.randn(B, 3, generator=gen)             # arbitrary global orientation
    beta = 0.5 * torch.randn(B, 10, generator=gen)
    verts, _, _ = mo.mano_forward(tables, pose, beta)
    root = torch.stack([0.05 * (torch.rand(B, generator=gen) - 0.5), 0.05 * (torch.rand(B, generator=gen) - 0.5),
                        z + 0.2 * torch.rand(B, generator=gen)], dim=1)
    verts = (verts + root.unsqueeze(1)).detach()
    f = 450.0 + 200.0 * torch.rand(B, generator=gen)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = f; K[:, 1, 1] = f; K[:, 2, 2] = 1
    K[:, 0, 2] = 112 + 20 * (torch.rand(B, generator=gen) - 0.5)
    K[:, 1, 2] = 112 + 20 * (torch.rand(B, generator=gen) - 0.5)
    cam = ro.ndc_camera_from_K(K)                             # NDC camera: independent of the raster size
    vcol = 0.3 + 0.6 * torch.rand(B, 778, 3, generator=gen)
    lc = torch.rand(B, 3, generator=gen) * 1.6 - 0.6           # hardtanh range [-1,1]
    ld = torch.randn(B, 3, generator=gen)
    return verts, vcol, cam, lc, ld


def texture_pca_case(lib, device, B, K, n, seed=0, with_mean=True):
    """csrc/texpca.hip vs torch: tex = mean + coef . basis and d(sum(tex * w))/dcoef."""
    gen = torch.Generator().manual_seed(seed)
    coef = torch.randn(B, K, generator=gen); basis = torch.randn(K, n, generator=gen) * 0.1
    mean = torch.rand(n, generator=gen) if with_mean else None
    w = torch.randn(B, n, generator=gen)
    cr = coef.clone().requires_grad_(True)
    ref = cr @ basis + (mean if with_mean else 0.0)
    (ref * w).sum().backward()
    d = lambda t: t.to(device).contiguous() if t is not None else None
    out = torch.full((B, n), 7.0, device=device)
    lib.texture_pca_fwd(d(coef), d(basis), d(mean), out)
    assert float((out.cpu() - ref.detach()).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    dc = torch.zeros(B, K, device=device)
    lib.texture_pca_bwd(d(w), d(basis), dc)
    assert float((dc.cpu() - cr.grad).abs().max()) <= 2e-5 * float(cr.grad.abs().max()) * max(1.0, (n / 4096) ** 0.5)


def nimble_sized_mesh(B, seed, V=5990):
    """A closed genus-0 mesh with the NIMBLE skin's counts (V = 5990 vertices, F = 2 V - 4 = 11976 faces; reference
    models_res_nimble.py:135-136): a UV sphere of 499 rings x 12 segments + 2 poles, hand-sized (about 0.1 x 0.06 x 0.18 m), with a
    seeded bumpy radial displacement per batch item so that layers of surface overlap in the image like fingers do.  Synthetic: the
    real NIMBLE assets are not available."""
    rings, segs = (V - 2) // 12, 12
    assert rings * segs + 2 == V
    gen = torch.Generator().manual_seed(seed)
    th = (torch.arange(rings, dtype=torch.float32) + 1) / (rings + 1) * np.pi
    ph = torch.arange(segs, dtype=torch.float32) / segs * 2 * np.pi
    T, P = torch.meshgrid(th, ph, indexing="ij")
    base = torch.stack([torch.sin(T) * torch.cos(P), torch.sin(T) * torch.sin(P), torch.cos(T)], -1).reshape(-1, 3)
    base = torch.cat([torch.tensor([[0.0, 0.0, 1.0]]), base, torch.tensor([[0.0, 0.0, -1.0]])], 0)                       # [V,3]
    faces = []
    for j in range(segs):
        faces.append((0, 1 + j, 1 + (j + 1) % segs))
        last = 1 + (rings - 1) * segs
        faces.append((V - 1, last + (j + 1) % segs, last + j))
    for i in range(rings - 1):
        for j in range(segs):
            a, b = 1 + i * segs + j, 1 + i * segs + (j + 1) % segs
            c, d = a + segs, b + segs
            faces.append((a, c, b)); faces.append((b, c, d))
    faces = np.asarray(faces, dtype=np.int32)
    assert faces.shape[0] == 2 * V - 4
    k = torch.randn(B, 6, 3, generator=gen) * 3.0
    amp = 0.25 * torch.rand(B, 6, generator=gen)
    bump = 1.0 + (amp.unsqueeze(1) * torch.sin(torch.einsum("vc,bkc->bvk", base, k))).sum(-1)                                # [B,V]
    verts = base.unsqueeze(0) * bump.unsqueeze(-1) * torch.tensor([0.05, 0.03, 0.09])
    return verts, faces


def render_case(lib, tables, device, B, seed, image_size, aa, check_grad=True, rgb_atol=2e-5, gtol=2e-3, mesh=None, point_lights=False):
    from oracle import render_oracle as ro
    verts, vcol, cam, lc, ld = make_render_inputs(tables, B, seed, image_size)
    if point_lights:                            # PointLights defaults: diffuse .3, location (0, 1, 0) (+ a second, closer location)
        lc = torch.full((B, 3), 0.3)
        ld = torch.tensor([[0.0, 1.0, 0.0]]).repeat(B, 1)
        if B > 1:
            ld[1] = torch.tensor([0.1, -0.2, 0.3])
    faces_np, V = tables.faces, 778
    if mesh is not None:                        # another mesh in place of the hand: (verts [B,V,3] around the origin, faces [F,3])
        mv, faces_np = mesh
        V = mv.shape[1]
        gen = torch.Generator().manual_seed(seed + 5)
        verts = mv + verts.mean(1, keepdim=True)                    # same placements in front of the camera
        vcol = 0.3 + 0.6 * torch.rand(B, V, 3, generator=gen)
    faces = torch.as_tensor(faces_np).long()
    vr, cr, lcr, ldr = (t.clone().requires_grad_(True) for t in (verts, vcol, lc, ld))
    rgba_ref, p2f_ref = ro.render(vr, cr, cam, lcr, ldr, faces, image_size=image_size, aa=aa, point_lights=point_lights)
    S = image_size * aa
    h = lib.renderer_create(faces_np, V, image_size=image_size, aa=aa)
    if point_lights:
        lib.renderer_set_light_mode(h, True)
    try:
        ws = torch.empty(lib.render_workspace_bytes(h, B), dtype=torch.uint8, device=device)
        d = lambda t: t.to(device).contiguous()
        rgba = torch.empty(B, 4, image_size, image_size, device=device)
        fid = torch.empty(B, S, S, dtype=torch.int32, device=device)
        dv, dc, dcam, dlc, dld = d(verts), d(vcol), d(cam), d(lc), d(ld)
        lib.render_fwd(h, dv, dc, dcam, dlc, dld, rgba, fid, ws)
        fid_np = fid.cpu().numpy()
        assert (p2f_ref >= 0).mean() > 0.02, "test mesh barely visible"
        np.testing.assert_array_equal(fid_np, p2f_ref)             # bit-exact face indices
        np.testing.assert_allclose(rgba.cpu().numpy(), rgba_ref.detach().numpy(), atol=rgb_atol, rtol=0)
        if not check_grad:
            return
        gen = torch.Generator().manual_seed(seed + 1)
        w = torch.randn(B, 4, image_size, image_size, generator=gen)
        (rgba_ref * w).sum().backward()
        gv = torch.empty(B, V, 3, device=device); gc = torch.empty(B, V, 3, device=device)
        glc = torch.empty(B, 3, device=device); gld = torch.empty(B, 3, device=device)
        lib.render_bwd(h, dv, dcam, dlc, dld, fid, d(w), gv, gc, glc, gld, ws)
        checks = [("verts", gv, vr.grad), ("vcolors", gc, cr.grad), ("light_color", glc, lcr.grad)]
        if point_lights:
            assert float(gld.abs().max()) == 0.0           # the location is a constant of the default-lighting branch
        else:
            checks.append(("light_dir", gld, ldr.grad))
        for name, got, ref in checks:
            ref = ref.numpy()
            scale = np.abs(ref).max() + 1e-12
            err = np.abs(got.cpu().numpy() - ref).max() / scale
            assert err < gtol, f"grad {name}: max err / max |ref| = {err:.3e} (scale {scale:.3e})"
        # a SECOND backward after the one forward: the accumulators the forward's vertex kernel zeroed are dirty now, the launcher clears them
        gv2 = torch.full((B, V, 3), 7.0, device=device); gc2 = torch.full((B, V, 3), 7.0, device=device)
        glc2 = torch.full((B, 3), 7.0, device=device); gld2 = torch.full((B, 3), 7.0, device=device)
        lib.render_bwd(h, dv, dcam, dlc, dld, fid, d(w), gv2, gc2, glc2, gld2, ws)
        for name, a, b2 in (("verts", gv, gv2), ("vcolors", gc, gc2), ("light_color", glc, glc2), ("light_dir", gld, gld2)):
            scale = float(a.abs().max()) + 1e-12
            assert float((a - b2).abs().max()) <= 1e-5 * scale, f"second backward on one forward's workspace: grad {name} differs"
    finally:
        lib.renderer_destroy(h)


def synthetic_uv_tables(faces_np, V, seed=0):
    """A UV layout for any mesh: one uv per (face, corner) -- faces_uvs = arange(3 F) -- placed by a seeded planar map of the vertex index
    plus a per-face jitter, all inside [0.05, 0.95] (texture seams everywhere: the general TexturesUV case)."""
    rng = np.random.default_rng(seed)
    F_ = len(faces_np)
    base = rng.random((V, 2)).astype(np.float32) * 0.8 + 0.1
    uv = base[np.asarray(faces_np).reshape(-1)] + (rng.random((3 * F_, 2)).astype(np.float32) - 0.5) * 0.1
    return np.arange(3 * F_, dtype=np.int32).reshape(F_, 3), np.clip(uv, 0.05, 0.95).astype(np.float32)


def render_uv_case(lib, tables, device, B, seed, image_size, aa, TH=24, TW=40, rgb_atol=3e-5, gtol=3e-3, uv_scale=1.0):
    """hifihr_render_fwd_uv / _bwd_uv vs oracle/render_oracle.render(textures_uv=...) ([recalled] PyTorch3D TexturesUV semantics through
    torch's own grid_sample): face ids exact, pixels, and the gradients w.r.t. vertices (incl. the path through uv), texture maps, light."""
    from oracle import render_oracle as ro
    verts, _, cam, lc, ld = make_render_inputs(tables, B, seed, image_size)
    faces_np, V = tables.faces, 778
    faces = torch.as_tensor(faces_np).long()
    fu, vu = synthetic_uv_tables(faces_np, V, seed)
    if uv_scale != 1.0:                         # uvs outside [0, 1]: grid_sample's border padding (clamped coordinate, zero uv gradient there)
        vu = ((vu - 0.5) * uv_scale + 0.5).astype(np.float32)
        assert (vu < 0).any() and (vu > 1).any()
    gen = torch.Generator().manual_seed(seed + 3)
    maps = torch.rand(B, TH, TW, 3, generator=gen)
    vr, mr, lcr, ldr = (t.clone().requires_grad_(True) for t in (verts, maps, lc, ld))
    rgba_ref, p2f_ref = ro.render(vr, None, cam, lcr, ldr, faces, image_size=image_size, aa=aa,
                                  textures_uv=(mr, torch.from_numpy(fu).long(), torch.from_numpy(vu)))
    S = image_size * aa
    h = lib.renderer_create(faces_np, V, image_size=image_size, aa=aa)
    try:
        lib.renderer_set_uv(h, fu, vu)
        ws = torch.empty(lib.render_workspace_bytes(h, B), dtype=torch.uint8, device=device)
        d = lambda t: t.to(device).contiguous()
        rgba = torch.empty(B, 4, image_size, image_size, device=device)
        fid = torch.empty(B, S, S, dtype=torch.int32, device=device)
        texels = gtexels = None                                     # (reserved arguments: the texture is sampled inside the tile kernels)
        assert lib.render_uv_scratch_bytes(h, B) == 0
        dv, dm, dcam, dlc, dld = d(verts), d(maps), d(cam), d(lc), d(ld)
        lib.render_fwd_uv(h, dv, dm, dcam, dlc, dld, rgba, fid, texels, ws)
        assert (p2f_ref >= 0).mean() > 0.02, "test mesh barely visible"
        np.testing.assert_array_equal(fid.cpu().numpy(), p2f_ref)
        np.testing.assert_allclose(rgba.cpu().numpy(), rgba_ref.detach().numpy(), atol=rgb_atol, rtol=0)
        w = torch.randn(B, 4, image_size, image_size, generator=torch.Generator().manual_seed(seed + 1))
        (rgba_ref * w).sum().backward()
        gv = torch.empty(B, V, 3, device=device); gm = torch.zeros(B, TH, TW, 3, device=device)
        glc = torch.empty(B, 3, device=device); gld = torch.empty(B, 3, device=device)
        lib.render_bwd_uv(h, dv, dm, dcam, dlc, dld, fid, d(w), texels, gtexels, gv, gm, glc, gld, ws)
        for name, got, ref in (("verts", gv, vr.grad), ("maps", gm, mr.grad), ("light_color", glc, lcr.grad), ("light_dir", gld, ldr.grad)):
            ref = ref.numpy()
            scale = np.abs(ref).max() + 1e-12
            err = np.abs(got.cpu().numpy() - ref).max() / scale
            assert err < gtol, f"grad {name}: max err / max |ref| = {err:.3e} (scale {scale:.3e})"
    finally:
        lib.renderer_destroy(h)


# ------------------------------------------------------------------------------------------------
# fused Adam
# ------------------------------------------------------------------------------------------------
def adam_case(lib, device, n, wd, steps, grad_scale=0.5, lr=1e-3):
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p = p0.clone().to(device); m = torch.zeros(n, device=device); v = torch.zeros(n, device=device)
    for s in range(1, steps + 1):
        g = torch.randn(n, generator=gen)
        ref.grad = (g * grad_scale).clone()
        opt.step()
        if s % 2:
            lib.adam_step(p, g.to(device), m, v, grad_scale, lr, 0.9, 0.999, 1e-8, wd, s)
        else:           # the graph-replayable variant: scalars from device memory
            dyn = torch.tensor([lr / (1 - 0.9 ** s), 1.0 / (1 - 0.999 ** s) ** 0.5], dtype=torch.float32).to(device)
            lib.adam_step_dyn(p, g.to(device), m, v, grad_scale, 0.9, 0.999, 1e-8, wd, dyn)
    np.testing.assert_allclose(p.cpu().numpy(), ref.detach().numpy(), atol=2e-6, rtol=1e-5)
    # the counted variant (step counter and lr in device memory, bias corrections derived by the kernel): the same trajectory, and the counter
    # the last workgroup advances ends at `steps`; started from a state image at step 1 to cover a restored counter
    gen = torch.Generator().manual_seed(n)
    torch.randn(n, generator=gen)
    pc = p0.clone().to(device); mc = torch.zeros(n, device=device); vc = torch.zeros(n, device=device)
    state = None
    for s in range(1, steps + 1):
        g = torch.randn(n, generator=gen)
        if s == 1:
            lib.adam_step(pc, g.to(device), mc, vc, grad_scale, lr, 0.9, 0.999, 1e-8, wd, 1)
            state = lib.adam_state_image(lr, 0.9, 0.999, 1).to(device)
        else:
            lib.adam_step_counted(pc, g.to(device), mc, vc, grad_scale, 1e-8, wd, state)
    np.testing.assert_allclose(pc.cpu().numpy(), ref.detach().numpy(), atol=2e-6, rtol=1e-5)
    import struct
    lr_d, b1_d, b2_d, p1_d, p2_d, step_d, done_d = struct.unpack("<dddddii", bytes(state.cpu().numpy().tobytes()))
    assert (lr_d, step_d, done_d) == (lr, steps, 0), (lr_d, step_d, done_d)
    assert abs(p1_d - 0.9 ** steps) <= 1e-14 and abs(p2_d - 0.999 ** steps) <= 1e-14


# ------------------------------------------------------------------------------------------------
# convolution (NHWC implicit GEMM on the f32 matrix cores) vs plain PyTorch fp32 conv2d
# ------------------------------------------------------------------------------------------------
def conv_case(lib, device, N, H, W, C, K, R, stride, pad, seed=0, bias=False, rtol=2e-5, zero_last_channel=False):
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(K, C, R, R, generator=gen) / (C * R * R) ** 0.5
    if zero_last_channel:                       # the encoder's NHWC4 stem: channel 3 of the image and of the filter is padding
        x[:, C - 1] = 0.0; w[:, C - 1] = 0.0
    b = torch.randn(K, generator=gen) if bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, b, stride=stride, padding=pad)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    OH, OW = y.shape[2], y.shape[3]
    d = lambda t: t.to(device).contiguous()
    x_nhwc = d(x.permute(0, 2, 3, 1)); w_krsc = d(w.permute(0, 2, 3, 1)); gy_nhwc = d(gy.permute(0, 2, 3, 1))
    out = torch.empty(N, OH, OW, K, device=device)
    lib.conv2d_fwd(x_nhwc, w_krsc, d(b) if bias else None, out, N, H, W, C, K, R, R, stride, pad)
    ref = y.detach().permute(0, 2, 3, 1)
    scale = float(ref.abs().max())
    assert float((out.cpu() - ref).abs().max()) <= rtol * scale + 1e-6, "conv fwd"
    dx = torch.empty(N, H, W, C, device=device)
    scratch = torch.empty(K * R * R * C, device=device)
    lib.conv2d_bwd_data(gy_nhwc, w_krsc, dx, scratch, N, H, W, C, K, R, R, stride, pad)
    refx = xr.grad.permute(0, 2, 3, 1)
    assert float((dx.cpu() - refx).abs().max()) <= rtol * float(refx.abs().max()) + 1e-6, "conv bwd data"
    dw = torch.zeros(K, R, R, C, device=device)
    lib.conv2d_bwd_weight(x_nhwc, gy_nhwc, dw, N, H, W, C, K, R, R, stride, pad)
    refw = wr.grad.permute(0, 2, 3, 1)
    assert float((dw.cpu() - refw).abs().max()) <= 5 * rtol * float(refw.abs().max()) + 1e-6, "conv bwd weight"
    # accumulation semantics: a second call adds
    lib.conv2d_bwd_weight(x_nhwc, gy_nhwc, dw, N, H, W, C, K, R, R, stride, pad)
    assert float((dw.cpu() - 2 * refw).abs().max()) <= 1e-4 * float(refw.abs().max()) + 1e-6, "conv bwd weight accumulate"
    # slab forms of the weight gradient (caller's scratch, any contents): same gradient, bit-reproducible
    nws = lib.conv2d_wgrad_workspace_bytes(N, H, W, C, K, R, R, stride, pad)
    if nws:
        wsw = torch.full((nws // 4,), 3.0, device=device)
        dws = torch.full((K, R, R, C), 0.5, device=device)
        lib.conv2d_bwd_weight(x_nhwc, gy_nhwc, dws, N, H, W, C, K, R, R, stride, pad, ws=wsw)
        assert float((dws.cpu() - 0.5 - refw).abs().max()) <= 5 * rtol * float(refw.abs().max()) + 1e-6, "conv bwd weight (slabs)"
        dws2 = torch.full((K, R, R, C), 0.5, device=device)
        lib.conv2d_bwd_weight(x_nhwc, gy_nhwc, dws2, N, H, W, C, K, R, R, stride, pad, ws=wsw)
        assert torch.equal(dws, dws2), "slab weight gradient must be bit-reproducible"
    # balanced (stream-K) schedule through a zero-initialised, self-cleaning workspace: same results, workspace zero again
    nb_f = lib.conv2d_workspace_bytes(N, H, W, C, K, R, R, stride, pad, False)
    nb_b = lib.conv2d_workspace_bytes(N, H, W, C, K, R, R, stride, pad, True)
    used = 0
    if nb_f and not bias:
        ws = torch.zeros(nb_f // 4, device=device); out2 = torch.full_like(out, 7.0)
        for _ in range(2):                                  # twice: the second call must find the workspace clean
            lib.conv2d_fwd(x_nhwc, w_krsc, None, out2, N, H, W, C, K, R, R, stride, pad, ws=ws)
            assert float((out2.cpu() - ref).abs().max()) <= rtol * scale + 1e-6, "conv fwd (balanced schedule)"
            assert float(ws.abs().max()) == 0.0, "workspace not cleaned"
        used += 1
    if nb_b:
        ws = torch.zeros(nb_b // 4, device=device); dx2 = torch.full_like(dx, 7.0)
        lib.conv2d_bwd_data(gy_nhwc, w_krsc, dx2, scratch, N, H, W, C, K, R, R, stride, pad, ws=ws)
        assert float((dx2.cpu() - refx).abs().max()) <= rtol * float(refx.abs().max()) + 1e-6, "conv bwd data (balanced schedule)"
        assert float(ws.abs().max()) == 0.0, "workspace not cleaned"
        used += 1
    return used


def image_to_nhwc4_case(lib, device):
    from oracle.torch_modules import normalize_batch_3C
    img = torch.rand(3, 3, 20, 12)
    out = torch.empty(3, 20, 12, 4, device=device)
    lib.image_to_nhwc4(img.to(device), out)
    ref = normalize_batch_3C(img).permute(0, 2, 3, 1)
    np.testing.assert_allclose(out.cpu()[..., :3].numpy(), ref.numpy(), atol=1e-6)
    assert float(out.cpu()[..., 3].abs().max()) == 0.0
    # padded, un-normalised variant (EfficientNet stem): F.pad(img, (left, right, top, bottom)) as NHWC4
    import torch.nn.functional as F
    pad4 = (0, 1, 0, 1)
    out2 = torch.full((3, 21, 13, 4), 7.0, device=device)
    lib.image_to_nhwc4_padded(img.to(device), out2, pad4, False)
    ref2 = F.pad(img, pad4).permute(0, 2, 3, 1)
    assert torch.equal(out2.cpu()[..., :3], ref2) and float(out2.cpu()[..., 3].abs().max()) == 0.0
    out3 = torch.full((3, 23, 15, 4), 7.0, device=device)
    lib.image_to_nhwc4_padded(img.to(device), out3, (2, 1, 1, 2), True)
    ref3 = F.pad(normalize_batch_3C(img), (2, 1, 1, 2)).permute(0, 2, 3, 1)
    np.testing.assert_allclose(out3.cpu()[..., :3].numpy(), ref3.numpy(), atol=1e-6)


# ------------------------------------------------------------------------------------------------
# fused SSIM vs vectors produced by the reference's utils/pytorch_ssim (tests/golden/ssim.npz) and vs the
# torch restatement in oracle/loss_oracle.py (itself pinned to the same vectors on the CPU)
# ------------------------------------------------------------------------------------------------
def ssim_case(lib, device, a, b, ref_val=None, ref_grad=None):
    from oracle import loss_oracle as L
    from hifihr_amd.ops import _ssim_window
    win = _ssim_window()
    a_t, b_t = torch.as_tensor(a), torch.as_tensor(b)
    if ref_val is None:
        ar = a_t.clone().requires_grad_(True)
        v = L.ssim(ar, b_t)
        v.backward()
        ref_val, ref_grad = float(v), ar.grad.numpy()
    B, C, H, W = a_t.shape
    da, db = a_t.to(device).contiguous(), b_t.to(device).contiguous()
    partial = torch.empty(lib.ssim_partial_count(B * C, H, W), device=device)
    maps = torch.empty(3, B, C, H, W, device=device)
    lib.ssim_fwd(win, da, db, partial, maps[0], maps[1], maps[2])
    val = float(partial.sum()) / (B * C * H * W)
    assert abs(val - float(ref_val)) <= 2e-6 * max(1.0, abs(float(ref_val))), (val, float(ref_val))
    g = torch.empty_like(da)
    lib.ssim_bwd(win, da, db, maps[0], maps[1], maps[2], torch.full((1,), 2.0, device=device), g)
    ref = 2.0 * np.asarray(ref_grad)
    assert np.abs(g.cpu().numpy() - ref).max() <= 2e-4 * np.abs(ref).max() + 1e-10
    # the call site's scalar glue: lambda * (1 - SSIM) in one finishing launch, the gradient scale folded into the backward
    n, lam = B * C * H * W, 0.37
    out = torch.full((), 7.0, device=device)
    lib.ssim_finish(partial, 1.0 / n, 0.0, out)
    assert abs(float(out) - val) <= 2e-6 * max(1.0, abs(val))
    lib.ssim_finish(partial, -lam / n, lam, out)
    assert abs(float(out) - lam * (1.0 - val)) <= 2e-6
    g2 = torch.empty_like(da)
    lib.ssim_bwd_scaled(win, da, db, maps[0], maps[1], maps[2], torch.full((1,), 2.0, device=device), -lam, g2)
    assert float((g2 + lam * g).abs().max()) <= 1e-6 * float(g.abs().max()) + 1e-12


# ------------------------------------------------------------------------------------------------
# fused train-mode BatchNorm (+ residual add + ReLU), NHWC, vs plain PyTorch fp32 (F.batch_norm + add + relu autograd)
# ------------------------------------------------------------------------------------------------
def bn_act_case(lib, device, N, H, W, C, relu, residual, seed=0, from_conv=False):
    """relu: True / False / "swish"."""
    act = {False: 0, True: 1, "swish": 2}[relu]
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    M = N * H * W
    x = torch.randn(N, C, H, W, generator=gen) * 1.5 + 0.3
    gamma = 1 + 0.1 * torch.randn(C, generator=gen); beta = 0.1 * torch.randn(C, generator=gen)
    res = torch.randn(N, C, H, W, generator=gen) if residual else None
    rm0, rv0 = torch.randn(C, generator=gen) * 0.1, 1 + 0.1 * torch.rand(C, generator=gen)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if residual else None
    rm, rv = rm0.clone(), rv0.clone()
    out = F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5)
    if residual:
        out = out + rr
    if act == 1:
        out = F.relu(out)
    elif act == 2:
        out = out * torch.sigmoid(out)
    gy = torch.randn(out.shape, generator=gen)
    out.backward(gy)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(device)
    dx_in = nhwc(x)
    stats = torch.zeros(lib.bn_stats_floats(C), device=device)      # zero on entry (self-cleaning contract)
    lib.bn_stats(dx_in, M, C, stats)
    np.testing.assert_allclose(bn_slots(stats, C).sum(0)[0].cpu().numpy(), x.permute(1, 0, 2, 3).reshape(C, -1).sum(1).numpy(),
                               rtol=1e-4, atol=1e-3)
    y = torch.empty(N, H, W, C, device=device); sm = torch.empty(C, device=device); si = torch.empty(C, device=device)
    rmd, rvd = rm0.clone().to(device), rv0.clone().to(device)
    lib.bn_act_fwd(dx_in, stats, gamma.to(device), beta.to(device), nhwc(res) if residual else None, act, M, C, 1e-5, 0.1, y, sm, si, rmd, rvd)
    assert float(stats.abs().max()) == 0.0, "bn_act_fwd must leave the slots and arrival counters zeroed"
    ref = out.detach().permute(0, 2, 3, 1)
    assert float((y.cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), "bn fwd"
    np.testing.assert_allclose(rmd.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rvd.cpu().numpy(), rv.numpy(), rtol=1e-4, atol=1e-6)
    red = torch.zeros(lib.bn_stats_floats(C), device=device); dxo = torch.empty_like(y); dres = torch.empty_like(y) if residual else None
    dg = torch.full((C,), 0.5, device=device); db = torch.full((C,), -0.25, device=device)     # accumulate semantics
    lib.bn_act_bwd(nhwc(gy), y if act == 1 else None, dx_in, sm, si, gamma.to(device), beta.to(device), act, M, C, red, dxo, dres, dg, db)
    assert float(red[:32 * 4 * C + 64].abs().max()) == 0.0, "bn_act_bwd must leave the slots and arrival counters zeroed"
    if act == 1 and not residual:       # ReLU mask recomputed from x instead of read from y: the same gradients (the slot sums
        #                                 are float atomics, so two launches agree to rounding, not to the bit)
        dxo2 = torch.full_like(dxo, 7.0); dg2 = torch.zeros_like(dg); db2 = torch.zeros_like(db)
        lib.bn_act_bwd(nhwc(gy), None, dx_in, sm, si, gamma.to(device), beta.to(device), act, M, C, red, dxo2, None, dg2, db2)
        dg1 = torch.zeros_like(dg); db1 = torch.zeros_like(db); dxo1 = torch.full_like(dxo, 7.0)
        lib.bn_act_bwd(nhwc(gy), y, dx_in, sm, si, gamma.to(device), beta.to(device), act, M, C, red, dxo1, None, dg1, db1)
        scale = float(dxo1.abs().max())
        assert float((dxo1 - dxo2).abs().max()) <= 2e-6 * scale, "mask recomputed from x: dx"
        assert float(((dxo1 == 0) != (dxo2 == 0)).float().mean()) <= 1e-5, "mask recomputed from x: same zero pattern"
        assert float((dg1 - dg2).abs().max()) <= 1e-5 * float(dg1.abs().max()) + 1e-6 and float((db1 - db2).abs().max()) <= 1e-5 * float(db1.abs().max()) + 1e-6
    refdx = xr.grad.permute(0, 2, 3, 1)
    assert float((dxo.cpu() - refdx).abs().max()) <= 2e-4 * float(refdx.abs().max()) + 1e-7, "bn bwd dx"
    assert float((dg.cpu() - 0.5 - gr.grad).abs().max()) <= 2e-4 * float(gr.grad.abs().max()) + 1e-5, "bn dgamma"
    assert float((db.cpu() + 0.25 - br.grad).abs().max()) <= 2e-4 * float(br.grad.abs().max()) + 1e-5, "bn dbeta"
    if residual:
        assert float((dres.cpu() - rr.grad.permute(0, 2, 3, 1)).abs().max()) <= 1e-6, "bn dres"


def conv_bnstats_case(lib, device, N, H, W, C, K, R, stride, pad, seed=0, use_ws=False):
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen); w = torch.randn(K, C, R, R, generator=gen) / (C * R * R) ** 0.5
    y = F.conv2d(x, w, None, stride, pad)
    OH, OW = y.shape[2], y.shape[3]
    d = lambda t: t.to(device).contiguous()
    out = torch.empty(N, OH, OW, K, device=device); stats = torch.zeros(lib.bn_stats_floats(K), device=device)
    nb = lib.conv2d_workspace_bytes(N, H, W, C, K, R, R, stride, pad, False) if use_ws else 0
    ws = torch.zeros(nb // 4, device=device) if nb else None
    assert not use_ws or nb > 0, "this case was meant to exercise the balanced schedule"
    lib.conv2d_fwd_bnstats(d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), out, stats, N, H, W, C, K, R, R, stride, pad, ws=ws)
    assert ws is None or float(ws.abs().max()) == 0.0
    ref = y.permute(0, 2, 3, 1)
    assert float((out.cpu() - ref).abs().max()) <= 3e-5 * float(ref.abs().max()) + 1e-6
    s_ref = y.permute(1, 0, 2, 3).reshape(K, -1)
    st = bn_slots(stats, K).sum(0)
    np.testing.assert_allclose(st[0].cpu().numpy(), s_ref.sum(1).numpy(), rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(st[1].cpu().numpy(), (s_ref ** 2).sum(1).numpy(), rtol=1e-4, atol=2e-3)


def conv_fwd_pair_case(lib, device, N, H, W, C, K1, K2, seed=0):
    """hifihr_conv2d_fwd_bnstats_pair: the strided 3x3 convolution of a residual stage's first block and the stride-2 1x1 convolution of its
    downsample branch in ONE launch == the two hifihr_conv2d_fwd_bnstats calls: outputs bit for bit, folded statistics to the f32 rounding of the per-share partial sums."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen); w1 = torch.randn(K1, C, 3, 3, generator=gen) / (9 * C) ** 0.5; w2 = torch.randn(K2, C, 1, 1, generator=gen) / C ** 0.5
    r1, r2 = F.conv2d(x, w1, None, 2, 1), F.conv2d(x, w2, None, 2, 0)
    OH, OW = r1.shape[2], r1.shape[3]
    assert r2.shape[2:] == r1.shape[2:]
    d = lambda t: t.to(device).contiguous()
    xd, w1d, w2d = d(x.permute(0, 2, 3, 1)), d(w1.permute(0, 2, 3, 1)), d(w2.permute(0, 2, 3, 1))
    assert lib.conv2d_fwd_bnstats_pair_supported(N, H, W, C, 2, K1, 3, 1, K2, 1, 0)
    ya, yb = torch.full((N, OH, OW, K1), 7.0, device=device), torch.full((N, OH, OW, K2), 7.0, device=device)
    sa, sb = torch.zeros(lib.bn_stats_floats(K1), device=device), torch.zeros(lib.bn_stats_floats(K2), device=device)
    lib.conv2d_fwd_bnstats_pair(xd, w1d, ya, sa, K1, 3, 1, w2d, yb, sb, K2, 1, 0, N, H, W, C, 2)
    y1, y2 = torch.empty_like(ya), torch.empty_like(yb)
    s1, s2 = torch.zeros_like(sa), torch.zeros_like(sb)
    lib.conv2d_fwd_bnstats(xd, w1d, y1, s1, N, H, W, C, K1, 3, 3, 2, 1)
    lib.conv2d_fwd_bnstats(xd, w2d, y2, s2, N, H, W, C, K2, 1, 1, 2, 0)
    assert torch.equal(ya, y1) and torch.equal(yb, y2), "pair: outputs differ from the separate launches"
    for K, p, q in ((K1, sa, s1), (K2, sb, s2)):
        a, b = bn_slots(p, K).sum(0).double().cpu(), bn_slots(q, K).sum(0).double().cpu()
        # (the shifted partial sums are f32 inside a workgroup's share, and the shares differ between the two forms: equal to f32 rounding of the
        #  per-share partials, observed 3e-8 of the largest sum)
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()) + 1e-9
    assert float((ya.cpu() - r1.permute(0, 2, 3, 1)).abs().max()) <= 3e-5 * float(r1.abs().max()) + 1e-6
    assert float((yb.cpu() - r2.permute(0, 2, 3, 1)).abs().max()) <= 3e-5 * float(r2.abs().max()) + 1e-6


def conv_dgrad_plus1x1_case(lib, device, N, H, W, C, K, stride=2, seed=0):
    """hifihr_conv2d_bwd_data_pre_plus1x1: backward-data of the strided 3x3 convolution with the data gradient of the 1x1 / same stride / pad 0
    convolution of the same input as one more tap of parity class (0, 0) == torch autograd of conv(x, w1) + conv(x, w2) wrt x, and ==
    the two separate launches (hifihr_conv2d_bwd_data_pre on the 1x1, its result as the residual of hifihr_conv2d_bwd_data_pre_res on the
    3x3) to the rounding of one more term per pixel of that class."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen).requires_grad_(True)
    w1 = torch.randn(K, C, 3, 3, generator=gen) / (9 * C) ** 0.5; w2 = torch.randn(K, C, 1, 1, generator=gen) / C ** 0.5
    y1, y2 = F.conv2d(x, w1, None, stride, 1), F.conv2d(x, w2, None, stride, 0)
    assert y1.shape == y2.shape
    g1, g2 = torch.randn(y1.shape, generator=gen), torch.randn(y2.shape, generator=gen)
    (y1 * g1).sum().backward(retain_graph=True)
    ref1 = x.grad.clone()
    x.grad = None
    ((y1 * g1).sum() + (y2 * g2).sum()).backward()
    ref = x.grad.permute(0, 2, 3, 1)
    d = lambda t: t.to(device).contiguous()
    g1d, g2d = d(g1.permute(0, 2, 3, 1)), d(g2.permute(0, 2, 3, 1))
    w1d, w2d = d(w1.permute(0, 2, 3, 1)), d(w2.permute(0, 2, 3, 1))                   # [K][R][S][C]
    wt1, wt2 = torch.empty(w1d.numel(), device=device), torch.empty(w2d.numel(), device=device)
    lib.weight_transpose(w1d, wt1, K, 9, C); lib.weight_transpose(w2d, wt2, K, 1, C)  # [C][R][S][K]
    assert lib.conv2d_bwd_data_pre_plus1x1_supported(N, H, W, C, K, 3, 3, stride, 1)
    dx = torch.full((N, H, W, C), 7.0, device=device)
    lib.conv2d_bwd_data_pre_plus1x1(g1d, wt1, g2d, wt2, dx, N, H, W, C, K, 3, 3, stride, 1)
    scale = float(ref.abs().max())
    assert float((dx.cpu() - ref).abs().max()) <= 3e-5 * scale + 1e-6, float((dx.cpu() - ref).abs().max())
    # the two-launch form it replaces
    dx2 = torch.full((N, H, W, C), 7.0, device=device); dxs = torch.full((N, H, W, C), 7.0, device=device)
    lib.conv2d_bwd_data_pre(g2d, wt2, dx2, N, H, W, C, K, 1, 1, stride, 0)
    lib.conv2d_bwd_data_pre_res(g1d, wt1, dx2, dxs, N, H, W, C, K, 3, 3, stride, 1)
    assert float((dx - dxs).abs().max()) <= 2e-6 * scale + 1e-7, float((dx - dxs).abs().max())
    # the pixels off class (0, 0) carry the 3x3 convolution's gradient alone: bit for bit what the plain launch gives
    dx1 = torch.full((N, H, W, C), 7.0, device=device)
    lib.conv2d_bwd_data_pre(g1d, wt1, dx1, N, H, W, C, K, 3, 3, stride, 1)
    off = torch.ones(H, W, dtype=torch.bool); off[::stride, ::stride] = False
    assert torch.equal(dx.cpu()[:, off], dx1.cpu()[:, off])
    assert float((dx1.cpu() - ref1.permute(0, 2, 3, 1)).abs().max()) <= 3e-5 * scale + 1e-6


def conv_wgrad_plus1x1_case(lib, device, N, H, W, C, K, stride=2, seed=0):
    """hifihr_conv2d_bwd_weight_plus1x1: the weight gradients of the strided 3x3 convolution and of the 1x1 / same stride / pad 0 convolution
    of the same input in one launch == torch autograd, and == hifihr_conv2d_bwd_weight on each (float atomics: to rounding); both ACCUMULATE."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen)
    w1 = (torch.randn(K, C, 3, 3, generator=gen) / (9 * C) ** 0.5).requires_grad_(True); w2 = (torch.randn(K, C, 1, 1, generator=gen) / C ** 0.5).requires_grad_(True)
    y1, y2 = F.conv2d(x, w1, None, stride, 1), F.conv2d(x, w2, None, stride, 0)
    g1, g2 = torch.randn(y1.shape, generator=gen), torch.randn(y2.shape, generator=gen)
    ((y1 * g1).sum() + (y2 * g2).sum()).backward()
    r1, r2 = w1.grad.permute(0, 2, 3, 1), w2.grad.permute(0, 2, 3, 1)
    d = lambda t: t.to(device).contiguous()
    xd, g1d, g2d = d(x.permute(0, 2, 3, 1)), d(g1.permute(0, 2, 3, 1)), d(g2.permute(0, 2, 3, 1))
    assert lib.conv2d_bwd_weight_plus1x1_supported(N, H, W, C, K, 3, 3, stride, 1)
    dw1 = torch.full((K, 3, 3, C), 0.5, device=device); dw2 = torch.full((K, 1, 1, C), -0.25, device=device)     # accumulated into
    lib.conv2d_bwd_weight_plus1x1(xd, g1d, dw1, g2d, dw2, N, H, W, C, K, 3, 3, stride, 1)
    for got, ref, base in ((dw1, r1, 0.5), (dw2, r2, -0.25)):
        sc = float(ref.abs().max())
        assert float((got.cpu() - base - ref).abs().max()) <= 3e-5 * sc + 1e-5, float((got.cpu() - base - ref).abs().max())
    s1 = torch.zeros(K, 3, 3, C, device=device); s2 = torch.zeros(K, 1, 1, C, device=device)
    lib.conv2d_bwd_weight(xd, g1d, s1, N, H, W, C, K, 3, 3, stride, 1)
    lib.conv2d_bwd_weight(xd, g2d, s2, N, H, W, C, K, 1, 1, stride, 0)
    assert float((dw1 - 0.5 - s1).abs().max()) <= 1e-5 * float(s1.abs().max()) + 1e-6
    assert float((dw2 + 0.25 - s2).abs().max()) <= 1e-5 * float(s2.abs().max()) + 1e-6


# ------------------------------------------------------------------------------------------------
# the convolution C ABI's contract: every entry point on any geometry (N, H, W, C, K, R, S, stride, pad) it is handed either refuses it
# (HIFIHR_EINVAL, output untouched) or computes it -- against float64 autograd, err <= c * sqrt(L) * max|ref| with L the reduction length
# ------------------------------------------------------------------------------------------------
# c per direction: the largest err / (sqrt(L) max|ref|) seen over the contract sweep times >= 4 (tests/test_hostsim_conv_contract.py, the GPU
# half in tests/test_gpu_conv.py).  A dropped tap or 16-channel chunk costs 1e-1 of max|ref| or more, c * sqrt(L) stays below 1e-3 at the sizes tested.
CONV_CONTRACT_C = {"fwd": 3e-7, "dgrad": 3e-7, "wgrad": 3e-7}
CONV_CONTRACT_STATS_C = 1e-6           # statistic sums: err <= c * sqrt(M) * sum over pixels of |y| (resp. y^2), M = N * OH * OW
CONV_CONTRACT_LOG = {}                 # entry -> [accepted, rejected, largest err / (c sqrt(L) max|ref|)] (the tests print it)


def _contract_log(entry, accepted, ratio=0.0):
    row = CONV_CONTRACT_LOG.setdefault(entry, [0, 0, 0.0])
    row[0 if accepted else 1] += 1
    row[2] = max(row[2], ratio)


def _contract_rejects(call, canaries, what):
    """call() must fail with HIFIHR_EINVAL and leave every canary tensor as it was."""
    from hifihr_amd._lib import HifihrError
    before = [t.clone() for t in canaries]
    try:
        call()
    except HifihrError as e:
        assert "failed (-1)" in str(e), f"{what}: refused with a code other than HIFIHR_EINVAL: {e}"
    else:
        raise AssertionError(f"{what}: accepted, expected HIFIHR_EINVAL")
    for a, b in zip(canaries, before):
        assert torch.equal(a, b), f"{what}: refused but wrote its output"


def _contract_close(entry, got, ref, L, what, kind=None, base=0.0):
    """err <= c * sqrt(L) * max|ref| + tiny (float64 ref, got on any device); logs the ratio."""
    c = CONV_CONTRACT_C[kind or entry]
    scale = float(ref.abs().max())
    err = float((got.detach().cpu().double() - base - ref).abs().max())
    bound = c * max(L, 1) ** 0.5 * scale + 1e-12
    _contract_log(entry, True, err / bound)
    assert err <= bound, f"{what}: err {err:.3e} vs bound {bound:.3e} (max|ref| {scale:.3e}, L {L})"


def conv_contract_expect(N, H, W, C, K, R, S, stride, pad):
    """Which plain entries the header documents as accepting this geometry (include/hifihr.h: C % 4 == 0; backward-data K % 4 == 0,
    K % 16 == 0 when stride > 1; backward-weight C % 4 == 0 and K % 4 == 0), given that the sizes themselves are valid."""
    ok = min(N, H, W, C, K, R, S, stride) > 0 and pad >= 0 and H + 2 * pad >= R and W + 2 * pad >= S
    return {"fwd": ok and C % 4 == 0, "dgrad": ok and K % 4 == 0 and (stride == 1 or K % 16 == 0), "wgrad": ok and C % 4 == 0 and K % 4 == 0}


def conv_contract_case(lib, device, N, H, W, C, K, R, S, stride, pad, seed=0):
    """Every convolution entry point of the C ABI on one geometry.  Plain entries (fwd, fwd_bnstats, bwd_data[_pre[_res]], bwd_weight) must accept
    exactly what conv_contract_expect documents; the fused entries (bwd_data_pre_plus1x1, bwd_weight_plus1x1, bwd_weight_c3) must do what their
    _supported predicate says.  An accepted call matches float64 autograd; a refused one returns HIFIHR_EINVAL and leaves its output's canary alone.
    Returns {entry: accepted}."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(K, C, R, S, generator=gen, dtype=torch.float64) / (C * R * S) ** 0.5
    b = torch.randn(K, generator=gen, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride=stride, padding=pad)
    OH, OW = y.shape[2], y.shape[3]
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(gy)
    ref, refx, refw = y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1), wr.grad.permute(0, 2, 3, 1)
    res = torch.randn(N, H, W, C, generator=gen, dtype=torch.float64)
    d = lambda t: t.float().to(device).contiguous()
    xd, wd, gyd, bd, resd = d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), d(gy.permute(0, 2, 3, 1)), d(b), d(res)
    wtd = d(w.permute(1, 2, 3, 0))                                                      # [C][R][S][K]: the pre-transposed filter
    geo = (N, H, W, C, K, R, S, stride, pad)
    Lf, Lw = C * R * S, N * OH * OW
    Ld = K * -(-R // stride) * -(-S // stride)
    expect = conv_contract_expect(*geo)
    got = {}
    canary = lambda *shape: torch.full(shape, 7.0, device=device)

    # ---- forward: no bias, bias, ReLU, the balanced schedule; with statistics (+ balanced)
    y_out = canary(N, OH, OW, K)
    if not expect["fwd"]:
        for e, call in (("fwd", lambda: lib.conv2d_fwd(xd, wd, None, y_out, *geo)),
                        ("fwd_bnstats", lambda: lib.conv2d_fwd_bnstats(xd, wd, y_out, torch.zeros(lib.bn_stats_floats(K), device=device), *geo))):
            _contract_rejects(call, [y_out], f"{e} {geo}")
            _contract_log(e, False)
            got[e] = False
    else:
        lib.conv2d_fwd(xd, wd, None, y_out, *geo)
        _contract_close("fwd", y_out, ref, Lf, f"fwd {geo}")
        y_b = canary(N, OH, OW, K)
        lib.conv2d_fwd(xd, wd, bd, y_b, *geo)
        _contract_close("fwd_bias", y_b, ref + b, Lf, f"fwd + bias {geo}", "fwd")
        y_r = canary(N, OH, OW, K)
        lib.conv2d_fwd(xd, wd, None, y_r, *geo, act=1)
        _contract_close("fwd_relu", y_r, ref.clamp_min(0), Lf, f"fwd + ReLU {geo}", "fwd")
        nb_f = lib.conv2d_workspace_bytes(*geo, False)
        if nb_f:
            ws = torch.zeros(nb_f // 4, device=device)
            for rep in range(2):                            # twice: the second call must find the workspace clean
                y_s = canary(N, OH, OW, K)
                lib.conv2d_fwd(xd, wd, None, y_s, *geo, ws=ws)
                _contract_close("fwd_ws", y_s, ref, Lf, f"fwd (balanced, call {rep}) {geo}", "fwd")
                assert float(ws.abs().max()) == 0.0, f"fwd (balanced) {geo}: workspace not handed back clean"
        M = N * OH * OW
        for use_ws in ((False, True) if nb_f else (False,)):
            e = "fwd_bnstats_ws" if use_ws else "fwd_bnstats"
            ws = torch.zeros(nb_f // 4, device=device) if use_ws else None
            y_s, st = canary(N, OH, OW, K), torch.zeros(lib.bn_stats_floats(K), device=device)
            lib.conv2d_fwd_bnstats(xd, wd, y_s, st, *geo, ws=ws)
            _contract_close(e, y_s, ref, Lf, f"{e} {geo}", "fwd")
            assert ws is None or float(ws.abs().max()) == 0.0, f"{e} {geo}: workspace not handed back clean"
            # the statistics of the y just checked against ref: its float64 column sums to the f32 rounding of the per-share partials
            sums, yk = bn_slots(st, K).sum(0).double().cpu(), y_s.cpu().double().reshape(-1, K)
            for i, (want, mag) in enumerate(((yk.sum(0), yk.abs().sum(0)), ((yk ** 2).sum(0), (yk ** 2).sum(0)))):
                err = float(((sums[i] - want).abs() / (mag + 1e-30)).max())
                bound = CONV_CONTRACT_STATS_C * M ** 0.5
                _contract_log(e + "_stats", True, err / bound)
                assert err <= bound, f"{e} {geo}: statistic {i} err {err:.3e} of sum|y| vs {bound:.3e}"
        got["fwd"] = got["fwd_bnstats"] = True

    # ---- backward-data: plain (transposes into scratch), pre-transposed, + residual, balanced
    dx_out = canary(N, H, W, C)
    scratch = torch.empty(K * R * S * C, device=device)
    dcalls = (("bwd_data", lambda o: lib.conv2d_bwd_data(gyd, wd, o, scratch, *geo), refx),
              ("bwd_data_pre", lambda o: lib.conv2d_bwd_data_pre(gyd, wtd, o, *geo), refx),
              ("bwd_data_pre_res", lambda o: lib.conv2d_bwd_data_pre_res(gyd, wtd, resd, o, *geo), refx + res))
    for e, call, want in dcalls:
        if not expect["dgrad"]:
            _contract_rejects(lambda: call(dx_out), [dx_out], f"{e} {geo}")
            _contract_log(e, False)
        else:
            o = canary(N, H, W, C)
            call(o)
            _contract_close(e, o, want, Ld, f"{e} {geo}", "dgrad")
    got["bwd_data"] = expect["dgrad"]
    nb_b = lib.conv2d_workspace_bytes(*geo, True) if expect["dgrad"] else 0
    if nb_b:
        ws = torch.zeros(nb_b // 4, device=device)
        for rep in range(2):
            o = canary(N, H, W, C)
            lib.conv2d_bwd_data(gyd, wd, o, scratch, *geo, ws=ws)
            _contract_close("bwd_data_ws", o, refx, Ld, f"bwd_data (balanced, call {rep}) {geo}", "dgrad")
            assert float(ws.abs().max()) == 0.0, f"bwd_data (balanced) {geo}: workspace not handed back clean"

    # ---- backward-weight: accumulates; a second call adds; the slab form is bit-reproducible
    dw = torch.full((K, R, S, C), 0.5, device=device)
    if not expect["wgrad"]:
        _contract_rejects(lambda: lib.conv2d_bwd_weight(xd, gyd, dw, *geo), [dw], f"bwd_weight {geo}")
        _contract_log("bwd_weight", False)
    else:
        lib.conv2d_bwd_weight(xd, gyd, dw, *geo)
        _contract_close("bwd_weight", dw, refw, Lw, f"bwd_weight {geo}", "wgrad", base=0.5)
        lib.conv2d_bwd_weight(xd, gyd, dw, *geo)
        _contract_close("bwd_weight_acc", dw, 2 * refw, Lw, f"bwd_weight (second call adds) {geo}", "wgrad", base=0.5)
        nws = lib.conv2d_wgrad_workspace_bytes(*geo)
        if nws:
            wsw = torch.full((nws // 4,), 3.0, device=device)           # any contents
            d1, d2 = torch.full((K, R, S, C), 0.5, device=device), torch.full((K, R, S, C), 0.5, device=device)
            lib.conv2d_bwd_weight(xd, gyd, d1, *geo, ws=wsw)
            lib.conv2d_bwd_weight(xd, gyd, d2, *geo, ws=wsw)
            _contract_close("bwd_weight_ws", d1, refw, Lw, f"bwd_weight (slabs) {geo}", "wgrad", base=0.5)
            assert torch.equal(d1, d2), f"bwd_weight (slabs) {geo}: not bit-reproducible"
    got["bwd_weight"] = expect["wgrad"]

    # ---- the fused entries: the second convolution is 1x1 / the same stride / pad 0 on the same input
    w2 = torch.randn(K, C, 1, 1, generator=gen, dtype=torch.float64) / C ** 0.5
    x2r, w2r = x.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    y2 = F.conv2d(x2r, w2r, None, stride=stride)
    gy2 = torch.randn(y2.shape, generator=gen, dtype=torch.float64)
    y2.backward(gy2)
    gy2d, w2d, wt2d = d(gy2.permute(0, 2, 3, 1)), d(w2.permute(0, 2, 3, 1)), d(w2.reshape(K, C).t())
    ok = lib.conv2d_bwd_data_pre_plus1x1_supported(*geo)
    o = canary(N, H, W, C)
    if not ok:
        _contract_rejects(lambda: lib.conv2d_bwd_data_pre_plus1x1(gyd, wtd, gy2d, wt2d, o, *geo), [o], f"bwd_data_pre_plus1x1 {geo}")
        _contract_log("bwd_data_pre_plus1x1", False)
    else:
        assert y2.shape == y.shape, f"bwd_data_pre_plus1x1 {geo}: accepted with different output grids"
        lib.conv2d_bwd_data_pre_plus1x1(gyd, wtd, gy2d, wt2d, o, *geo)
        want = refx + x2r.grad.permute(0, 2, 3, 1)
        _contract_close("bwd_data_pre_plus1x1", o, want, Ld + K, f"bwd_data_pre_plus1x1 {geo}", "dgrad")
        two, sep = canary(N, H, W, C), canary(N, H, W, C)                  # the two-launch form it replaces
        lib.conv2d_bwd_data_pre(gy2d, wt2d, two, N, H, W, C, K, 1, 1, stride, 0)
        lib.conv2d_bwd_data_pre_res(gyd, wtd, two, sep, *geo)
        _contract_close("bwd_data_pre_plus1x1_vs_2", o, sep.cpu().double(), Ld + K, f"bwd_data_pre_plus1x1 vs two launches {geo}", "dgrad")
    got["bwd_data_pre_plus1x1"] = ok

    ok = lib.conv2d_bwd_weight_plus1x1_supported(*geo)
    dw1, dw2 = torch.full((K, R, S, C), 0.5, device=device), torch.full((K, 1, 1, C), -0.25, device=device)
    if not ok:
        _contract_rejects(lambda: lib.conv2d_bwd_weight_plus1x1(xd, gyd, dw1, gy2d, dw2, *geo), [dw1, dw2], f"bwd_weight_plus1x1 {geo}")
        _contract_log("bwd_weight_plus1x1", False)
    else:
        assert y2.shape == y.shape, f"bwd_weight_plus1x1 {geo}: accepted with different output grids"
        lib.conv2d_bwd_weight_plus1x1(xd, gyd, dw1, gy2d, dw2, *geo)
        _contract_close("bwd_weight_plus1x1", dw1, refw, Lw, f"bwd_weight_plus1x1 (first) {geo}", "wgrad", base=0.5)
        _contract_close("bwd_weight_plus1x1", dw2, w2r.grad.permute(0, 2, 3, 1), Lw, f"bwd_weight_plus1x1 (1x1) {geo}", "wgrad", base=-0.25)
        s1, s2 = torch.zeros(K, R, S, C, device=device), torch.zeros(K, 1, 1, C, device=device)
        lib.conv2d_bwd_weight(xd, gyd, s1, *geo)
        lib.conv2d_bwd_weight(xd, gy2d, s2, N, H, W, C, K, 1, 1, stride, 0)
        _contract_close("bwd_weight_plus1x1_vs_2", dw1, s1.cpu().double(), Lw, f"bwd_weight_plus1x1 vs bwd_weight {geo}", "wgrad", base=0.5)
        _contract_close("bwd_weight_plus1x1_vs_2", dw2, s2.cpu().double(), Lw, f"bwd_weight_plus1x1 vs bwd_weight (1x1) {geo}", "wgrad", base=-0.25)
    got["bwd_weight_plus1x1"] = ok

    # ---- the 3-channel stem parameter (NHWC4 input): asked on the C = 4 geometries
    if C == 4:
        ok = lib.conv2d_bwd_weight_c3_supported(N, H, W, K, R, S, stride, pad)
        nws = lib.conv2d_wgrad_workspace_bytes(*geo)
        ws = torch.full((max(nws, 4096) // 4,), 3.0, device=device)
        dw3 = torch.full((K, R, S, 3), 0.25, device=device)
        if not ok:
            _contract_rejects(lambda: lib.conv2d_bwd_weight_c3(xd, gyd, dw3, N, H, W, K, R, S, stride, pad, ws), [dw3], f"bwd_weight_c3 {geo}")
            _contract_log("bwd_weight_c3", False)
        else:
            lib.conv2d_bwd_weight_c3(xd, gyd, dw3, N, H, W, K, R, S, stride, pad, ws)
            _contract_close("bwd_weight_c3", dw3, refw[..., :3], Lw, f"bwd_weight_c3 {geo}", "wgrad", base=0.25)
            again = torch.full((K, R, S, 3), 0.25, device=device)
            lib.conv2d_bwd_weight_c3(xd, gyd, again, N, H, W, K, R, S, stride, pad, ws)
            assert torch.equal(again, dw3), f"bwd_weight_c3 {geo}: not bit-reproducible"
        got["bwd_weight_c3"] = ok
    return got


def conv_pair_contract_case(lib, device, N, H, W, C, stride, K1, R1, pad1, K2, R2, pad2, seed=0):
    """hifihr_conv2d_fwd_bnstats_pair on one pair: refused (EINVAL, outputs untouched) where its _supported says so; else both outputs equal
    the two hifihr_conv2d_fwd_bnstats launches bit for bit, their statistics agree to the f32 rounding of per-share partials, and both
    outputs match float64 conv2d.  Returns whether the pair was accepted."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    w1 = torch.randn(K1, C, R1, R1, generator=gen, dtype=torch.float64) / (C * R1 * R1) ** 0.5
    w2 = torch.randn(K2, C, R2, R2, generator=gen, dtype=torch.float64) / (C * R2 * R2) ** 0.5
    r1, r2 = F.conv2d(x, w1, None, stride, pad1).permute(0, 2, 3, 1), F.conv2d(x, w2, None, stride, pad2).permute(0, 2, 3, 1)
    d = lambda t: t.float().to(device).contiguous()
    xd, w1d, w2d = d(x.permute(0, 2, 3, 1)), d(w1.permute(0, 2, 3, 1)), d(w2.permute(0, 2, 3, 1))
    ya, yb = torch.full(r1.shape, 7.0, device=device), torch.full(r2.shape, 7.0, device=device)
    sa, sb = torch.zeros(lib.bn_stats_floats(K1), device=device), torch.zeros(lib.bn_stats_floats(K2), device=device)
    call = lambda: lib.conv2d_fwd_bnstats_pair(xd, w1d, ya, sa, K1, R1, pad1, w2d, yb, sb, K2, R2, pad2, N, H, W, C, stride)
    what = f"fwd_bnstats_pair {(N, H, W, C, stride, K1, R1, pad1, K2, R2, pad2)}"
    if not lib.conv2d_fwd_bnstats_pair_supported(N, H, W, C, stride, K1, R1, pad1, K2, R2, pad2):
        _contract_rejects(call, [ya, yb, sa, sb], what)
        _contract_log("fwd_bnstats_pair", False)
        return False
    call()
    for (K, R, pad, y, s, r, wd) in ((K1, R1, pad1, ya, sa, r1, w1d), (K2, R2, pad2, yb, sb, r2, w2d)):
        _contract_close("fwd_bnstats_pair", y, r, C * R * R, what, "fwd")
        y1, s1 = torch.empty_like(y), torch.zeros_like(s)
        lib.conv2d_fwd_bnstats(xd, wd, y1, s1, N, H, W, C, K, R, R, stride, pad)
        assert torch.equal(y, y1), f"{what}: output differs from the separate launch"
        p, q = bn_slots(s, K).sum(0).double().cpu(), bn_slots(s1, K).sum(0).double().cpu()
        assert float((p - q).abs().max()) <= 1e-6 * float(q.abs().max()) + 1e-9, f"{what}: statistics differ from the separate launch"
    return True


# ------------------------------------------------------------------------------------------------
# depthwise convolution (EfficientNet MBConv) vs plain PyTorch fp32 (F.pad + grouped F.conv2d autograd)
# ------------------------------------------------------------------------------------------------
def dwconv_case(lib, device, N, H, W, C, K, stride, seed=0):
    import torch.nn.functional as F
    from hifihr_amd.effnet import static_same_pad
    gen = torch.Generator().manual_seed(seed)
    pl, pr, pt, pb = static_same_pad(K, stride)
    x = torch.randn(N, C, H, W, generator=gen); w = torch.randn(C, 1, K, K, generator=gen) / K
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(F.pad(xr, (pl, pr, pt, pb)), wr, None, stride, 0, 1, C)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    OH, OW = y.shape[2], y.shape[3]
    d = lambda t: t.to(device).contiguous()
    xd, wd, gyd = d(x.permute(0, 2, 3, 1)), d(w.reshape(C, K, K)), d(gy.permute(0, 2, 3, 1))
    out = torch.empty(N, OH, OW, C, device=device)
    stats = torch.zeros(lib.bn_stats_floats(C), device=device)
    lib.dwconv2d_fwd(xd, wd, out, N, H, W, C, OH, OW, K, stride, pt, pl, stats=stats)
    ref = y.detach().permute(0, 2, 3, 1)
    assert float((out.cpu() - ref).abs().max()) <= 2e-5 * float(ref.abs().max()) + 1e-6, "dw fwd"
    st = bn_slots(stats, C).sum(0).cpu()
    flat = ref.reshape(-1, C)
    np.testing.assert_allclose(st[0].numpy(), flat.sum(0).numpy(), rtol=1e-4, atol=2e-3, err_msg="dw fwd: batch-norm sum")
    np.testing.assert_allclose(st[1].numpy(), (flat ** 2).sum(0).numpy(), rtol=1e-4, atol=2e-3, err_msg="dw fwd: batch-norm sum of squares")
    out2 = torch.empty_like(out)
    lib.dwconv2d_fwd(xd, wd, out2, N, H, W, C, OH, OW, K, stride, pt, pl)            # without statistics
    assert torch.equal(out2, out)
    dx = torch.empty(N, H, W, C, device=device)
    lib.dwconv2d_bwd_data(gyd, wd, dx, N, H, W, C, OH, OW, K, stride, pt, pl)
    refx = xr.grad.permute(0, 2, 3, 1)
    assert float((dx.cpu() - refx).abs().max()) <= 2e-5 * float(refx.abs().max()) + 1e-6, "dw bwd data"
    dw = torch.zeros(C, K, K, device=device)
    lib.dwconv2d_bwd_weight(xd, gyd, dw, N, H, W, C, OH, OW, K, stride, pt, pl)
    refw = wr.grad.reshape(C, K, K)
    assert float((dw.cpu() - refw).abs().max()) <= 1e-4 * float(refw.abs().max()) + 1e-6, "dw bwd weight"


def dwconv_bnswish_case(lib, device, N, H, W, C, K, stride, seed=0, mean=0.3, std=1.5):
    """The expand half of an MBConv block without its activated tensor (hifihr_bn_finalize_fwd + hifihr_dwconv2d_fwd_bnswish /
    _bwd_weight_bnswish + hifihr_dwconv2d_bwd_data + hifihr_bn_act_bwd(swish)) vs plain PyTorch: nn.BatchNorm2d (training mode, eps
    1e-3, momentum 0.01 as the reference's blocks) -> x * sigmoid(x) -> F.pad + grouped F.conv2d, forward, every gradient, the
    running statistics; and bit for bit against the library's own unfused pair hifihr_bn_act_fwd + hifihr_dwconv2d_fwd."""
    import torch.nn.functional as F
    from hifihr_amd.effnet import static_same_pad
    gen = torch.Generator().manual_seed(seed)
    pl, pr, pt, pb = static_same_pad(K, stride)
    e = torch.randn(N, C, H, W, generator=gen) * std + mean
    w = torch.randn(C, 1, K, K, generator=gen) / K
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    eps, mom = 1e-3, 0.01
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    er, wr = e.clone().requires_grad_(True), w.clone().requires_grad_(True)
    z = bn(er)
    a = z * torch.sigmoid(z)
    y = F.conv2d(F.pad(a, (pl, pr, pt, pb)), wr, None, stride, 0, 1, C)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    OH, OW = y.shape[2], y.shape[3]
    M = N * H * W
    d = lambda t: t.to(device).contiguous()
    ed, wd, gyd, gd, bd = d(e.permute(0, 2, 3, 1)), d(w.reshape(C, K, K)), d(gy.permute(0, 2, 3, 1)), d(gamma), d(beta)
    f = lambda *shape: torch.empty(*shape, device=device)
    # statistics of e as its producer leaves them (the slot buffer), consumed by the finalize call
    stats = torch.zeros(lib.bn_stats_floats(C), device=device)
    lib.bn_stats(ed, M, C, stats)
    stats2 = stats.clone()
    mean_d, invstd_d, rm, rv = f(C), f(C), torch.zeros(C, device=device), torch.ones(C, device=device)
    lib.bn_finalize_fwd(stats, M, C, eps, mom, mean_d, invstd_d, rm, rv)
    assert float(stats.abs().max()) == 0.0, "finalize must hand the slots back zeroed"
    np.testing.assert_allclose(rm.cpu().numpy(), bn.running_mean.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rv.cpu().numpy(), bn.running_var.numpy(), rtol=1e-5, atol=1e-6)
    out = f(N, OH, OW, C)
    ystats = torch.zeros(lib.bn_stats_floats(C), device=device)
    lib.dwconv2d_fwd_bnswish(ed, mean_d, invstd_d, gd, bd, wd, out, N, H, W, C, OH, OW, K, stride, pt, pl, stats=ystats)
    ref = y.detach().permute(0, 2, 3, 1)
    err = float((out.cpu() - ref).abs().max()) / float(ref.abs().max())
    assert err <= 3e-5, f"dw fwd (bn + swish on load): {err}"
    st = bn_slots(ystats, C).sum(0).cpu()
    flat = ref.reshape(-1, C)
    np.testing.assert_allclose(st[0].numpy(), flat.sum(0).numpy(), rtol=2e-4, atol=5e-3)
    np.testing.assert_allclose(st[1].numpy(), (flat ** 2).sum(0).numpy(), rtol=2e-4, atol=5e-3)
    # the unfused pair of the same library: bn_act_fwd (swish) then dwconv2d_fwd -- the same bits
    a_d, m2, i2 = f(N, H, W, C), f(C), f(C)
    lib.bn_act_fwd(ed, stats2, gd, bd, None, 2, M, C, eps, mom, a_d, m2, i2, None, None)
    assert torch.equal(m2, mean_d) and torch.equal(i2, invstd_d)
    out_u = f(N, OH, OW, C)
    lib.dwconv2d_fwd(a_d, wd, out_u, N, H, W, C, OH, OW, K, stride, pt, pl)
    eu = float((out_u - out).abs().max()) / float(ref.abs().max())
    assert eu <= 2e-6, f"fused vs unfused forward: {eu}"
    # weight gradient from e
    dw = torch.zeros(C, K, K, device=device)
    lib.dwconv2d_bwd_weight_bnswish(ed, mean_d, invstd_d, gd, bd, gyd, dw, N, H, W, C, OH, OW, K, stride, pt, pl)
    refw = wr.grad.reshape(C, K, K)
    assert float((dw.cpu() - refw).abs().max()) <= 2e-4 * float(refw.abs().max()) + 1e-6, "dw bwd weight (bn + swish on load)"
    # gradient wrt e, gamma, beta: dwconv_bwd_data then the fused batch-norm backward with act = swish on (d a, e)
    da = f(N, H, W, C)
    lib.dwconv2d_bwd_data(gyd, wd, da, N, H, W, C, OH, OW, K, stride, pt, pl)
    red = torch.zeros(lib.bn_stats_floats(C), device=device)
    de, dg, db = f(N, H, W, C), torch.zeros(C, device=device), torch.zeros(C, device=device)
    lib.bn_act_bwd(da, None, ed, mean_d, invstd_d, gd, bd, 2, M, C, red, de, None, dg, db)
    refe = er.grad.permute(0, 2, 3, 1)
    assert float((de.cpu() - refe).abs().max()) <= 3e-4 * float(refe.abs().max()) + 1e-7, "d e"
    assert float((dg.cpu() - bn.weight.grad).abs().max()) <= 3e-4 * float(bn.weight.grad.abs().max()) + 1e-5, "d gamma"
    assert float((db.cpu() - bn.bias.grad).abs().max()) <= 3e-4 * float(bn.bias.grad.abs().max()) + 1e-5, "d beta"


# ------------------------------------------------------------------------------------------------
# pooling (csrc/pool.hip) vs plain PyTorch fp32
# ------------------------------------------------------------------------------------------------
def mmpool_case(lib, device, B, H, W, C, p0=0.3, seed=0, ties=False):
    """MMPool((1,1)): adaptive max + adaptive avg mixed by sigmoid(p) (reference network/res_encoder.py:247-265)."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen)
    if ties:
        x = torch.relu(x - 1.5)                    # mostly zeros with repeated maxima: first-index tie rule
    xr = x.clone().requires_grad_(True); pr = torch.tensor([p0], requires_grad=True)
    w = torch.sigmoid(pr)
    y = (F.adaptive_max_pool2d(xr, (1, 1)) * w + F.adaptive_avg_pool2d(xr, (1, 1)) * (1 - w)).reshape(B, C)
    gy = torch.randn(B, C, generator=gen)
    y.backward(gy)
    xd = x.permute(0, 2, 3, 1).contiguous().to(device); pd = torch.tensor([p0], device=device)
    out = torch.empty(B, C, device=device); am = torch.empty(B, C, dtype=torch.int32, device=device)
    xmax, xavg = torch.empty_like(out), torch.empty_like(out)
    lib.mmpool_fwd(xd, pd, B, H * W, C, out, am, xmax, xavg)
    assert float((out.cpu() - y.detach()).abs().max()) <= 1e-5 * max(1.0, float(y.detach().abs().max())), "mmpool fwd"
    _, ref_idx = F.adaptive_max_pool2d(x, (1, 1), return_indices=True)
    assert torch.equal(am.cpu().long(), ref_idx.reshape(B, C)), "mmpool argmax (first maximum in scan order)"
    dx = torch.empty(B, H, W, C, device=device); dp = torch.full((1,), 0.25, device=device)
    lib.mmpool_bwd(gy.to(device), pd, am, xmax, xavg, B, H * W, C, dx, dp)
    refdx = xr.grad.permute(0, 2, 3, 1)
    assert float((dx.cpu() - refdx).abs().max()) <= 1e-6 + 1e-5 * float(refdx.abs().max()), "mmpool dx"
    assert abs(float(dp.cpu()) - 0.25 - float(pr.grad)) <= 1e-4 * max(1.0, abs(float(pr.grad))), "mmpool dp (accumulates)"


def bn_relu_maxpool_case(lib, device, N, H, W, C, seed=0):
    """hifihr_bn_relu_maxpool_{fwd,bwd} vs (a) the unfused kernels of the same library (forward: the same bits; backward: to the
    rounding of the slot atomics) and (b) plain PyTorch fp32 autograd of MaxPool2d(3, 2, 1)(relu(batch_norm(x)))."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    M = N * H * W
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn(N, C, H, W, generator=gen) * 1.5 + 0.3
    gamma = 1 + 0.1 * torch.randn(C, generator=gen); beta = 0.1 * torch.randn(C, generator=gen) - 0.3     # plenty of ReLU zeros: ties
    gamma[1] = 2e-4; beta[1] = 0.05                      # a near-zero scale (positive shift: every tap passes the ReLU)
    gamma[2] = -0.8                                      # a negative scale: the winner is the SMALLEST x of the window
    rm0, rv0 = torch.randn(C, generator=gen) * 0.1, 1 + 0.1 * torch.rand(C, generator=gen)
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    out = F.max_pool2d(F.relu(F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5)), 3, 2, 1)
    gy = torch.randn(out.shape, generator=gen)
    out.backward(gy)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(device)
    xd, gd, bd, gyd = nhwc(x), gamma.to(device), beta.to(device), nhwc(gy)
    assert lib.bn_relu_maxpool_supported(N, H, W, C)
    # fused
    stats = torch.zeros(lib.bn_stats_floats(C), device=device)
    lib.bn_stats(xd, M, C, stats)
    stats2 = stats.clone()
    y = torch.empty(N, OH, OW, C, device=device); tap = torch.empty(N * OH * OW * C, dtype=torch.uint8, device=device)
    sm = torch.empty(C, device=device); si = torch.empty(C, device=device)
    rmd, rvd = rm0.clone().to(device), rv0.clone().to(device)
    lib.bn_relu_maxpool_fwd(xd, stats, gd, bd, N, H, W, C, 1e-5, 0.1, y, tap, sm, si, rmd, rvd)
    assert float(stats.abs().max()) == 0.0, "bn_relu_maxpool_fwd must leave the slots and arrival counters zeroed"
    # unfused kernels of the same library
    yf = torch.empty(N, H, W, C, device=device); sm2 = torch.empty(C, device=device); si2 = torch.empty(C, device=device)
    lib.bn_act_fwd(xd, stats2, gd, bd, None, 1, M, C, 1e-5, 0.1, yf, sm2, si2, None, None)
    y2 = torch.empty_like(y); tap2 = torch.empty_like(tap)
    lib.maxpool2d_fwd(yf, N, H, W, C, 3, 2, 1, y2, tap2)
    assert torch.equal(sm, sm2) and torch.equal(si, si2), "fused stem: batch statistics"
    assert torch.equal(y, y2) and torch.equal(tap, tap2), "fused stem forward == bn_act_fwd + maxpool2d_fwd (bits, winning taps)"
    ref = out.detach().permute(0, 2, 3, 1)
    assert float((y.cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), "fused stem fwd vs torch"
    np.testing.assert_allclose(rmd.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rvd.cpu().numpy(), rv.numpy(), rtol=1e-4, atol=1e-6)
    # backward
    red = torch.zeros(lib.bn_stats_floats(C), device=device)
    dx = torch.full((N, H, W, C), 7.0, device=device)
    dg = torch.full((C,), 0.5, device=device); db = torch.full((C,), -0.25, device=device)
    lib.bn_relu_maxpool_bwd(gyd, tap, xd, sm, si, gd, bd, N, H, W, C, red, dx, dg, db)
    assert float(red.abs().max()) == 0.0, "bn_relu_maxpool_bwd must leave the slots and arrival counters zeroed"
    dyf = torch.empty(N, H, W, C, device=device)
    lib.maxpool2d_bwd(gyd, tap, N, H, W, C, 3, 2, 1, dyf)
    dx2 = torch.empty_like(dx); dg2 = torch.zeros(C, device=device); db2 = torch.zeros(C, device=device)
    lib.bn_act_bwd(dyf, None, xd, sm, si, gd, bd, 1, M, C, red, dx2, None, dg2, db2)
    scale = float(dx2.abs().max())
    assert float((dx - dx2).abs().max()) <= 2e-6 * scale + 1e-9, "fused stem backward vs maxpool2d_bwd + bn_act_bwd"
    assert float((dg - 0.5 - dg2).abs().max()) <= 1e-5 * float(dg2.abs().max()) + 1e-6
    assert float((db + 0.25 - db2).abs().max()) <= 1e-5 * float(db2.abs().max()) + 1e-6
    refdx = xr.grad.permute(0, 2, 3, 1)
    assert float((dx.cpu() - refdx).abs().max()) <= 2e-4 * float(refdx.abs().max()) + 1e-7, "fused stem dx vs torch"
    assert float((dg.cpu() - 0.5 - gr.grad).abs().max()) <= 2e-4 * float(gr.grad.abs().max()) + 1e-5
    assert float((db.cpu() + 0.25 - br.grad).abs().max()) <= 2e-4 * float(br.grad.abs().max()) + 1e-5
    # the same backward with the reduction walked over the POOLED grid (hifihr_bn_relu_maxpool_bwd_y: xhat of a window's winner recovered
    # from the pooled value; channels with |gamma| < 1e-3 -- channel 1 of this case -- gather the winner's x through the tap)
    dx3 = torch.full((N, H, W, C), 7.0, device=device)
    dg3 = torch.full((C,), 0.5, device=device); db3 = torch.full((C,), -0.25, device=device)
    lib.bn_relu_maxpool_bwd_y(gyd, y, tap, xd, sm, si, gd, bd, N, H, W, C, red, dx3, dg3, db3)
    assert float(red.abs().max()) == 0.0, "bn_relu_maxpool_bwd_y must leave the slots and arrival counters zeroed"
    assert float((dx3 - dx).abs().max()) <= 5e-6 * scale + 1e-9, "pooled-grid reduction vs the pass over x (dx)"
    assert float((dg3 - dg).abs().max()) <= 2e-5 * float(dg2.abs().max()) + 1e-6
    assert float((db3 - db).abs().max()) <= 2e-5 * float(db2.abs().max()) + 1e-6
    assert float((dx3.cpu() - refdx).abs().max()) <= 2e-4 * float(refdx.abs().max()) + 1e-7, "pooled-grid stem dx vs torch"
    assert float((dg3.cpu() - 0.5 - gr.grad).abs().max()) <= 2e-4 * float(gr.grad.abs().max()) + 1e-5


def maxpool_case(lib, device, N, H, W, C, seed=0, ties=False, ksp=(3, 2, 1)):
    """nn.MaxPool2d(k, s, p) forward / backward on NHWC."""
    k, s_, p_ = ksp
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen)
    if ties:
        x = torch.relu(x)                          # post-ReLU activations: many exact zeros tie inside a window
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, k, s_, p_)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    OH, OW = y.shape[2], y.shape[3]
    xd = x.permute(0, 2, 3, 1).contiguous().to(device)
    out = torch.empty(N, OH, OW, C, device=device); tap = torch.empty(N * OH * OW * C, dtype=torch.uint8, device=device)
    lib.maxpool2d_fwd(xd, N, H, W, C, k, s_, p_, out, tap)
    assert torch.equal(out.cpu(), y.detach().permute(0, 2, 3, 1)), "maxpool fwd (exact)"
    dx = torch.full((N, H, W, C), 7.0, device=device)          # overwritten, not accumulated
    lib.maxpool2d_bwd(gy.permute(0, 2, 3, 1).contiguous().to(device), tap, N, H, W, C, k, s_, p_, dx)
    refdx = xr.grad.permute(0, 2, 3, 1)
    # overlapping windows (stride < kernel): several gradients are summed per input pixel, in a different order than ATen
    assert float((dx.cpu() - refdx).abs().max()) <= 1e-6 + 2e-6 * float(refdx.abs().max()), "maxpool bwd"
    # the flattening form: y as the [N, C * OH * OW] matrix of `y.view(N, -1)` (NCHW order), gy likewise -- the same bits as the form above
    if hasattr(lib, "maxpool2d_fwd_flat"):
        flat = torch.full((N, C * OH * OW), 7.0, device=device); tap2 = torch.empty_like(tap)
        lib.maxpool2d_fwd_flat(xd, N, H, W, C, k, s_, p_, flat, tap2)
        assert torch.equal(flat.cpu(), y.detach().reshape(N, -1)) and torch.equal(tap2, tap), "maxpool fwd, flattened output"
        dx2 = torch.full((N, H, W, C), 7.0, device=device)
        lib.maxpool2d_bwd_flat(gy.reshape(N, -1).contiguous().to(device), tap2, N, H, W, C, k, s_, p_, dx2)
        assert torch.equal(dx2, dx), "maxpool bwd from the flattened gradient"


# ------------------------------------------------------------------------------------------------
# fused losses (csrc/losses.hip) vs the torch-op restatement in oracle/loss_oracle.py (pinned against the reference's
# own functions by tests/golden/losses.npz and loss_dict.npz in test_host_logic.py / test_oracle_losses.py)
# ------------------------------------------------------------------------------------------------
def vertex_face_csr(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1)
    order = np.argsort(f, kind="stable")
    off = np.zeros(V + 1, dtype=np.int32)
    np.add.at(off, f + 1, 1)
    return np.cumsum(off).astype(np.int32), ((order // 3) * 4 + (order % 3)).astype(np.int32)


def geom_loss_case(lib, device, B, V, F, mse, seed=0, J=21, NS=10, NP=48):
    import torch.nn.functional as Fn
    from oracle.loss_oracle import edge_length_loss
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    joints, jgt, verts, vgt = rnd(B, J, 3) * 0.05, rnd(B, J, 3) * 0.05, rnd(B, V, 3) * 0.05, rnd(B, V, 3) * 0.05
    shape, pose = rnd(B, NS), rnd(B, NP)
    faces = torch.stack([torch.randperm(V, generator=gen)[:3] for _ in range(F)]).int() if F else None
    lam = [1e4, 1e4, 1e2, 0.25, 0.5]
    base = Fn.mse_loss if mse else Fn.l1_loss
    jr, vr, sr, pr = (t.clone().requires_grad_(True) for t in (joints, verts, shape, pose))
    ref = [lam[0] * base(jr, jgt), lam[1] * base(vr, vgt),
           lam[2] * edge_length_loss(vr, vgt, faces.unsqueeze(0)) if F else torch.zeros(()),
           lam[3] * Fn.mse_loss(sr, torch.zeros_like(sr)), lam[4] * Fn.mse_loss(pr, torch.zeros_like(pr))]
    gout = torch.tensor([0.7, 1.3, 0.9, 1.1, 0.6])
    sum(g * r for g, r in zip(gout, ref)).backward()
    d = lambda t: t.to(device).contiguous() if t is not None else None
    partial = torch.empty(B * 5, device=device); out = torch.empty(5, device=device)
    args = (d(joints), d(jgt), d(verts), d(vgt), d(shape), d(pose), d(faces))
    lib.geom_loss_fwd(*args, mse, lam, partial, out)
    refv = torch.stack([r.detach() for r in ref])
    np.testing.assert_allclose(out.cpu().numpy(), refv.numpy(), rtol=2e-5, atol=1e-7)
    off, idx = vertex_face_csr(faces.numpy(), V) if F else (None, None)
    gj, gv, gs, gp = (torch.full(t.shape, 7.0, device=device) for t in (joints, verts, shape, pose))
    lib.geom_loss_bwd(*args, d(torch.from_numpy(off)) if F else None, d(torch.from_numpy(idx)) if F else None, mse, lam, d(gout), gj, gv, gs, gp)
    for got, want, name in ((gj, jr.grad, "joints"), (gv, vr.grad, "verts"), (gs, sr.grad, "shape"), (gp, pr.grad, "pose")):
        assert float((got.cpu() - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-9, f"geom loss grad {name}"


def light_split_case(lib, device, B=7, seed=0):
    """hifihr_light_split_fwd / _bwd vs torch: colors = hardtanh(lights[:, :3]), directions = lights[:, 3:] and their gradient, incl.
    values exactly at the clamp ends (gradient 0 there, as nn.Hardtanh) and absent gradients."""
    gen = torch.Generator().manual_seed(seed)
    l = (torch.randn(B, 6, generator=gen) * 1.5)
    l[0, 0] = 1.0; l[min(1, B - 1), 1] = -1.0
    l[B - 1, 2] = float("nan")                         # a NaN colour stays NaN and passes its gradient, exactly as torch's hardtanh
    l.requires_grad_(True)
    c = torch.nn.functional.hardtanh(l[:, :3]); dd = l[:, 3:]
    gc, gd = torch.randn(B, 3, generator=gen), torch.randn(B, 3, generator=gen)
    ((c * gc).sum() + (dd * gd).sum()).backward()
    ld = l.detach().to(device).contiguous()
    oc, od = torch.full((B, 3), 7.0, device=device), torch.full((B, 3), 7.0, device=device)
    lib.light_split_fwd(ld, oc, od)
    same = lambda a, b: bool(((a == b) | (a.isnan() & b.isnan())).all())
    assert same(oc.cpu(), c.detach()) and bool(oc.cpu()[B - 1, 2].isnan()) and torch.equal(od.cpu(), dd.detach().contiguous())
    gl = torch.full((B, 6), 7.0, device=device)
    lib.light_split_bwd(ld, gc.to(device), gd.to(device), gl)
    assert same(gl.cpu(), l.grad) and float(gl.cpu()[B - 1, 2]) == float(gc[B - 1, 2])
    lib.light_split_bwd(ld, None, gd.to(device), gl)
    assert float(gl.cpu()[:, :3].abs().max()) == 0.0 and torch.equal(gl.cpu()[:, 3:], gd)
    lib.light_split_bwd(ld, gc.to(device), None, gl)
    assert float(gl.cpu()[:, 3:].abs().max()) == 0.0


def loss_total_case(lib, device, seed=0):
    """hifihr_loss_total_fwd / _bwd: the sum of the leading entries of up to four small vectors, and its gradient (reference
    train_hrnet.py:98-104: loss = sum of the selected loss_dic entries)."""
    gen = torch.Generator().manual_seed(seed)
    parts = [torch.randn(5, generator=gen), torch.randn(4, generator=gen), torch.randn(1, generator=gen)]
    counts = [5, 3, 1]
    d = [p.to(device) for p in parts]
    total = torch.full((), 7.0, device=device)
    lib.loss_total_fwd(d, counts, total)
    want = sum(float(p[:n].double().sum()) for p, n in zip(parts, counts))
    assert abs(float(total) - want) <= 1e-6 * max(1.0, abs(want))
    g = torch.tensor(1.75, device=device)
    grads = [torch.full_like(p, 9.0) for p in d]
    lib.loss_total_bwd(g, grads, counts)
    for gr, n in zip(grads, counts):
        assert torch.equal(gr.cpu()[:n], torch.full((n,), 1.75)) and float(gr.cpu()[n:].abs().sum()) == 0.0
    one = torch.randn(1, generator=gen).to(device)
    lib.loss_total_fwd([one], [1], total)
    assert float(total) == float(one)


def photo_loss_case(lib, device, B, H, W, seed=0, with_g=True):
    import torch.nn.functional as Fn
    gen = torch.Generator().manual_seed(seed)
    rgba = torch.rand(B, 4, H, W, generator=gen)
    rgba[:, 3] = torch.where(torch.rand(B, H, W, generator=gen) > 0.5, rgba[:, 3], torch.zeros(B, H, W))     # holes: alpha == 0
    imgs = torch.rand(B, 3, H, W, generator=gen)
    seg = (torch.rand(B, H, W, generator=gen) > 0.4).long()
    l_tex, l_mrgb, l_sil = 0.005, 0.005, 0.1
    rr = rgba.clone().requires_grad_(True)
    re_sil = rr[:, 3:4].detach()
    re_sil = torch.where(re_sil > 0, torch.full_like(re_sil, 255.0), re_sil)
    segf = seg.unsqueeze(1).float()
    mask_rgbs = segf * imgs
    re_img = rr[:, :3] * (re_sil / 255.0)
    tex = l_tex * Fn.l1_loss(re_img, mask_rgbs)
    mrgb = l_mrgb * Fn.mse_loss(torch.mean(mask_rgbs), torch.mean(re_img))
    sil = l_sil * Fn.l1_loss(re_sil, segf)
    g_re = torch.randn(B, 3, H, W, generator=gen) * 1e-6 if with_g else None
    gout = torch.tensor([0.8, 1.7, 0.0, 0.0])
    tot = gout[0] * tex + gout[1] * mrgb
    if with_g:
        tot = tot + (re_img * g_re).sum()
    tot.backward()
    d = lambda t: t.to(device).contiguous() if t is not None else None
    rd, idd, sd = d(rgba), d(imgs), d(seg)
    re_m = torch.empty(B, 3, H, W, device=device); mk = torch.empty_like(re_m)
    partial = torch.empty(lib.photo_loss_partial_floats(), device=device); out = torch.empty(4, device=device)
    lib.photo_loss_fwd(rd, idd, sd, l_tex, l_mrgb, l_sil, re_m, mk, partial, out)
    assert float((re_m.cpu() - re_img.detach()).abs().max()) <= 1e-6 and torch.equal(mk.cpu(), mask_rgbs)
    want = torch.stack([tex.detach(), mrgb.detach(), sil, (re_img.mean() - mask_rgbs.mean()).detach()])
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=3e-5, atol=1e-9)
    grad = torch.full((B, 4, H, W), 7.0, device=device)
    lib.photo_loss_bwd(rd, re_m, mk, d(g_re), d(gout), out, l_tex, l_mrgb, grad)
    assert float((grad.cpu() - rr.grad).abs().max()) <= 2e-5 * float(rr.grad.abs().max()) + 1e-12, "photo loss grad"
    rs = torch.empty(B, 1, H, W, device=device); mrgbs = torch.empty(B, 3, H, W, device=device)
    lib.sil_post(rd, idd, rs, mrgbs)
    assert torch.equal(rs.cpu(), re_sil) and torch.equal(mrgbs.cpu(), imgs * (re_sil > 0).float())


# ------------------------------------------------------------------------------------------------
# small-batch fully connected layer (csrc/mlp.hip) vs nn.Linear (+ BatchNorm1d training mode) (+ ReLU)
# ------------------------------------------------------------------------------------------------
def linear_case(lib, device, B, I, O, act, bn, seed=0, need_dx=True):
    import torch.nn.functional as Fn
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x, w, b = rnd(B, I), rnd(O, I) / I ** 0.5, rnd(O) * 0.1
    gamma, beta = 1 + 0.2 * rnd(O), 0.1 * rnd(O)
    rm0, rv0 = 0.1 * rnd(O), 1 + 0.1 * torch.rand(O, generator=gen)
    xr, wr, br, gr, ber = (t.clone().requires_grad_(True) for t in (x, w, b, gamma, beta))
    rm, rv = rm0.clone(), rv0.clone()
    out = Fn.linear(xr, wr, br)
    if bn:
        out = Fn.batch_norm(out, rm, rv, gr, ber, training=True, momentum=0.1, eps=1e-5)
    if act:
        out = Fn.relu(out)
    gy = rnd(B, O)
    out.backward(gy)
    d = lambda t: t.to(device).contiguous()
    xd, wd, bd = d(x), d(w), d(b)
    y = torch.empty(B, O, device=device)
    bnf = bnb = None
    if bn:
        z, sm, si = torch.empty(B, O, device=device), torch.empty(O, device=device), torch.empty(O, device=device)
        rmd, rvd = d(rm0), d(rv0)
        bnf = (d(gamma), d(beta), 1e-5, 0.1, rmd, rvd, z, sm, si)
    lib.linear_fwd(xd, wd, bd, act, y, bnf)
    tol = 3e-5 * max(1.0, float(out.detach().abs().max()))
    assert float((y.cpu() - out.detach()).abs().max()) <= tol, "linear fwd"
    if bn:
        np.testing.assert_allclose(rmd.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rvd.cpu().numpy(), rv.numpy(), rtol=1e-4, atol=1e-6)
    dz = torch.empty(B, O, device=device)
    dW = torch.full((O, I), 0.5, device=device); db = torch.full((O,), -0.25, device=device)       # accumulate semantics
    dx = torch.full((B, I), 7.0, device=device) if need_dx else None                               # overwritten
    if bn:
        dg, dbt = torch.full((O,), 0.125, device=device), torch.full((O,), 2.0, device=device)
        bnb = (bnf[0], z, sm, si, dg, dbt)
    lib.linear_bwd(d(gy), y if act else None, xd, wd, act, dz, dW, db, dx, bnb)
    rel = lambda got, want, name, t=2e-4: (float((got.cpu() - want).abs().max()) <= t * float(want.abs().max()) + 1e-6) or \
        (_ for _ in ()).throw(AssertionError(f"linear {name}: {float((got.cpu() - want).abs().max())} vs {float(want.abs().max())}"))
    rel(dW - 0.5, wr.grad, "dW")
    if bn:       # the true bias gradient under batch-norm is zero (the batch mean removes it): absolute check
        assert float((db.cpu() + 0.25).abs().max()) <= 1e-4, "linear db (batch-norm: ~0)"
    else:
        rel(db + 0.25, br.grad, "db")
    if need_dx:
        rel(dx, xr.grad, "dx")
    if bn:
        rel(dg - 0.125, gr.grad, "dgamma")
        rel(dbt - 2.0, ber.grad, "dbeta")


def conv_relu_nobias_case(lib, device, N, H, W, C, K, R, stride, seed=0, pad=0):
    """hifihr_conv2d_fwd(bias = NULL, act = 1): the output is clamped whatever kernel the shape dispatches to (the 1x1 / stride-1
    shapes with K % 128 == 0 once took the GEMM kernels, which have no activation epilogue: round-2 advisor finding)."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen); w = torch.randn(K, C, R, R, generator=gen) / (C * R * R) ** 0.5
    ref = F.relu(F.conv2d(x, w, None, stride=stride, padding=pad)).permute(0, 2, 3, 1)
    d = lambda t: t.to(device).contiguous()
    out = torch.full(tuple(ref.shape), -3.0, device=device)
    lib.conv2d_fwd(d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), None, out, N, H, W, C, K, R, R, stride, pad, act=1)
    assert float(out.min()) >= 0.0, "ReLU epilogue dropped"
    assert float((out.cpu() - ref).abs().max()) <= 3e-5 * float(ref.abs().max()) + 1e-6, "conv+relu fwd"


def conv_wino2_case(lib, device, N, H, W, seed=0, bias_relu=False, rtol=2e-5):
    """hifihr_conv3x3_c64_wino (conv_wino2_kernel: 64 -> 64, 3x3 / stride 1 / pad 1 as Winograd F(2x2, 3x3) with the transforms in registers)
    vs F.conv2d: forward (+ bias + ReLU, + batch-norm statistics slots) and backward-data through U' of the transposed, rotated filter."""
    import torch.nn.functional as F
    assert lib.conv3x3_c64_wino_supported(N, H, W, 64, 64)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 64, H, W, generator=gen) + 0.5
    w = torch.randn(64, 64, 3, 3, generator=gen) / 24.0
    b = torch.randn(64, generator=gen) * 0.3 if bias_relu else None
    xr = x.clone().requires_grad_(True)
    z = F.conv2d(xr, w, b, padding=1)
    y = F.relu(z) if bias_relu else z
    gy = torch.randn(z.shape, generator=gen)
    z.backward(gy)
    d = lambda t: t.to(device).contiguous()
    w_krsc = d(w.permute(0, 2, 3, 1))
    U = torch.empty(16 * 64 * 64, device=device)
    lib.wino_weight_transform(w_krsc, U, 64, 64, 0)
    out = torch.full((N, H, W, 64), 7.0, device=device)
    stats = None if bias_relu else torch.zeros(lib.bn_stats_floats(64), device=device)
    lib.conv3x3_c64_wino(d(x.permute(0, 2, 3, 1)), U, d(b) if bias_relu else None, bias_relu, out, stats, N, H, W)
    ref = y.detach().permute(0, 2, 3, 1)
    err = float((out.cpu() - ref).abs().max())
    assert err <= rtol * float(ref.abs().max()) + 1e-6, f"wino2 conv fwd: {err}"
    if stats is not None:
        sl = bn_slots(stats.cpu(), 64).sum(0)
        r2 = ref.double().reshape(-1, 64)
        assert float((sl[0] - r2.sum(0)).abs().max()) <= 2e-5 * float(r2.abs().sum(0).max()), "wino2 conv: channel sums"
        assert float((sl[1] - (r2 * r2).sum(0)).abs().max()) <= 2e-5 * float((r2 * r2).sum(0).max()), "wino2 conv: channel sums of squares"
    if not bias_relu:
        # backward-data: U' from the [C][R][S][K] transpose with flip (what hifihr_weight_prep kind 2 produces from w directly)
        wt = d(w.permute(1, 2, 3, 0))
        U2 = torch.empty(16 * 64 * 64, device=device)
        lib.wino_weight_transform(wt, U2, 64, 64, 1)
        dx = torch.full((N, H, W, 64), 7.0, device=device)
        lib.conv3x3_c64_wino(d(gy.permute(0, 2, 3, 1)), U2, None, False, dx, None, N, H, W)
        refx = xr.grad.permute(0, 2, 3, 1)
        err = float((dx.cpu() - refx).abs().max())
        assert err <= rtol * float(refx.abs().max()) + 1e-6, f"wino2 conv bwd data: {err}"


def conv_c64_bwd_pair_case(lib, device, N, H, W, seed=0, with_res=False):
    """hifihr_conv3x3_c64_bwd_pair (conv_c64_bwd_pair_kernel: data gradient + weight gradient of a 64 -> 64 3x3 layer in one launch) vs the two
    separate calls it replaces: dx bit for bit (every output element is computed the same way whatever the workgroup's share), dw within
    the summation-order difference of the slab split and equal to itself on a second launch; both vs F.conv2d's gradients."""
    import torch.nn.functional as F
    assert lib.conv3x3_c64_bwd_pair_supported(N, H, W)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 64, H, W, generator=gen) + 0.5
    w = torch.randn(64, 64, 3, 3, generator=gen) / 24.0
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, None, padding=1)
    gy = torch.randn(z.shape, generator=gen)
    z.backward(gy)
    res = torch.randn(N, H, W, 64, generator=gen) if with_res else None
    d = lambda t: t.to(device).contiguous()
    U2 = torch.empty(16 * 64 * 64, device=device)
    lib.wino_weight_transform(d(w.permute(1, 2, 3, 0)), U2, 64, 64, 1)
    x_d, gy_d = d(x.permute(0, 2, 3, 1)), d(gy.permute(0, 2, 3, 1))
    res_d = d(res) if with_res else None
    dx0 = torch.full((N, H, W, 64), 7.0, device=device)
    if with_res:
        lib.conv3x3_c64_wino_res(gy_d, U2, res_d, dx0, N, H, W)
    else:
        lib.conv3x3_c64_wino(gy_d, U2, None, False, dx0, None, N, H, W)
    dw0 = torch.full((64, 3, 3, 64), 0.25, device=device)
    lib.conv2d_bwd_weight(x_d, gy_d, dw0, N, H, W, 64, 64, 3, 3, 1, 1)
    outs = []
    for _ in range(2):
        dx = torch.full((N, H, W, 64), 7.0, device=device); dw = torch.full((64, 3, 3, 64), 0.25, device=device)
        lib.conv3x3_c64_bwd_pair(gy_d, U2, res_d, dx, x_d, dw, N, H, W)
        outs.append((dx, dw))
    assert torch.equal(outs[0][0], dx0), "pair: dx differs from the separate launch"
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "pair: not bit-reproducible"
    refw = wr.grad.permute(0, 2, 3, 1)
    err = float((outs[0][1].cpu() - 0.25 - refw).abs().max())
    assert err <= 2e-4 * float(refw.abs().max()) + 1e-6, f"pair: dw vs torch {err}"
    err0 = float((outs[0][1] - dw0).abs().max())
    assert err0 <= 2e-5 * float(refw.abs().max()) + 1e-6, f"pair: dw vs the separate launch {err0}"
    refx = xr.grad.permute(0, 2, 3, 1) + (res if with_res else 0.0)
    err = float((outs[0][0].cpu() - refx).abs().max())
    assert err <= 2e-5 * float(refx.abs().max()) + 1e-6, f"pair: dx vs torch {err}"
    # the same launch with the slab sum left to hifihr_conv_halo_wgrad_reduce_multi (the step's deferred form): two "layers" in one reduce launch,
    # each bit-identical to the sum the pair call makes itself
    nb = lib.conv2d_wgrad_workspace_bytes(N, H, W, 64, 64, 3, 3, 1, 1)
    jobs, dxs = [], []
    for rep in range(2):
        slabs = torch.full(((nb + 3) // 4,), float("nan"), device=device)
        dx = torch.full((N, H, W, 64), 7.0, device=device); dw = torch.full((64, 3, 3, 64), 0.25, device=device)
        ns = lib.conv3x3_c64_bwd_pair_slabs(gy_d, U2, res_d, dx, x_d, slabs, N, H, W)
        assert ns > 0
        jobs.append((slabs, ns, dw)); dxs.append(dx)
    lib.conv_halo_wgrad_reduce_multi(jobs)
    for (slabs, ns, dw), dx in zip(jobs, dxs):
        assert torch.equal(dx, outs[0][0]) and torch.equal(dw, outs[0][1]), "deferred slab sum differs from the pair call's own"


def conv_bias_relu_case(lib, device, N, H, W, C, K, R, stride, seed=0, pad=0):
    """conv + bias + ReLU in one launch (act = 1) and its backward prologue bias_relu_bwd, vs torch."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen); w = torch.randn(K, C, R, R, generator=gen) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=gen) * 0.3
    br = b.clone().requires_grad_(True)
    z = F.conv2d(x, w, br, stride=stride, padding=pad)
    z.retain_grad()
    y = F.relu(z)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    OH, OW = y.shape[2], y.shape[3]
    d = lambda t: t.to(device).contiguous()
    out = torch.empty(N, OH, OW, K, device=device)
    lib.conv2d_fwd(d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), d(b), out, N, H, W, C, K, R, R, stride, pad, act=1)
    ref = y.detach().permute(0, 2, 3, 1)
    assert float((out.cpu() - ref).abs().max()) <= 3e-5 * float(ref.abs().max()) + 1e-6, "conv+bias+relu fwd"
    g = torch.full_like(out, 7.0); db = torch.full((K,), 0.5, device=device)
    lib.bias_relu_bwd(d(gy.permute(0, 2, 3, 1)), out, N * OH * OW, K, g, db)
    # the mask comes from OUR y (elements within rounding of 0 may differ from torch's): compare where |z| is not tiny
    zr = z.detach().permute(0, 2, 3, 1)
    safe = zr.abs() > 1e-5
    refg = z.grad.permute(0, 2, 3, 1)
    assert float(((g.cpu() - refg) * safe).abs().max()) <= 1e-6, "masked gradient"
    assert float((db.cpu() - 0.5 - br.grad).abs().max()) <= 1e-4 * float(br.grad.abs().max()) + 1e-5, "bias gradient (accumulates)"


# ------------------------------------------------------------------------------------------------
# squeeze-and-excitation (csrc/se.hip + the linear kernels with swish / sigmoid epilogues) vs torch autograd
# ------------------------------------------------------------------------------------------------
def se_case(lib, device, B, H, W, C, SQ, seed=0):
    import torch.nn.functional as Fn
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x = rnd(B, C, H, W); w1 = rnd(SQ, C) / C ** 0.5; b1 = rnd(SQ) * 0.1; w2 = rnd(C, SQ) / SQ ** 0.5; b2 = rnd(C) * 0.1
    xr, w1r, b1r, w2r, b2r = (t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2))
    m = xr.mean((2, 3))
    z1 = Fn.linear(m, w1r, b1r)
    h1 = z1 * torch.sigmoid(z1)
    gate = torch.sigmoid(Fn.linear(h1, w2r, b2r))
    y = xr * gate[:, :, None, None]
    gy = rnd(B, C, H, W)
    y.backward(gy)
    d = lambda t: t.to(device).contiguous()
    HW = H * W
    xd = d(x.permute(0, 2, 3, 1)); gyd = d(gy.permute(0, 2, 3, 1))
    mean = torch.zeros(B, C, device=device)
    lib.se_pool(xd, B, HW, C, mean)
    assert float((mean.cpu() - m.detach()).abs().max()) <= 1e-5, "se pool"
    h1d, z1d, gd = torch.empty(B, SQ, device=device), torch.empty(B, SQ, device=device), torch.empty(B, C, device=device)
    w1d, b1d, w2d, b2d = d(w1), d(b1), d(w2), d(b2)
    lib.linear_fwd(mean, w1d, b1d, 2, h1d, z=z1d)
    lib.linear_fwd(h1d, w2d, b2d, 3, gd)
    assert float((gd.cpu() - gate.detach()).abs().max()) <= 2e-5, "se gate"
    yd = torch.empty(B, H, W, C, device=device)
    lib.se_scale(xd, gd, None, 0.0, B, HW, C, yd)
    ref = y.detach().permute(0, 2, 3, 1)
    assert float((yd.cpu() - ref).abs().max()) <= 3e-5 * float(ref.abs().max()), "se fwd"
    dgate = torch.zeros(B, C, device=device)
    lib.se_bwd_gate(gyd, xd, B, HW, C, dgate)
    dw1, db1, dw2, db2 = (torch.zeros_like(t) for t in (w1d, b1d, w2d, b2d))
    dh1, dmean = torch.empty(B, SQ, device=device), torch.empty(B, C, device=device)
    dz2, dz1 = torch.empty(B, C, device=device), torch.empty(B, SQ, device=device)
    lib.linear_bwd(dgate, gd, h1d, w2d, 3, dz2, dw2, db2, dh1)
    lib.linear_bwd(dh1, None, mean, w1d, 2, dz1, dw1, db1, dmean, z=z1d)
    dx = torch.empty(B, H, W, C, device=device)
    lib.se_scale(gyd, gd, dmean, 1.0 / HW, B, HW, C, dx)
    def rel(got, want, name, t=3e-4):
        err, mag = float((got.cpu() - want).abs().max()), float(want.abs().max())
        assert err <= t * mag + 1e-7, f"se {name}: {err} vs {mag}"
    rel(dx, xr.grad.permute(0, 2, 3, 1), "dx")
    rel(dw1, w1r.grad, "dw1"); rel(db1, b1r.grad, "db1"); rel(dw2, w2r.grad, "dw2"); rel(db2, b2r.grad, "db2")
    # ---- the two layers fused (se_mlp_fwd / se_mlp_bwd): same numbers, accumulators handed back zeroed, gradients ACCUMULATED
    assert lib.se_mlp_supported(C, SQ)
    acc = torch.zeros(B, C, device=device)
    lib.se_pool(xd, B, HW, C, acc)
    w2t = d(w2.t())
    mean2, z2, h2, g2 = torch.empty(B, C, device=device), torch.empty(B, SQ, device=device), torch.empty(B, SQ, device=device), torch.empty(B, C, device=device)
    lib.se_mlp_fwd(acc, w1d, b1d, w2t, b2d, B, C, SQ, mean2, z2, h2, g2)
    assert float(acc.abs().max()) == 0.0, "se_mlp_fwd hands the accumulator back zeroed"
    assert float((mean2.cpu() - m.detach()).abs().max()) <= 1e-5 and float((g2.cpu() - gate.detach()).abs().max()) <= 2e-5, "fused se gate"
    assert float((z2.cpu() - z1.detach()).abs().max()) <= 2e-5 and float((h2.cpu() - h1.detach()).abs().max()) <= 2e-5
    dacc = torch.zeros(B, C, device=device)
    lib.se_bwd_gate(gyd, xd, B, HW, C, dacc)
    pre = 0.25                                                    # the gradient buffers already hold something: += semantics
    fw1, fb1, fw2, fb2 = (torch.full_like(t, pre) for t in (w1d, b1d, w2d, b2d))
    dz2f, dz1f, dmeanf = torch.empty(B, C, device=device), torch.empty(B, SQ, device=device), torch.empty(B, C, device=device)
    lib.se_mlp_bwd(dacc, g2, z2, h2, mean2, w1d, w2t, B, C, SQ, dz2f, dz1f, dmeanf, fw1, fb1, fw2, fb2)
    assert float(dacc.abs().max()) == 0.0, "se_mlp_bwd hands the accumulator back zeroed"
    dx2 = torch.empty(B, H, W, C, device=device)
    lib.se_scale(gyd, g2, dmeanf, 1.0 / HW, B, HW, C, dx2)
    rel(dx2, xr.grad.permute(0, 2, 3, 1), "fused dx")
    rel(fw1 - pre, w1r.grad, "fused dw1"); rel(fb1 - pre, b1r.grad, "fused db1"); rel(fw2 - pre, w2r.grad, "fused dw2"); rel(fb2 - pre, b2r.grad, "fused db2")


# ------------------------------------------------------------------------------------------------
# Winograd F(2x2, 3x3) path (csrc/wino.hip + the batched MFMA GEMM) vs torch conv2d, forward and backward-data
# ------------------------------------------------------------------------------------------------
def wino4_dw_multi_case(lib, device, seed=0):
    """hifihr_wino4_dw_transform_multi: the F(4x4) weight-gradient transforms of several layers in one launch == one
    hifihr_wino_dw_transform_parts(..., 4) call per layer, bit for bit (same per-item arithmetic, slabs in slab order) -- wide-form layers
    (<= 8 192 items), item-per-thread layers, 1 .. 7 slabs, a layer whose item count is not a multiple of the workgroup's, accumulation
    into non-zero targets; more jobs than one launch's argument block holds (24)."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(64, 64, 3), (128, 128, 7), (256, 128, 1), (72, 100, 2), (264, 128, 2)] + [(16, 8 + 4 * i, 1 + i % 3) for i in range(22)]
    jobs, want = [], []
    for K, C, parts in shapes:
        dU = torch.randn(parts * 36 * K * C, generator=gen).to(device)
        base = torch.randn(K * 9 * C, generator=gen).to(device)
        single = base.clone()
        lib.wino_dw_transform_parts(dU, parts, single, K, C, 4)
        tgt = base.clone()
        jobs.append((dU, parts, tgt, K, C)); want.append(single)
    lib.wino4_dw_transform_multi(jobs)
    for (dU, parts, tgt, K, C), single in zip(jobs, want):
        assert torch.equal(tgt, single), (K, C, parts, float((tgt - single).abs().max()))


def wino_case(lib, device, N, H, W, C, K, seed=0, with_stats=True, use_ws=True, m=2):
    """m = 2: F(2x2, 3x3) (csrc/wino.hip, 16 positions); m = 4: F(4x4, 3x3) (csrc/wino4.hip, 36 positions, slab backward-weight only)."""
    P = (m + 2) ** 2
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen); w = torch.randn(K, C, 3, 3, generator=gen) / (9 * C) ** 0.5
    xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, 1, 1)
    gy = torch.randn(y.shape, generator=gen)
    y.backward(gy)
    d = lambda t: t.to(device).contiguous()
    T = lib.wino_tiles(N, H, W, m)               # (the library's count: 16 images share a mosaic of tiles at m = 4, H % 4 in {1, 2})
    xd, wd, gyd = d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), d(gy.permute(0, 2, 3, 1))
    nb = max(lib.wino_gemm_workspace_bytes(N, H, W, C, K, m), lib.wino_gemm_workspace_bytes(N, H, W, K, C, m)) if use_ws else 0
    ws = torch.zeros(nb // 4, device=device) if nb else None
    # forward
    U = torch.empty(P, K, C, device=device); V = torch.empty(P, T, C, device=device); M = torch.empty(P, T, K, device=device)
    out = torch.full((N, H, W, K), 7.0, device=device)
    stats = torch.zeros(lib.bn_stats_floats(K), device=device) if with_stats else None
    lib.wino_weight_transform(wd, U, K, C, 0, m)
    lib.wino_input_transform(xd, V, N, H, W, C, m)
    lib.wino_gemm(V, U, M, N, H, W, C, K, ws=ws, m=m)
    lib.wino_output_transform(M, out, stats, N, H, W, K, m=m)
    ref = y.detach().permute(0, 2, 3, 1)
    err = float((out.cpu() - ref).abs().max())
    # F(4x4, 3x3) in fp32: 8-9e-6 of max |y| typical (profiles/r02_wino43_error.txt), 2.0e-5 at 512 x 512 channels (4 608-term sums;
    # flake check of round 5): the bound leaves a factor 2.5 over the worst shape.  F(2x2): ~1e-6.
    wtol = 5e-5 if m == 4 else 3e-5
    assert err <= wtol * float(ref.abs().max()) + 1e-6, f"winograd fwd: {err} vs {float(ref.abs().max())}"
    if with_stats:
        st = bn_slots(stats, K).sum(0).cpu(); flat = ref.reshape(-1, K)
        np.testing.assert_allclose(st[0].numpy(), flat.sum(0).numpy(), rtol=1e-4, atol=2e-3)
        np.testing.assert_allclose(st[1].numpy(), (flat ** 2).sum(0).numpy(), rtol=1e-4, atol=2e-3)
    # bias (+ ReLU) epilogue of the output transform (VGG19 layers): same M
    bias = torch.randn(K, generator=gen) * 0.3
    for act in (0, 1):
        out2 = torch.full((N, H, W, K), 7.0, device=device)
        lib.wino_output_transform(M, out2, None, N, H, W, K, bias=d(bias), act=act, m=m)
        ref2 = ref + bias
        ref2 = F.relu(ref2) if act else ref2
        assert float((out2.cpu() - ref2).abs().max()) <= wtol * float(ref.abs().max()) + 1e-6, f"winograd bias/act epilogue (act={act})"
    # backward-data: the same pipeline on dy with the transposed, rotated filter
    wt = torch.empty(C, 3, 3, K, device=device)
    lib.weight_transpose(wd, wt, K, 9, C)
    U2 = torch.empty(P, C, K, device=device); V2 = torch.empty(P, T, K, device=device); M2 = torch.empty(P, T, C, device=device)
    dx = torch.full((N, H, W, C), 7.0, device=device)
    lib.wino_weight_transform(wt, U2, C, K, 1, m)
    lib.wino_input_transform(gyd, V2, N, H, W, K, m)
    # one read of dy for both backward transforms == the two separate kernels, bit for bit
    V2b = torch.full_like(V2, 7.0); Ytb = torch.full((P, T, K), 7.0, device=device); Yt_ref = torch.empty(P, T, K, device=device)
    lib.wino_input_dy_transform(gyd, V2b, Ytb, N, H, W, K, m)
    lib.wino_dy_transform(gyd, Yt_ref, N, H, W, K, m)
    assert torch.equal(V2b, V2) and torch.equal(Ytb, Yt_ref), "dual dy transform"
    lib.wino_gemm(V2, U2, M2, N, H, W, K, C, ws=ws, m=m)
    lib.wino_output_transform(M2, dx, None, N, H, W, C, m=m)
    refx = xr.grad.permute(0, 2, 3, 1)
    err = float((dx.cpu() - refx).abs().max())
    assert err <= wtol * float(refx.abs().max()) + 1e-6, f"winograd bwd data: {err} vs {float(refx.abs().max())}"
    assert ws is None or float(ws.abs().max()) == 0.0
    # backward-weight: dU = sum over tiles of (A dy A^T) . (B^T d B), then dw += G^T dU G
    lib.wino_input_transform(xd, V, N, H, W, C, m)
    Yt = torch.empty(P, T, K, device=device); dU = torch.zeros(P, K, C, device=device)
    lib.wino_dy_transform(gyd, Yt, N, H, W, K, m)
    refw = wr.grad.permute(0, 2, 3, 1)
    if m == 2:                                                           # the atomics form exists for F(2x2, 3x3) only
        lib.wino_wgrad_gemm(V, Yt, dU, N, H, W, C, K)
        dw = torch.full((K, 3, 3, C), 0.5, device=device)                # accumulate semantics
        lib.wino_dw_transform(dU, dw, K, C)
        assert float(dU.abs().max()) == 0.0, "the dU accumulator must come back zeroed"
        err = float((dw.cpu() - 0.5 - refw).abs().max())
        assert err <= 1e-4 * float(refw.abs().max()) + 1e-6, f"winograd bwd weight: {err} vs {float(refw.abs().max())}"
    # the same reduction as slabs on csrc/gemm.hip (no atomics, nothing zero-initialised), summed by the slab form of the transform
    parts = lib.wino_wgrad_parts(N, H, W, C, K, m)
    assert m == 2 or parts > 0
    if parts > 0:
        dUp = torch.full((parts, P, K, C), 7.0, device=device)
        lib.wino_wgrad_gemm_parts(V, Yt, dUp, N, H, W, C, K, parts, m)
        dw2 = torch.full((K, 3, 3, C), 0.5, device=device)
        lib.wino_dw_transform_parts(dUp, parts, dw2, K, C, m)
        err = float((dw2.cpu() - 0.5 - refw).abs().max())
        assert err <= 1e-4 * float(refw.abs().max()) + 1e-6, f"winograd bwd weight (slabs): {err} vs {float(refw.abs().max())}"
        if m == 4 and C % 64 == 0 and K % 64 == 0:
            # the two backward products in ONE launch (hifihr_wino4_bwd_gemm_pair): the same bits as the two separate launches
            M2p = torch.full_like(M2, 7.0); dUq = torch.full_like(dUp, 7.0)
            lib.wino4_bwd_gemm_pair(V2, U2, M2p, V, Yt, dUq, N, H, W, C, K, parts)
            M2s = torch.full_like(M2, 7.0)
            lib.wino_gemm(V2, U2, M2s, N, H, W, K, C, ws=None, m=m)            # (same kernel family as the pair: no balanced-schedule workspace)
            Tr = lib.wino_tiles_computed(N, H, W, m)                            # (rows behind the last mosaic tile are padding: never written)
            assert torch.equal(M2p[:, :Tr], M2s[:, :Tr]), "pair launch: backward-data product"
            assert torch.equal(dUq, dUp), "pair launch: backward-weight slabs"
    return 0 if ws is None else 1


def bgemm_case(lib, device, M, N, K, batch, seed=0):
    """csrc/gemm.hip through the C ABI vs torch matmul (fp64 reference): NT (c = a b^T) and TN (slabs of a^T b)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(batch, M, K, generator=gen); b = torch.randn(batch, N, K, generator=gen)
    c = torch.full((batch, M, N), 7.0, device=device)
    nb = lib.bgemm_nt_workspace_bytes(M, N, K, batch)          # > 0: the persistent, balanced kernel (zero-initialised, self-cleaning)
    ws = torch.zeros(nb // 4, device=device) if nb else None
    ad, bd = a.to(device).contiguous(), b.to(device).contiguous()
    ref = torch.matmul(a.double(), b.double().transpose(1, 2))
    for rep in range(2 if nb else 1):                         # twice on the same workspace: it must come back clean
        c.fill_(7.0)
        lib.bgemm_nt(ad, bd, c, M, N, K, batch, ws=ws)
        err = float((c.cpu().double() - ref).abs().max())
        assert err <= 2e-6 * K ** 0.5 * float(ref.abs().max()) + 1e-6, f"bgemm_nt {M}x{N}x{K}x{batch} (rep {rep}, ws {nb}): {err}"
        assert ws is None or float(ws.abs().max()) == 0.0, "workspace not handed back clean"
    return nb


def bgemm_tn_case(lib, device, M, N, T, batch, seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(batch, T, M, generator=gen); b = torch.randn(batch, T, N, generator=gen)
    parts = lib.bgemm_tn_parts(M, N, T, batch)
    assert parts >= 1
    cp = torch.full((parts, batch, M, N), 7.0, device=device)
    lib.bgemm_tn(a.to(device).contiguous(), b.to(device).contiguous(), cp, M, N, T, batch, parts)
    ref = torch.matmul(a.double().transpose(1, 2), b.double())
    err = float((cp.cpu().double().sum(0) - ref).abs().max())
    assert err <= 2e-6 * T ** 0.5 * float(ref.abs().max()) + 1e-6, f"bgemm_tn {M}x{N}x{T}x{batch} ({parts} parts): {err}"
    return parts


# ------------------------------------------------------------------------------------------------
# evaluation: batched Procrustes-with-scale alignment (csrc/eval.hip) vs the reference's align_w_scale vectors
# ------------------------------------------------------------------------------------------------
def procrustes_case(lib, device, golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "eval.npz"))
    for pr, gt, al, key in ((g["pr_j"], g["gt_j"], g["al_j"], "mpjpe"), (g["pr_v"], g["gt_v"], g["al_v"], "mpvpe")):
        pred = torch.from_numpy(pr).float().to(device).contiguous(); gtt = torch.from_numpy(gt).float().to(device).contiguous()
        aligned = torch.full_like(pred, 7.0); err = torch.full((pred.shape[0],), 7.0, device=device)
        lib.procrustes_error(pred, gtt, aligned, err)
        np.testing.assert_allclose(aligned.cpu().numpy(), al, atol=2e-7, rtol=0)     # metres; fp32 storage of ~0.1 m values
        got = float(err.sum()) / (pred.shape[0] * pred.shape[1])
        assert abs(got - float(g[key])) <= 1e-6 * float(g[key]), (key, got, float(g[key]))
        err2 = torch.full((pred.shape[0],), 7.0, device=device)
        lib.procrustes_error(pred, gtt, None, err2)                                  # error only
        assert torch.equal(err, err2)
    # properties: a similarity transform (incl. a reflection) of the ground truth aligns back exactly; coplanar input is finite
    gen = torch.Generator().manual_seed(3)
    gt = torch.randn(4, 50, 3, generator=gen) * 0.05
    q, _ = torch.linalg.qr(torch.randn(4, 3, 3, generator=gen))
    pred = 1.7 * gt @ q.transpose(1, 2) + torch.randn(4, 1, 3, generator=gen)
    flat = gt.clone(); flat[3, :, 2] = 0.0; pflat = pred.clone(); pflat[3] = flat[3] * 2.0 + 0.3
    for p_, g_ in ((pred, gt), (pflat, flat)):
        aligned = torch.empty(4, 50, 3, device=device); err = torch.empty(4, device=device)
        lib.procrustes_error(p_.to(device).contiguous(), g_.to(device).contiguous(), aligned, err)
        assert float((aligned.cpu() - g_).abs().max()) <= 2e-6 and float(err.max()) <= 50 * 2e-6


# ------------------------------------------------------------------------------------------------
# FreiHAND augmentation warp (csrc/augment.hip) vs the reference's PIL path (tests/golden/data_path.npz)
# ------------------------------------------------------------------------------------------------
def augment_case(lib, device, golden_dir):
    import os
    from hifihr_amd.data import affine_for_rotation, pil_affine_fixed_terms
    g = np.load(os.path.join(golden_dir, "data_path.npz"))
    for i in range(int(g["n"])):
        img, mask, rot = g[f"img{i}"], g[f"mask{i}"], float(g[f"rot{i}"])
        res = img.shape[0]
        total, post = affine_for_rotation(np.asarray([res // 2, res // 2]), res, [res, res], rot)
        assert np.array_equal(total, g[f"aff{i}"]) and np.array_equal(post, g[f"post{i}"]), "get_affine_transform restatement"
        # a cache of three images with the wanted one in the middle: the gather index is exercised too
        rgbx = np.zeros((3, res, res, 4), np.uint8); rgbx[1, :, :, :3] = img; rgbx[0] = 9; rgbx[2] = 17
        mk = np.zeros((3, res, res), np.uint8); mk[1] = mask; mk[0] = 255
        cache = torch.from_numpy(rgbx).to(device).view(torch.int32).reshape(3, res, res)
        out_i = torch.full((2, 3, res, res), 7.0, device=device); out_m = torch.full((2, 3, res, res), 7.0, device=device)
        idx = torch.tensor([1, 1], dtype=torch.int32, device=device)
        ident = pil_affine_fixed_terms(np.eye(3, dtype=np.float32))
        coef = torch.tensor([pil_affine_fixed_terms(total), ident], dtype=torch.int32, device=device)
        lib.freihand_augment(cache, torch.from_numpy(mk).to(device), idx, coef, out_i, out_m)
        want = torch.from_numpy(g[f"timg{i}"]).permute(2, 0, 1).float().div(255)
        assert torch.equal(out_i[0].cpu(), want), f"image warp case {i} (rot {rot})"
        wm = torch.round(torch.from_numpy(g[f"tmask{i}"]).float().div(255))
        assert torch.equal(out_m[0].cpu(), wm.unsqueeze(0).repeat(3, 1, 1)), f"mask warp case {i}"
        assert torch.equal(out_i[1].cpu(), torch.from_numpy(img).permute(2, 0, 1).float().div(255)), "identity warp"
        # K and joints (data/dataset.py:258-260, 271-275)
        np.testing.assert_array_equal(post.dot(g[f"K{i}"]).astype(np.float32), g[f"tK{i}"])


def freihand_batch_case(lib, device, seed=0, B=5, n=7, res=32, J=21, V=50):
    """hifihr_freihand_batch == hifihr_freihand_augment + the torch broadcast expressions of hifihr_amd/data.py:batch and
    traineval.data_dic (Ks, Ps, joints, verts, j2d_gt, scales, idxs, segms_gt)."""
    from hifihr_amd.data import batch_affine_terms
    from hifihr_amd.traineval import proj_func
    rng = np.random.default_rng(seed)
    rgbx = rng.integers(0, 256, (n, res, res, 4), dtype=np.uint8)
    mk = (rng.random((n, res, res)) > 0.5).astype(np.uint8) * 255
    Ks = np.tile(np.array([[400.0, 0, 112], [0, 410.0, 108], [0, 0, 1]], np.float32), (n, 1, 1)) + rng.normal(0, 1, (n, 3, 3)).astype(np.float32)
    joints = (rng.normal(0, 0.05, (n, J, 3)) + np.array([0, 0, 0.6])).astype(np.float32)
    verts = (rng.normal(0, 0.05, (n, V, 3)) + np.array([0, 0, 0.6])).astype(np.float32)
    scales = rng.random(n).astype(np.float32)
    idx = rng.integers(0, n, B)
    rots = rng.uniform(-np.pi, np.pi, B)
    fixed, post, rmat = batch_affine_terms(np.asarray([res // 2, res // 2]), res, [res, res], rots)
    packed = np.concatenate([idx.astype(np.int32), fixed.reshape(-1), post.reshape(-1).view(np.int32), rmat.reshape(-1).view(np.int32)])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    cache = d(rgbx).view(torch.int32).reshape(n, res, res)
    f = lambda *shape: torch.full(shape, 7.0, device=device)
    out = {"imgs": f(B, 3, res, res), "masks": f(B, 3, res, res), "segms_gt": torch.full((B, res, res), 7, dtype=torch.int64, device=device),
           "Ks": f(B, 3, 3), "Ps": f(B, 3, 4), "joints": f(B, J, 3), "verts": f(B, V, 3), "j2d_gt": f(B, J, 2), "scales": f(B),
           "idxs": torch.full((B,), 7, dtype=torch.int64, device=device)}
    lib.freihand_batch(cache, d(mk), d(Ks), d(joints), d(verts), d(scales), d(packed), B, out)
    wi, wm = f(B, 3, res, res), f(B, 3, res, res)
    lib.freihand_augment(cache, d(mk), d(idx.astype(np.int32)), d(fixed), wi, wm)
    assert torch.equal(out["imgs"], wi) and torch.equal(out["masks"], wm) and torch.equal(out["segms_gt"], wm[:, 0].long())
    il = torch.from_numpy(idx).long()
    post_t, rmat_t = torch.from_numpy(post), torch.from_numpy(rmat)
    wK = (post_t.unsqueeze(3) * torch.from_numpy(Ks)[il].unsqueeze(1)).sum(2)
    rot = lambda pts: (pts.unsqueeze(2) * rmat_t.unsqueeze(1)).sum(3)
    wj, wv = rot(torch.from_numpy(joints)[il]), rot(torch.from_numpy(verts)[il])
    close = lambda a, b, tol=2e-6: float((a.cpu() - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))
    assert close(out["Ks"], wK) and close(out["joints"], wj) and close(out["verts"], wv)
    assert torch.equal(out["Ps"][:, :, :3], out["Ks"]) and float(out["Ps"][:, :, 3].abs().max()) == 0.0
    assert close(out["j2d_gt"], proj_func(wj, wK), 1e-5)
    assert torch.equal(out["scales"].cpu(), torch.from_numpy(scales)[il]) and torch.equal(out["idxs"].cpu(), il)
    # hifihr_freihand_batch_step: the same outputs bit for bit + what a training iteration derives from them (train_hrnet.py:62-68,
    # models_res_nimble.py:228-235), for a root inside the skeleton and for "no root"
    for root_id in (min(9, J - 1), 0, -1):
        out2 = {k: torch.full_like(v, 7) for k, v in out.items()}
        out2.update({"root_xyz": f(B, 1, 3), "joints_rel": f(B, J, 3), "verts_rel": f(B, V, 3), "cam_ndc": f(B, 4)})
        lib.freihand_batch(cache, d(mk), d(Ks), d(joints), d(verts), d(scales), d(packed), B, out2, root_id=root_id, image_size=res)
        for k in out:
            assert torch.equal(out[k], out2[k]), k
        root = out["joints"][:, root_id:root_id + 1] if root_id >= 0 else torch.zeros(B, 1, 3, device=device)
        assert torch.equal(out2["root_xyz"], root)
        assert torch.equal(out2["joints_rel"], out["joints"] - root) and torch.equal(out2["verts_rel"], out["verts"] - root)
        K = out["Ks"].cpu()
        cam = torch.stack([-2 * K[:, 0, 0] / res, -2 * K[:, 1, 1] / res, 1 - 2 * K[:, 0, 2] / res, 1 - 2 * K[:, 1, 2] / res], 1)
        assert close(out2["cam_ndc"], cam, 1e-6)


def ho3d_batch_case(lib, device, golden_dir):
    """hifihr_ho3d_batch vs tests/golden/ho3d_path.npz: Pillow's own crop + resize outputs (bit for bit) and the reference's uv21_crop /
    K_crop lines; windows from hifihr_amd.data.ho3d_crop_windows, itself checked against the reference's window lines here."""
    import os
    from hifihr_amd.data import ho3d_crop_windows
    g = np.load(os.path.join(golden_dir, "ho3d_path.npz"))
    ids = [i for i in range(int(g["n"])) if f"img_crop{i}" in g.files]
    allids = list(range(int(g["n"])))
    center, scale, size, box = ho3d_crop_windows(np.stack([g[f"uv21_{i}"] for i in allids]), np.stack([g[f"noise{i}"] for i in allids]),
                                                 np.concatenate([g[f"scale_noise{i}"] for i in allids]))
    for k, i in enumerate(allids):
        assert np.array_equal(center[k], g[f"crop_center{i}"]) and scale[k] == g[f"scale{i}"][0] and size[k] == g[f"size{i}"][0], i
        x1, y1, sz = float(g[f"x1_{i}"].reshape(-1)[0]), float(g[f"y1_{i}"].reshape(-1)[0]), float(g[f"size{i}"].reshape(-1)[0])
        assert tuple(box[k]) == tuple(int(round(v)) for v in (x1, y1, x1 + sz, y1 + sz)), i
    FH, FW = g[f"img{ids[0]}"].shape[:2]
    frames = np.zeros((len(ids) + 1, FH, FW, 4), np.uint8); masks = np.zeros((len(ids) + 1, FH, FW), np.uint8)
    for k, i in enumerate(ids):
        frames[k + 1, :, :, :3] = g[f"img{i}"]; masks[k + 1] = g[f"mask{i}"]
    frames[0] = 200; masks[0] = 255
    order = [2, 0, 3, 1]                                      # batch order != cache order: the gather index is exercised
    sel = [ids[k] for k in order]
    B, S = len(order), 224
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    packed = np.concatenate([np.asarray([k + 1 for k in order], np.int32), np.stack([box[i] for i in sel]).reshape(-1),
                             np.concatenate([np.stack([center[i] for i in sel]), np.asarray([scale[i] for i in sel])[:, None]], 1)
                             .astype(np.float32).reshape(-1).view(np.int32)])
    Ks = np.stack([np.eye(3, dtype=np.float32)] + [g[f"K{i}"] for i in ids]); uv = np.stack([np.zeros((21, 2), np.float32)] + [g[f"uv21_{i}"] for i in ids])
    xyz = np.random.default_rng(0).normal(size=(len(ids) + 1, 21, 3)).astype(np.float32)
    ws = torch.empty(lib.ho3d_workspace_bytes(B, S) // 4 + 1, dtype=torch.int32, device=device)
    f = lambda *shape: torch.full(shape, 7.0, device=device)
    out = {"img_crop": f(B, 3, S, S), "hand_mask_crop": f(B, 1, S, S), "K_crop": f(B, 3, 3), "uv21_crop": f(B, 21, 2), "xyz21": f(B, 21, 3)}
    lib.ho3d_batch(d(frames).view(torch.int32).reshape(len(ids) + 1, FH, FW), d(masks), d(Ks), d(uv), d(xyz), d(packed), B, S, ws, out)
    for b, i in enumerate(sel):
        want = torch.from_numpy(g[f"img_crop{i}"]).permute(2, 0, 1).float().div(255)
        assert torch.equal(out["img_crop"][b].cpu(), want), f"frame crop {i}"
        wm = torch.round(torch.from_numpy(g[f"mask_crop{i}"]).float().div(255))
        assert torch.equal(out["hand_mask_crop"][b, 0].cpu(), wm), f"mask crop {i}"
        assert torch.equal(out["uv21_crop"][b].cpu(), torch.from_numpy(g[f"uv21_crop{i}"])), f"uv21_crop {i}"
        np.testing.assert_allclose(out["K_crop"][b].cpu().numpy(), g[f"K_crop{i}"], rtol=1e-6, atol=1e-4)
        assert torch.equal(out["xyz21"][b].cpu(), torch.from_numpy(xyz[order[b] + 1]))


# ------------------------------------------------------------------------------------------------
# one-launch weight re-layout (hifihr_weight_prep) == the separate transpose / Winograd weight transforms, bit for bit
# ------------------------------------------------------------------------------------------------
def weight_prep_case(lib, device, seed=0):
    gen = torch.Generator().manual_seed(seed)
    shapes = [(32, 64, 3), (64, 32, 3), (48, 16, 1), (16, 4, 7), (128, 128, 3)]
    jobs, want = [], []
    for K, C, R in shapes:
        w = torch.randn(K, R, R, C, generator=gen).to(device)
        wt = torch.empty(C, R, R, K, device=device)
        lib.weight_transpose(w, wt, K, R * R, C)
        jobs.append((w, torch.full((K * R * R * C,), 7.0, device=device), K, C, R * R, 0)); want.append(wt.reshape(-1))
        if R == 3:
            U = torch.empty(16 * K * C, device=device); U2 = torch.empty(16 * K * C, device=device)
            lib.wino_weight_transform(w, U, K, C, 0)
            lib.wino_weight_transform(wt, U2, C, K, 1)
            jobs.append((w, torch.full((16 * K * C,), 7.0, device=device), K, C, 9, 1)); want.append(U)
            jobs.append((w, torch.full((16 * K * C,), 7.0, device=device), K, C, 9, 2)); want.append(U2)
            U4 = torch.empty(36 * K * C, device=device); U42 = torch.empty(36 * K * C, device=device)      # F(4x4, 3x3): kinds 3 / 4
            lib.wino_weight_transform(w, U4, K, C, 0, 4)
            lib.wino_weight_transform(wt, U42, C, K, 1, 4)
            jobs.append((w, torch.full((36 * K * C,), 7.0, device=device), K, C, 9, 3)); want.append(U4)
            jobs.append((w, torch.full((36 * K * C,), 7.0, device=device), K, C, 9, 4)); want.append(U42)
    for K, C, R in ((64, 3, 7), (8, 5, 3), (4, 1, 1)):          # kind 5: channels zero-padded to a multiple of 4
        w = torch.randn(K, R, R, C, generator=gen)
        C4 = (C + 3) // 4 * 4
        ref = torch.zeros(K, R, R, C4); ref[..., :C] = w
        jobs.append((w.to(device), torch.full((K * R * R * C4,), 7.0, device=device), K, C, R * R, 5)); want.append(ref.reshape(-1))
    table = lib.prep_jobs(jobs, device)
    lib.weight_prep(table, len(jobs), 3)
    for (_, dst, K, C, RS, kind), ref in zip(jobs, want):
        assert torch.equal(dst.cpu(), ref.cpu()), (K, C, RS, kind)


def stem_c3_wgrad_case(lib, device, N=2, H=56, seed=0):
    """hifihr_conv2d_bwd_weight_c3 (gradient in the 3-channel parameter's layout) == hifihr_conv2d_bwd_weight on the padded
    problem, first three channels; accumulate semantics; bit-reproducible."""
    gen = torch.Generator().manual_seed(seed)
    K, R, stride, pad = 64, 7, 2, 3
    assert lib.conv2d_bwd_weight_c3_supported(N, H, H, K, R, R, stride, pad)
    assert not lib.conv2d_bwd_weight_c3_supported(N, H, H, K, 3, 3, 1, 1)
    OH = (H + 2 * pad - R) // stride + 1
    x = torch.randn(N, H, H, 4, generator=gen); x[..., 3] = 0
    dy = torch.randn(N, OH, OH, K, generator=gen)
    xd, dyd = x.to(device), dy.to(device)
    nws = lib.conv2d_wgrad_workspace_bytes(N, H, H, 4, K, R, R, stride, pad)
    assert nws > 0
    ws = torch.empty(nws // 4, device=device)
    dw4 = torch.zeros(K, R, R, 4, device=device)
    lib.conv2d_bwd_weight(xd, dyd, dw4, N, H, H, 4, K, R, R, stride, pad, ws=ws)
    dw3 = torch.full((K, R, R, 3), 0.25, device=device)
    lib.conv2d_bwd_weight_c3(xd, dyd, dw3, N, H, H, K, R, R, stride, pad, ws)
    assert torch.equal(dw3 - 0.25, (dw4[..., :3] + 0.25) - 0.25), "3-channel stem gradient == padded problem (same slabs, same order)"
    again = torch.full((K, R, R, 3), 0.25, device=device)
    lib.conv2d_bwd_weight_c3(xd, dyd, again, N, H, H, K, R, R, stride, pad, ws)
    assert torch.equal(again, dw3)
    ref = torch.nn.functional.conv2d(x[..., :3].permute(3, 0, 1, 2).contiguous(), dy.permute(3, 0, 1, 2).contiguous(), None, 1, pad, stride)
    ref = ref[:, :, :R, :R].permute(1, 2, 3, 0)                   # [K][R][S][3]
    assert float((dw3.cpu() - 0.25 - ref).abs().max()) <= 2e-4 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------
# grouped linear layers (csrc/mlp.hip *_group_kernel) == the single-layer launches
# ------------------------------------------------------------------------------------------------
def linear_group_case(lib, device, B=32, seed=0):
    gen = torch.Generator().manual_seed(seed)
    shapes = [(512, 128, 1), (512, 128, 1), (128, 48, 0), (128, 10, 0), (32, 3, 0), (32, 1, 0)]
    d = lambda t: t.to(device).contiguous()
    mem, ref = [], []
    for I, O, act in shapes:
        x = torch.randn(B, I, generator=gen); w = torch.randn(O, I, generator=gen) / I ** 0.5; b = torch.randn(O, generator=gen) * 0.1
        dy = torch.randn(B, O, generator=gen)
        m = dict(x=d(x), w=d(w), b=d(b), y=torch.full((B, O), 7.0, device=device), act=act)
        y1 = torch.empty(B, O, device=device)
        lib.linear_fwd(m["x"], m["w"], m["b"], act, y1)
        dz = torch.empty(B, O, device=device); dW = torch.full((O, I), 0.5, device=device); db = torch.full((O,), -0.5, device=device)
        dx = torch.full((B, I), 7.0, device=device)
        lib.linear_bwd(d(dy), y1, m["x"], m["w"], act, dz, dW, db, dx)
        m.update(dy=d(dy), dz=torch.empty(B, O, device=device), dW=torch.full((O, I), 0.5, device=device), db=torch.full((O,), -0.5, device=device),
                 dx=torch.full((B, I), 7.0, device=device))
        mem.append(m); ref.append((y1, dW, db, dx))
    mem[3]["dx"] = None                                   # a member without an input gradient
    lib.linear_fwd_group(mem)
    for m, r in zip(mem, ref):
        assert torch.equal(m["y"], r[0]), "grouped forward"
    lib.linear_bwd_group(mem)
    for i, (m, r) in enumerate(zip(mem, ref)):
        assert float((m["dW"] - r[1]).abs().max()) <= 1e-5 * float(r[1].abs().max()) and float((m["db"] - r[2]).abs().max()) <= 1e-4, i
        if m["dx"] is not None:
            assert float((m["dx"] - r[3]).abs().max()) <= 1e-5 * float(r[3].abs().max()) + 1e-6, i
    # members that read the SAME input may share ONE dx (ops._LinearGroup.backward does for the heads' first layers): it then holds the sum
    shared = torch.full((B, 512), 7.0, device=device)
    mem[1]["x"] = mem[0]["x"]
    lib.linear_bwd_group([dict(mem[0], dx=shared, dW=torch.zeros_like(mem[0]["dW"]), db=torch.zeros_like(mem[0]["db"])),
                          dict(mem[1], dx=shared, dW=torch.zeros_like(mem[1]["dW"]), db=torch.zeros_like(mem[1]["db"]))])
    dx0, dx1 = torch.empty(B, 512, device=device), torch.empty(B, 512, device=device)
    lib.linear_bwd_group([dict(mem[0], dx=dx0, dW=torch.zeros_like(mem[0]["dW"]), db=torch.zeros_like(mem[0]["db"])),
                          dict(mem[1], dx=dx1, dW=torch.zeros_like(mem[1]["dW"]), db=torch.zeros_like(mem[1]["db"]))])
    want = dx0 + dx1
    assert float((shared - want).abs().max()) <= 1e-5 * float(want.abs().max()) + 1e-6, "shared dx"


MANO_PARENTS16 = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]     # ManoLayer's tree in its re-ordered joint index space (my_mano.py:395-434)


def random_lbs_tables(V, J, S, seed, K=4):
    """Small random skinned mesh: a random tree, <= K weights per vertex, a sparse convex joint regressor."""
    rng = np.random.RandomState(seed)
    vt = rng.randn(V, 3) * 0.05
    sd = rng.randn(V, 3, S) * 0.004
    parents = np.array([-1] + [rng.randint(0, j) for j in range(1, J)], dtype=np.int32)
    w = np.zeros((V, J))
    for v in range(V):
        idx = rng.choice(J, size=min(J, rng.randint(1, K + 1)), replace=False)
        w[v, idx] = rng.rand(idx.size) + 0.05
    w /= w.sum(1, keepdims=True)
    jr = np.zeros((J, V))
    for j in range(J):
        idx = rng.choice(V, size=min(V, 24), replace=False)
        jr[j, idx] = rng.rand(idx.size)
    jr /= jr.sum(1, keepdims=True)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (vt, sd, jr, w)) + (parents,)


def lbs_case(lib, device, tabs, B, seed, pose_scale=0.6, vtol=2e-6, gtol=2e-4):
    """csrc/lbs.hip through the C-ABI vs oracle/lbs_oracle.py: verts, posed joints, d/dtheta, d/dbeta of a random scalar of both
    outputs.  (The backward's vertex sums are float atomics: gtol is relative to the largest gradient entry.)"""
    from oracle import lbs_oracle as lo
    vt, sd, jr, w, parents = tabs
    V, J, S = vt.shape[0], w.shape[1], sd.shape[2]
    gen = torch.Generator().manual_seed(seed)
    theta = torch.randn(B, J, 3, generator=gen) * pose_scale
    theta[0, min(1, J - 1)] = 0.0                           # the zero-angle branch of Rodrigues
    beta = torch.randn(B, S, generator=gen)
    wv, wj = torch.randn(B, V, 3, generator=gen), torch.randn(B, J, 3, generator=gen)
    th, be = theta.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rv, rj = lo.lbs_forward(vt, sd, jr, w, parents, th, be)
    ((rv * wv).sum() + (rj * wj).sum()).backward()
    h = lib.lbs_create(vt, sd, jr, w, parents)
    try:
        d = lambda t: t.to(device).contiguous()
        verts, joints = torch.empty(B, V, 3, device=device), torch.empty(B, J, 3, device=device)
        lib.lbs_fwd(h, d(theta), d(beta), verts, joints)
        scale = float(rv.detach().abs().max())
        assert float((verts.cpu() - rv.detach()).abs().max()) <= vtol * max(1.0, scale / 0.1), float((verts.cpu() - rv.detach()).abs().max())
        assert float((joints.cpu() - rj.detach()).abs().max()) <= vtol * max(1.0, scale / 0.1)
        scratch = torch.zeros(B, J, 12, device=device)
        gtheta, gbeta = torch.full((B, J, 3), 9.0, device=device), torch.zeros(B, S, device=device)
        lib.lbs_bwd(h, d(theta), d(beta), d(wv), d(wj), scratch, gtheta, gbeta)
        for got, ref, name in ((gtheta, th.grad, "gtheta"), (gbeta, be.grad, "gbeta")):
            if ref is None or ref.numel() == 0:
                continue
            err, mag = float((got.cpu() - ref).abs().max()), float(ref.abs().max())
            assert err <= gtol * mag, (name, err, mag)
        gtheta2, gbeta2 = torch.empty(B, J, 3, device=device), torch.zeros(B, S, device=device)      # gjoints = NULL
        scratch.zero_()
        lib.lbs_bwd(h, d(theta), d(beta), d(wv), None, scratch, gtheta2, gbeta2)
        th.grad = None; be.grad = None
        rv2, _ = lo.lbs_forward(vt, sd, jr, w, parents, th, be)
        (rv2 * wv).sum().backward()
        assert float((gtheta2.cpu() - th.grad).abs().max()) <= gtol * float(th.grad.abs().max())
        if S:
            assert float((gbeta2.cpu() - be.grad).abs().max()) <= gtol * float(be.grad.abs().max())
    finally:
        lib.lbs_destroy(h)


# ------------------------------------------------------------------------------------------------
# the reference trunk's batch-of-8 fixture (tests/golden/resnet18_b8.npz, tools/make_golden.py:gen_resnet18_b8)
# ------------------------------------------------------------------------------------------------
def resnet18_b8_inputs(g):
    """x, wl, wf regenerated from the generator seed the fixture was made with, verified against its float64 checksums."""
    gen = torch.Generator().manual_seed(1234)
    x = torch.rand(8, 3, 64, 64, generator=gen)
    wl = torch.randn(tuple(g["low"].shape), generator=gen); wf = torch.randn(tuple(g["feat"].shape), generator=gen)
    got = np.array([x.double().sum().item(), wl.double().sum().item(), wf.double().sum().item()])
    assert np.allclose(got, g["checksums"], rtol=0, atol=1e-9), "the CPU generator no longer reproduces the fixture's inputs"
    return x, wl, wf


def resnet18_b8_check(g, net, low, feat, out_atol, grad_rtol, grad_l2=None):
    """net = a module with torchvision's ResNet attribute names whose .grad fields are filled; every gradient the fixture holds:
    max error / max |reference| < grad_rtol and, if given, relative L2 error < grad_l2."""
    np.testing.assert_allclose(low.detach().cpu().numpy(), g["low"], atol=out_atol, rtol=1e-4)
    np.testing.assert_allclose(feat.detach().cpu().numpy(), g["feat"], atol=out_atol, rtol=1e-4)
    params = dict(net.named_parameters())
    worst, l2 = {}, {}
    for key in g.files:
        if not key.startswith("g_"):
            continue
        toks = key[2:].split("_")               # g_layer2_0_downsample_0_weight -> layer2.0.downsample.0.weight
        name = ".".join(toks)
        grad = params[name].grad.detach().cpu().numpy()
        ref = g[key]
        if grad.ndim == 4:
            grad = grad[:8]
        worst[name] = float(np.abs(grad - ref).max() / (np.abs(ref).max() + 1e-12))
        l2[name] = float(np.linalg.norm((grad - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30))
    bad = {k: v for k, v in worst.items() if v >= grad_rtol}
    assert not bad, bad
    if grad_l2 is not None:
        bad = {k: v for k, v in l2.items() if v >= grad_l2}
        assert not bad, ("relative L2", bad)
    return worst, l2


# ------------------------------------------------------------------------------------------------
# batch statistics of activations with |mean| >> std (round-2 review: E[x^2] - mean^2 in fp32 loses the variance there)
# ------------------------------------------------------------------------------------------------
def bn_large_mean_case(lib, device, producer, seed=0, mean=50.0, std=0.1):
    """A batch-norm whose input has mean 50 / std 0.1 per channel (mean^2 / var = 2.5e5: in fp32 `E[x^2] - mean^2` has no correct digit
    left), statistics from every kind of producer, against F.batch_norm computed in float64 on the same values.
    producer: "stats" (hifihr_bn_stats on the tensor), "conv3x3" (implicit-GEMM epilogue), "conv1x1" (GEMM row-share epilogue),
    "halo" (layer-1 kernel), "wino4" / "wino2" (Winograd output transforms), "dw" (depthwise epilogue)."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    d = lambda t: t.to(device).contiguous()
    if producer == "stats":
        N, H, W, K = 4, 9, 7, 64
        y = mean + std * torch.randn(N, K, H, W, generator=gen)
        yd = d(y.permute(0, 2, 3, 1))
        stats = torch.zeros(lib.bn_stats_floats(K), device=device)
        lib.bn_stats(yd, N * H * W, K, stats)
    elif producer == "dw":
        N, H, W, K = 2, 9, 8, 64
        x = mean + std * torch.randn(N, K, H, W, generator=gen)
        w = torch.full((K, 1, 3, 3), 1.0 / 9) + 0.01 * torch.randn(K, 1, 3, 3, generator=gen)
        y = F.conv2d(x.double(), w.double(), None, 1, 0, groups=K).float()
        OH, OW = y.shape[2], y.shape[3]
        yd = torch.empty(N, OH, OW, K, device=device); stats = torch.zeros(lib.bn_stats_floats(K), device=device)
        lib.dwconv2d_fwd(d(x.permute(0, 2, 3, 1)), d(w.reshape(K, 3, 3)), yd, N, H, W, K, OH, OW, 3, 1, 0, 0, stats=stats)
        H, W = OH, OW
    else:
        N, H, W, C, K, R = {"conv3x3": (2, 9, 7, 16, 64, 3), "conv1x1": (2, 8, 8, 32, 128, 1), "halo": (2, 10, 14, 64, 64, 3),
                            "wino4": (2, 8, 8, 64, 64, 3), "wino2": (2, 8, 8, 64, 64, 3)}[producer]
        # a strongly positive input and filters that are (almost) a positive centre tap: every output channel sits at a large mean with a
        # small spread, at the zero-padded border too
        x = mean + std * torch.randn(N, C, H, W, generator=gen)
        w = 1e-4 * torch.randn(K, C, R, R, generator=gen) / C
        w[:, :, R // 2, R // 2] = (1.0 + 0.05 * torch.randn(K, C, generator=gen)) / C
        pad = R // 2
        y = F.conv2d(x.double(), w.double(), None, 1, pad).float()
        xd, wd = d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1))
        yd = torch.empty(N, H, W, K, device=device); stats = torch.zeros(lib.bn_stats_floats(K), device=device)
        if producer in ("wino4", "wino2"):
            m = 4 if producer == "wino4" else 2
            P, T = (m + 2) ** 2, lib.wino_tiles(N, H, W, m)
            U = torch.empty(P, K, C, device=device); V = torch.empty(P, T, C, device=device); Mm = torch.empty(P, T, K, device=device)
            lib.wino_weight_transform(wd, U, K, C, 0, m); lib.wino_input_transform(xd, V, N, H, W, C, m)
            lib.wino_gemm(V, U, Mm, N, H, W, C, K, ws=None, m=m); lib.wino_output_transform(Mm, yd, stats, N, H, W, K, m=m)
        else:
            lib.conv2d_fwd_bnstats(xd, wd, yd, stats, N, H, W, C, K, R, R, 1, pad)
    # interior channel statistics as they are (what the kernel saw is its OWN y: compare against statistics of that tensor in float64)
    yk = yd.cpu().double().reshape(-1, K)
    mu64, var64 = yk.mean(0), yk.var(0, unbiased=False)
    assert float((mu64.abs() / var64.sqrt()).min()) > 30.0, "the case is meant to have |mean| >> std"
    gamma = 1 + 0.1 * torch.randn(K, generator=gen); beta = 0.1 * torch.randn(K, generator=gen)
    out = torch.empty_like(yd); sm = torch.empty(K, device=device); si = torch.empty(K, device=device)
    rm, rv = torch.zeros(K, device=device), torch.ones(K, device=device)
    lib.bn_act_fwd(yd, stats, d(gamma), d(beta), None, 0, N * H * W, K, 1e-5, 0.1, out, sm, si, rm, rv)
    assert float(stats.abs().max()) == 0.0
    np.testing.assert_allclose(sm.cpu().double().numpy(), mu64.numpy(), rtol=2e-7, atol=0)
    inv64 = 1.0 / torch.sqrt(var64 + 1e-5)
    np.testing.assert_allclose(si.cpu().double().numpy(), inv64.numpy(), rtol=2e-4, atol=0, err_msg=f"{producer}: 1/sqrt(var + eps)")
    ref = ((yk - mu64) * inv64 * gamma.double() + beta.double()).float().reshape(out.shape)
    # the normalised output amplifies the rounding of y and of the saved fp32 mean (ulp(50) / std = 4e-5 of a standard deviation each)
    assert float((out.cpu() - ref).abs().max()) <= 2e-3, (producer, float((out.cpu() - ref).abs().max()))
    np.testing.assert_allclose(rv.cpu().double().numpy(), (0.9 + 0.1 * var64 * (N * H * W) / (N * H * W - 1)).numpy(), rtol=2e-4)


# ------------------------------------------------------------------------------------------------
# batch-norm fused into the Winograd F(4x4, 3x3) input transform (csrc/wino4_bn.hip) vs the two separate launches
# ------------------------------------------------------------------------------------------------
def wino_bn_input_case(lib, device, N, H, W, C, residual, seed=0):
    """hifihr_wino_bn_input_transform == hifihr_bn_act_fwd (ReLU, optional residual) followed by hifihr_wino_input_transform, bit for bit
    (same scale / shift / residual / ReLU expression, same transform), and both against torch: V through the known input transform of a
    torch-computed activation."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(seed)
    d = lambda t: t.to(device).contiguous()
    x = torch.randn(N, H, W, C, generator=gen) * 1.3 + 0.2
    res = torch.randn(N, H, W, C, generator=gen) if residual else None
    gamma = 1 + 0.1 * torch.randn(C, generator=gen); beta = 0.1 * torch.randn(C, generator=gen)
    M = N * H * W
    T = lib.wino_tiles(N, H, W, 4)

    def fresh():
        st = torch.zeros(lib.bn_stats_floats(C), device=device)
        lib.bn_stats(d(x), M, C, st)
        return st, torch.zeros(C, device=device), torch.ones(C, device=device), torch.empty(C, device=device), torch.empty(C, device=device)
    # the two separate launches
    st, rm0, rv0, sm0, si0 = fresh()
    a0 = torch.empty(N, H, W, C, device=device)
    lib.bn_act_fwd(d(x), st, d(gamma), d(beta), d(res) if residual else None, 1, M, C, 1e-5, 0.1, a0, sm0, si0, rm0, rv0)
    V0 = torch.empty(36, T, C, device=device)
    lib.wino_input_transform(a0, V0, N, H, W, C, 4)
    # the fused launch
    st, rm1, rv1, sm1, si1 = fresh()
    V1 = torch.full((36, T, C), 7.0, device=device)
    out = torch.full((N, H, W, C), 7.0, device=device) if residual else None
    lib.wino_bn_input_transform(d(x), st, d(gamma), d(beta), d(res) if residual else None, out, V1, N, H, W, C, 4, 1e-5, 0.1, sm1, si1, rm1, rv1)
    assert float(st.abs().max()) == 0.0, "statistics slots and counters must come back zeroed"
    assert torch.equal(V1, V0), float((V1 - V0).abs().max())
    assert torch.equal(sm1, sm0) and torch.equal(si1, si0) and torch.equal(rm1, rm0) and torch.equal(rv1, rv0)
    if residual:
        assert torch.equal(out, a0)
    # and against torch
    ref = F.batch_norm(x.permute(0, 3, 1, 2), None, None, gamma, beta, True, 0.0, 1e-5)
    if residual:
        ref = ref + res.permute(0, 3, 1, 2)
    ref = F.relu(ref).permute(0, 2, 3, 1)
    assert float((a0.cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))


def wino_bn_bwd_case(lib, device, N, H, W, C, residual, addend, seed=0):
    """The backward of the batch-norm / Winograd fusion (csrc/wino4_bn.hip) against the launches it replaces:
      hifihr_wino_output_transform_bnred + hifihr_bn_bwd_apply  ==  hifihr_wino_output_transform (+ add) + hifihr_bn_act_bwd
      hifihr_wino_bn_bwd_dual_transform                         ==  hifihr_bn_bwd_apply + hifihr_wino_input_dy_transform   (bit for bit)"""
    gen = torch.Generator().manual_seed(seed)
    d = lambda t: t.to(device).contiguous()
    M = N * H * W
    T = lib.wino_tiles(N, H, W, 4)
    x = d(torch.randn(N, H, W, C, generator=gen) * 1.3 + 0.2)
    res = d(torch.randn(N, H, W, C, generator=gen)) if residual else None
    gadd = d(torch.randn(N, H, W, C, generator=gen)) if addend else None
    gamma = d(1 + 0.1 * torch.randn(C, generator=gen)); beta = d(0.1 * torch.randn(C, generator=gen))
    Mm = d(torch.randn(36, T, C, generator=gen))
    # forward statistics and block output (for the mask)
    st = torch.zeros(lib.bn_stats_floats(C), device=device)
    lib.bn_stats(x, M, C, st)
    out = torch.empty(N, H, W, C, device=device); sm = torch.empty(C, device=device); si = torch.empty(C, device=device)
    lib.bn_act_fwd(x, st, gamma, beta, res, 1, M, C, 1e-5, 0.1, out, sm, si, None, None)
    # the separate launches
    dA = torch.empty(N, H, W, C, device=device)
    lib.wino_output_transform(Mm, dA, None, N, H, W, C, m=4)
    if addend:
        dA = dA + gadd
    red = torch.zeros(lib.bn_stats_floats(C), device=device)
    dx0 = torch.empty_like(x); dres0 = torch.empty_like(x); dg0 = torch.zeros(C, device=device); db0 = torch.zeros(C, device=device)
    lib.bn_act_bwd(dA, out if residual else None, x, sm, si, gamma, beta, 1, M, C, red, dx0, dres0, dg0, db0)
    # fused part 1 + apply
    g = torch.full((N, H, W, C), 7.0, device=device)
    red1 = torch.zeros(lib.bn_stats_floats(C), device=device)
    lib.wino_output_transform_bnred(Mm, x, out if residual else None, gadd, sm, si, gamma, beta, red1, g, N, H, W, C, 4)
    assert torch.equal(g, dres0), float((g - dres0).abs().max())            # the masked gradient, bit for bit
    red_keep = red1.clone()
    dx1 = torch.empty_like(x); dg1 = torch.zeros(C, device=device); db1 = torch.zeros(C, device=device)
    lib.bn_bwd_apply(g, x, sm, si, gamma, M, C, red1, dx1, dg1, db1)
    assert float(red1[:32 * 4 * C + 64].abs().max()) == 0.0
    tol = lambda ref: 2e-5 * float(ref.abs().max()) + 1e-7      # the reductions add in a different order
    assert float((dx1 - dx0).abs().max()) <= tol(dx0), float((dx1 - dx0).abs().max())
    assert float((dg1 - dg0).abs().max()) <= tol(dg0) and float((db1 - db0).abs().max()) <= tol(db0)
    # fused part 2 == apply + dual transform on the SAME sums, bit for bit
    V0 = torch.empty(36, T, C, device=device); Y0 = torch.empty(36, T, C, device=device)
    lib.wino_input_dy_transform(dx1, V0, Y0, N, H, W, C, 4)
    V1 = torch.full((36, T, C), 7.0, device=device); Y1 = torch.full((36, T, C), 7.0, device=device)
    dg2 = torch.zeros(C, device=device); db2 = torch.zeros(C, device=device)
    lib.wino_bn_bwd_dual_transform(g, x, sm, si, gamma, red_keep, V1, Y1, N, H, W, C, 4, dg2, db2)
    assert float(red_keep[:32 * 4 * C + 64].abs().max()) == 0.0
    assert torch.equal(V1, V0) and torch.equal(Y1, Y0), (float((V1 - V0).abs().max()), float((Y1 - Y0).abs().max()))
    assert torch.equal(dg2, dg1) and torch.equal(db2, db1)


# ------------------------------------------------------------------------------------------------
# joint_2d / bone_direc / bone_direc_3d (csrc/losses.hip joint_terms_*) vs the torch restatement pinned by tests/golden/losses.npz
# ------------------------------------------------------------------------------------------------
def joint_terms_case(lib, device, B, mse, seed=0, use2=True, use3=True):
    import torch.nn.functional as F
    from oracle.loss_oracle import bone_direction_loss
    gen = torch.Generator().manual_seed(seed)
    j2d = (torch.rand(B, 21, 2, generator=gen) * 224).requires_grad_(True); j2d_gt = torch.rand(B, 21, 2, generator=gen) * 224
    j3d = (torch.randn(B, 21, 3, generator=gen) * 0.05).requires_grad_(True); j3d_gt = torch.randn(B, 21, 3, generator=gen) * 0.05
    lam = (0.7, 1.3, 2.1)
    base = F.mse_loss if mse else F.l1_loss
    one = torch.ones(B, 21, 1)
    ref = [lam[0] * base(j2d_gt, j2d), lam[1] * bone_direction_loss(j2d, j2d_gt, one), lam[2] * bone_direction_loss(j3d, j3d_gt, one)]
    w = torch.tensor([0.9, -1.1, 0.6])
    tot = sum(wi * r for wi, r, u in zip(w, ref, (use2, use2, use3)) if u)
    tot.backward()
    d = lambda t: t.detach().to(device).contiguous()
    out = torch.empty(3, device=device)
    a2 = (d(j2d), d(j2d_gt)) if use2 else (None, None)
    a3 = (d(j3d), d(j3d_gt)) if use3 else (None, None)
    lib.joint_terms_fwd(a2[0], a2[1], a3[0], a3[1], mse, lam, out)
    for k, u in enumerate((use2, use2, use3)):
        want = float(ref[k]) if u else 0.0
        assert abs(float(out[k]) - want) <= 2e-5 * max(1.0, abs(want)), (k, float(out[k]), want)
    g2 = torch.full((B, 21, 2), 7.0, device=device) if use2 else None
    g3 = torch.full((B, 21, 3), 7.0, device=device) if use3 else None
    lib.joint_terms_bwd(a2[0], a2[1], a3[0], a3[1], mse, lam, d(w), g2, g3)
    if use2:
        assert float((g2.cpu() - j2d.grad).abs().max()) <= 1e-5 * float(j2d.grad.abs().max()) + 1e-9
    if use3:
        assert float((g3.cpu() - j3d.grad).abs().max()) <= 1e-5 * float(j3d.grad.abs().max()) + 1e-9


# ------------------------------------------------------------------------------------------------
# The layer contract: batch-norm (csrc/bn.hip), pooling (csrc/pool.hip), depthwise convolution (csrc/dwconv.hip), squeeze-excite
# (csrc/se.hip) and SSIM (csrc/ssim.hip) on fixed geometry lists (tests/test_hostsim_layer_contract.py; the GPU half in
# tests/test_gpu_conv.py and tests/test_gpu_tail.py), in the conv contract's form:
#   * an entry either refuses a geometry (HIFIHR_EINVAL, every output untouched) or matches a FLOAT64 reference of the same operation
#     within  err <= min(c sqrt(L), cap) max|ref| + floor,  L the reduction length of the quantity;
#   * every tensor sits inside a larger allocation (class Guards): margins of inputs are NaN (an out-of-bounds read poisons the output),
#     margins of outputs a canary that must survive bit for bit;
#   * accepted calls run twice on the same scratch; self-cleaning buffers must be all zero after each call; accumulate / overwrite as
#     include/hifihr.h states them.
# The references take a dtype: run in float32 they are "plain fp32 PyTorch on the CPU", whose worst err / (sqrt(L) max|ref|) over the
# emulator lists (tools/layer_contract_c.py prints them) times 4 is the constant c below.  cap = the relative tolerance the family's
# older case in this file asserts (never looser than that).  floor: fp32 torch's own absolute error where the reference is (near) zero,
# times 4, measured by the same tool.
# ------------------------------------------------------------------------------------------------
GUARD_FLOATS = 256
LAYER_CONTRACT_C = {
    # kind: (c, cap)                  fp32 torch's worst ratio (tools/layer_contract_c.py) x 4; the quantities and L; (where cap comes from)
    "bn_sum": (6.5e-7, 1e-4),         # 1.62e-07 x 4   per-channel sum / sum of squares (bn_stats, the depthwise forward's slots), L = rows   (bn_act_case rtol 1e-4)
    "bn_stat": (6.2e-7, 1e-5),        # 1.53e-07 x 4   save_mean / save_invstd / running statistics, L = 1     (bn_act_case rtol 1e-5)
    "bn_y": (8.2e-7, 2e-5),           # 2.03e-07 x 4   y, L = 1                                                (bn_act_case 2e-5)
    "bn_dx": (2.8e-6, 2e-4),          # 7.00e-07 x 4   dx, L = 1                                               (bn_act_case 2e-4)
    "bn_dparam": (1.9e-7, 2e-4),      # 4.53e-08 x 4   dgamma / dbeta, L = M                                   (bn_act_case 2e-4)
    "pool_dx": (1.3e-7, 2e-6),        # 3.03e-08 x 4   max-pool dx, L = ceil(k / s)^2 gradients per pixel      (maxpool_case 2e-6)
    "mm_y": (3.2e-7, 1e-5),           # 7.88e-08 x 4   mmpool y / xavg, L = HW                                 (mmpool_case 1e-5)
    "mm_dx": (2.9e-7, 1e-5),          # 7.07e-08 x 4   mmpool dx, L = 1                                        (mmpool_case 1e-5)
    "mm_dp": (1.5e-7, 1e-4),          # 3.71e-08 x 4   mmpool dp, L = B C                                      (mmpool_case 1e-4)
    "dw_fwd": (1.9e-7, 2e-5),         # 4.65e-08 x 4   depthwise y, L = K K                                    (dwconv_case 2e-5)
    "dw_pre": (2.1e-7, 3e-5),         # 5.21e-08 x 4   depthwise y with bn + swish on load, L = K K            (dwconv_bnswish_case 3e-5)
    "dw_dgrad": (2.2e-7, 2e-5),       # 5.49e-08 x 4   depthwise dx, L = K K                                   (dwconv_case 2e-5)
    "dw_wgrad": (1.5e-7, 1e-4),       # 3.66e-08 x 4   depthwise dw, L = N OH OW                               (dwconv_case 1e-4)
    "dw_wgrad_pre": (3.7e-7, 2e-4),   # 9.06e-08 x 4   the same with bn + swish on load                        (dwconv_bnswish_case 2e-4)
    "se_pool": (2.0e-7, 1e-5),        # 4.96e-08 x 4   se_pool mean / se_bwd_gate sums, L = HW                 (se_case 1e-5, absolute on |mean| <~ 1)
    "se_y": (2.9e-7, 3e-5),           # 7.03e-08 x 4   se_scale y, drop_connect_add out, L = 1                 (se_case 3e-5)
    "se_mlp": (3.3e-7, 2e-5),         # 8.04e-08 x 4   se_mlp_fwd z1, h1 (L = C), gate (L = SQ), mean (L = 1)  (se_case 2e-5)
    "se_grad": (6.6e-7, 3e-4),        # 1.64e-07 x 4   se_mlp_bwd dw1 / db1 / dw2 / db2 (L = B), dz2 (1), dz1 (C), dmean (SQ)   (se_case 3e-4)
    "ssim_val": (5.0e-7, 2e-6),       # 1.25e-07 x 4   SSIM value, ssim_finish, L = planes H W                 (ssim_case 2e-6)
    "ssim_part": (5.3e-7, 2e-6),      # 1.31e-07 x 4   per-tile partial sums, L = 1024                         (ssim_case 2e-6 on their sum)
    "ssim_map": (1.9e-4, 2.1e-3),     # 4.68e-05 x 4   the three derivative maps, L = 121: two constant images put 1 / (s1 + s2 + C2)^2 = 1.2e6 in
    #                                                  front of the rounding of E[x^2] - mu^2.  No older case looks at the maps themselves (cap =
    #                                                  c sqrt(121)); the gradient they feed keeps ssim_case's 2e-4 in the next line
    "ssim_grad": (4.4e-5, 2e-4),      # 1.10e-05 x 4   d SSIM / d img1, L = 121 (the same pair)                (ssim_case 2e-4)
}
# fp32 torch's absolute error x 4 where the reference is zero to rounding (an identical pair: maps and gradient are 1e-15 in float64)
LAYER_CONTRACT_FLOOR = {
    "ssim_map": 7.7e-6,               # 1.91e-06 x 4
    "ssim_grad": 6.5e-8,              # 1.61e-08 x 4
}
LAYER_CONTRACT_LOG = {}               # entry -> [accepted, refused, largest err / bound] (the tests print it)


def _layer_log(entry, accepted, ratio=0.0):
    row = LAYER_CONTRACT_LOG.setdefault(entry, [0, 0, 0.0])
    row[0 if accepted else 1] += 1
    row[2] = max(row[2], ratio) if ratio == ratio else float("inf")


def layer_bound(kind, ref, L, cond=0.0):
    """min(c sqrt(L), cap) max|ref| + c cond + floor.  cond: the size of the terms whose CANCELLATION gives the quantity, where the operation
    itself has one (the references state it: batch-norm's y = x sc + sh with sh = beta - mean sc; dx = gamma invstd (g - mean g - xhat mean(g xhat)),
    which vanishes identically at M <= 2; SSIM's variances E[x^2] - mu^2 under a denominator of 9e-4; a sum added onto a prefilled
    accumulator).  fp32 rounds each term to eps times ITS size, so no fp32 evaluation -- torch's included -- can be held to eps max|ref|
    there; the constants c were measured against the same expression."""
    c, cap = LAYER_CONTRACT_C[kind]
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return min(c * max(L, 1) ** 0.5, cap) * scale + c * float(cond) + LAYER_CONTRACT_FLOOR.get(kind, 0.0)


def layer_err(got, ref):
    """max |got - ref| in float64; NaN (a poisoned output) when any element is NaN."""
    if ref.numel() == 0:
        return 0.0
    d = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    return float("nan") if bool(torch.isnan(d).any()) else float(d.max())


def layer_passes(kind, got, ref, L, cond=0.0):
    """The comparator itself (the detection check feeds it references with one contribution removed)."""
    return layer_err(got, ref) <= layer_bound(kind, ref, L, cond)


def _close_ref(entry, ref, name, got, tag, prefill=0.0):
    """got against ref[name] = (kind, L, tensor[, cond]).  prefill: what the accumulator held before the call (taken off `got` by the caller;
    the sum onto it is rounded at its size)."""
    q = ref[name]
    _layer_close(entry, q[0], got, q[2], q[1], f"{tag}: {entry} {name}", (q[3] if len(q) > 3 else 0.0) + abs(prefill))


def _slots_clean(buf, C, what):
    """The self-cleaning part of a statistics / reduction buffer: the 32 slots and the 64 arrival counters behind them (include/hifihr.h).
    The last 2 C floats are plain scratch of the wide-layer backward (written before they are read)."""
    assert float(buf[:32 * 4 * C + 64].abs().max()) == 0.0, what


def _layer_close(entry, kind, got, ref, L, what, cond=0.0):
    err, bound = layer_err(got, ref), layer_bound(kind, ref, L, cond)
    _layer_log(entry, True, (err / bound) if bound > 0 else (0.0 if err == 0 else float("inf")))
    assert err <= bound, f"{what}: err {err:.3e} vs bound {bound:.3e} (kind {kind}, max|ref| {float(ref.abs().max()) if ref.numel() else 0:.3e}, L {L})"


def _layer_equal(entry, got, want, what):
    _layer_log(entry, True, 0.0)
    assert got.shape == want.shape and torch.equal(got.cpu(), want.cpu()), f"{what}: not bit-identical"


def layer_contract_report(title, prefixes=("",)):
    """The tally of the entries whose names start with one of `prefixes`: accepted / refused calls and the largest err / bound; printed, and
    appended to layer_contract_tally.txt in the directory HIFIHR_REPORT_DIR names, when it names one."""
    rows = [(e, v) for e, v in sorted(LAYER_CONTRACT_LOG.items()) if e.startswith(tuple(prefixes))]
    lines = [f"layer contract, {title} (entry: accepted / refused calls, largest err / bound):"]
    lines += [f"  {e:28s} {a:5d} / {r:4d}   {worst:6.3f}" for e, (a, r, worst) in rows]
    print("\n" + "\n".join(lines))
    out = os.environ.get("HIFIHR_REPORT_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "layer_contract_tally.txt"), "a") as fh:
            fh.write("\n".join(lines) + "\n")


_CANARY = {torch.float32: -1234.5, torch.uint8: 0xA5, torch.int32: -1234567}
_POISON = {torch.float32: float("nan"), torch.uint8: 0xFF, torch.int32: 0x7FFFFFF0}


class Guards:
    """Tensors inside larger allocations: at least GUARD_FLOATS elements of margin on each side (1 KiB for fp32: the view keeps the
    16-byte -- and for the float64 statistic slots 8-byte -- alignment a plain allocation has; offset_floats shifts it on purpose)."""

    def __init__(self, device):
        self.device, self.outs = device, []

    def _place(self, n, dtype, fill, offset):
        whole = torch.full((GUARD_FLOATS + offset + n + GUARD_FLOATS,), fill, dtype=dtype, device=self.device)
        return whole, GUARD_FLOATS + offset, GUARD_FLOATS + offset + n

    def inp(self, t, offset_floats=0):
        """A copy of t whose surroundings are NaN (float) / out-of-range values (bytes, ints)."""
        if t is None:
            return None
        t = t.contiguous()
        whole, lo, hi = self._place(t.numel(), t.dtype, _POISON[t.dtype], offset_floats)
        view = whole[lo:hi].view(t.shape)
        view.copy_(t.to(self.device))
        return view

    def out(self, *shape, fill=None, dtype=torch.float32, offset_floats=0):
        """An output of `shape`: canary around it and -- unless `fill` gives the prefill -- inside it."""
        n = 1
        for s in shape:
            n *= int(s)
        canary = _CANARY[dtype]
        whole, lo, hi = self._place(n, dtype, canary, offset_floats)
        view = whole[lo:hi].view(*shape)
        if fill is not None:
            view.fill_(fill)
        self.outs.append((whole, lo, hi, canary))
        return view

    def intact(self, what):
        for whole, lo, hi, canary in self.outs:
            ok = bool((whole[:lo] == canary).all()) and bool((whole[hi:] == canary).all())
            assert ok, f"{what}: wrote outside an output (guard band changed)"

    def wholes(self):
        return [w for w, _, _, _ in self.outs]


def _refuses(entry, call, guards, what):
    _contract_rejects(call, guards.wholes(), what)
    _layer_log(entry, False)


def _is_canary(t):
    return bool((t == _CANARY[t.dtype]).all())


# ---- batch-norm ------------------------------------------------------------------------------------------------------------------
def bn_contract_expect(M, C):
    """include/hifihr.h: C % 4 == 0, 4 <= C <= 4096 for every batch-norm entry; hifihr_bn_bwd_apply C <= 512."""
    ok = M > 0 and C >= 4 and C % 4 == 0 and C <= 4096
    return {"bn_stats": ok, "bn_act_fwd": ok, "bn_act_eval": ok, "bn_act_bwd": ok, "bn_finalize_fwd": ok, "bn_bwd_apply": ok and C <= 512}


def bn_stem_contract_expect(N, H, W, C):
    """include/hifihr.h: the fused stem takes C % 4 == 0, C <= 512, H, W >= 2."""
    return N > 0 and H >= 2 and W >= 2 and C >= 4 and C % 4 == 0 and C <= 512


def bn_contract_inputs(M, C, residual, seed):
    gen = torch.Generator().manual_seed(seed)
    Cc = max(4, (C + 3) // 4 * 4)                              # refused channel counts still get buffers a 4-wide lane could touch
    x = torch.randn(M, Cc, generator=gen) * 1.5 + 0.3
    gamma = 1 + 0.1 * torch.randn(Cc, generator=gen); beta = 0.1 * torch.randn(Cc, generator=gen)
    res = torch.randn(M, Cc, generator=gen) if residual else None
    rm0, rv0 = torch.randn(Cc, generator=gen) * 0.1, 1 + 0.1 * torch.rand(Cc, generator=gen)
    gy = torch.randn(M, Cc, generator=gen)
    return dict(x=x, gamma=gamma, beta=beta, res=res, rm0=rm0, rv0=rv0, gy=gy)


def _act_fwd_bwd(z, gy, act, mask=None):
    """(y, g = gy * act'(z)) in z's dtype; act 1 takes the ReLU mask when given."""
    if act == 1:
        m = (z > 0) if mask is None else mask
        return z * m, gy * m
    if act == 2:
        s = torch.sigmoid(z)
        return z * s, gy * (s * (1 + z * (1 - s)))
    return z, gy


def bn_contract_ref(inp, act, eps, mom, dt=torch.float64, mask=None, drop_row=None):
    """Training-mode batch-norm + residual + activation and its backward on x[M][C], written out (no autograd: M = 1, where nn.BatchNorm2d
    raises, is defined by the same formulas -- variance 0, invstd = 1 / sqrt(eps), running variance updated with the biased value).
    Returns {name: (kind, L, tensor)} plus the intermediates z, xhat.  drop_row: that row is left out of the sums (detection check)."""
    x, gamma, beta, gy = (inp[k].to(dt) for k in ("x", "gamma", "beta", "gy"))
    res = inp["res"].to(dt) if inp["res"] is not None else None
    M = x.shape[0]
    xs = x if drop_row is None else torch.cat([x[:drop_row], x[drop_row + 1:]])
    s1, s2 = xs.sum(0), (xs * xs).sum(0)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = (var + eps).rsqrt()
    xhat = (x - mean) * invstd
    z = xhat * gamma + beta + (res if res is not None else 0)
    y, g = _act_fwd_bwd(z, gy, act, mask)
    gs = g if drop_row is None else torch.cat([g[:drop_row], g[drop_row + 1:]])
    xh = xhat if drop_row is None else torch.cat([xhat[:drop_row], xhat[drop_row + 1:]])
    dbeta, dgamma = gs.sum(0), (gs * xh).sum(0)
    dx = gamma * invstd * (g - g.sum(0) / M - xhat * (g * xhat).sum(0) / M)
    rm = (1 - mom) * inp["rm0"].to(dt) + mom * mean
    rv = (1 - mom) * inp["rv0"].to(dt) + mom * (var * (M / (M - 1)) if M > 1 else var)
    ze = (x - inp["rm0"].to(dt)) * (inp["rv0"].to(dt) + eps).rsqrt() * gamma + beta + (res if res is not None else 0)
    ye, _ = _act_fwd_bwd(ze, gy, act)
    # the cancelling terms (layer_bound): y = x sc + sh, the two of size |mean| sc; dx's three terms of size gamma invstd |g|; xhat inside dgamma
    gmax = float(g.abs().max())
    cy = float((mean * invstd * gamma).abs().max())
    cye = float((inp["rm0"].to(dt) * (inp["rv0"].to(dt) + eps).rsqrt() * gamma).abs().max())
    cz = float(gy.abs().max()) * cy if act == 2 else 0.0                  # swish' recomputed from z = x sc + sh (|swish''| <= 1/2)
    cdx = float((gamma * invstd).abs().max()) * (gmax + cz)
    cdg = (float((mean * invstd).abs().max()) * gmax + cz) * M ** 0.5
    out = {"sum": ("bn_sum", M, s1), "sumsq": ("bn_sum", M, s2), "mean": ("bn_stat", 1, mean), "invstd": ("bn_stat", 1, invstd),
           "rm": ("bn_stat", 1, rm), "rv": ("bn_stat", 1, rv), "y": ("bn_y", 1, y, cy), "y_eval": ("bn_y", 1, ye, cye), "dx": ("bn_dx", 1, dx, cdx),
           "dgamma": ("bn_dparam", M, dgamma, cdg), "dbeta": ("bn_dparam", M, dbeta, cz * M ** 0.5)}
    return out, dict(z=z, ze=ze, xhat=xhat, g=g)


def _relu_mask(z64, y_got, what):
    """The ReLU mask of the float64 reference, with the kernel's own decision (y > 0) where fp32 cannot tell the sign of z: |z| within
    4e-6 max(1, max|z|) (the bound on y itself).  Outside that zone the two must agree."""
    amb = z64.abs() <= 4e-6 * max(1.0, float(z64.abs().max()))
    m_ref, m_got = z64 > 0, y_got.cpu().reshape(z64.shape) > 0
    assert bool((m_ref == m_got)[~amb].all()), f"{what}: ReLU zero pattern differs where the sign of z is not in doubt"
    return torch.where(amb, m_got, m_ref)


def bn_contract_case(lib, device, M, C, act=0, residual=False, y_given=True, running=True, eps=1e-5, mom=0.1, seed=0):
    """Every plain batch-norm entry on x[M][C].  Returns {entry: accepted}."""
    expect = bn_contract_expect(M, C)
    inp = bn_contract_inputs(M, C, residual, seed)
    Cc = inp["x"].shape[1]
    tag = f"bn M={M} C={C} act={act} res={residual}"
    G = Guards(device)
    x, gamma, beta, res, gy = (G.inp(inp[k]) for k in ("x", "gamma", "beta", "res", "gy"))
    nst = max(lib.bn_stats_floats(C), lib.bn_stats_floats(Cc))
    stats = G.out(nst, fill=0.0)
    y, sm, si = G.out(M, Cc), G.out(Cc), G.out(Cc)
    rm, rv = G.out(Cc), G.out(Cc)
    args_ok = not (act == 2 and residual)
    if not expect["bn_stats"]:
        _refuses("bn_stats", lambda: lib.bn_stats(x, M, C, stats), G, tag)
        _refuses("bn_act_fwd", lambda: lib.bn_act_fwd(x, stats, gamma, beta, res, act, M, C, eps, mom, y, sm, si, rm, rv), G, tag)
        _refuses("bn_act_eval", lambda: lib.bn_act_eval(x, gamma, beta, gamma, beta, res, act, M, C, eps, y), G, tag)
        _refuses("bn_finalize_fwd", lambda: lib.bn_finalize_fwd(stats, M, C, eps, mom, sm, si, rm, rv), G, tag)
        dxo, dgm, dbt = G.out(M, Cc), G.out(Cc), G.out(Cc)
        _refuses("bn_act_bwd", lambda: lib.bn_act_bwd(gy, None, x, gamma, beta, gamma, beta, act, M, C, stats, dxo, None, dgm, dbt), G, tag)
        _refuses("bn_bwd_apply", lambda: lib.bn_bwd_apply(gy, x, gamma, beta, gamma, M, C, stats, dxo, dgm, dbt), G, tag)
        assert float(stats.abs().max()) == 0.0
        return {e: False for e in expect}
    if not args_ok:                                             # swish takes no residual: refused by the forward and the evaluation entry
        _refuses("bn_act_fwd", lambda: lib.bn_act_fwd(x, stats, gamma, beta, res, act, M, C, eps, mom, y, sm, si, rm, rv), G, tag + " swish + residual")
        _refuses("bn_act_eval", lambda: lib.bn_act_eval(x, gamma, beta, gamma, beta, res, act, M, C, eps, y), G, tag + " swish + residual")
        return {"bn_act_fwd": False, "bn_act_eval": False}
    ref, mid = bn_contract_ref(inp, act, eps, mom)
    close = lambda entry, name, got: _close_ref(entry, ref, name, got, tag)
    # one running statistic without the other is refused
    _refuses("bn_act_fwd", lambda: lib.bn_act_fwd(x, stats, gamma, beta, res, act, M, C, eps, mom, y, sm, si, rm, None), G, tag + " one running statistic")
    _refuses("bn_finalize_fwd", lambda: lib.bn_finalize_fwd(stats, M, C, eps, mom, sm, si, None, rv), G, tag + " one running statistic")
    ys = []
    for rep in range(2):                                       # twice on the same slot buffer
        lib.bn_stats(x, M, C, stats)
        sl = bn_slots(stats, C).sum(0).cpu()
        close("bn_stats", "sum", sl[0]); close("bn_stats", "sumsq", sl[1])
        rm.copy_(inp["rm0"]); rv.copy_(inp["rv0"])
        y.fill_(_CANARY[torch.float32])
        lib.bn_act_fwd(x, stats, gamma, beta, res, act, M, C, eps, mom, y, sm, si, rm if running else None, rv if running else None)
        assert float(stats.abs().max()) == 0.0, f"{tag}: bn_act_fwd must hand the whole slot buffer back zeroed (call {rep + 1})"
        close("bn_act_fwd", "y", y); close("bn_act_fwd", "mean", sm); close("bn_act_fwd", "invstd", si)
        if running:
            close("bn_act_fwd", "rm", rm); close("bn_act_fwd", "rv", rv)
        else:
            assert torch.equal(rm.cpu(), inp["rm0"]) and torch.equal(rv.cpu(), inp["rv0"])
        ys.append(y.clone())
    G.intact(tag + " forward")
    # the statistics half alone: the same save_mean / save_invstd bits as the fused apply, the slots handed back zeroed
    sm2, si2, rm2, rv2 = G.out(Cc), G.out(Cc), G.out(Cc), G.out(Cc)
    rm2.copy_(inp["rm0"]); rv2.copy_(inp["rv0"])
    lib.bn_stats(x, M, C, stats)
    lib.bn_finalize_fwd(stats, M, C, eps, mom, sm2, si2, rm2 if running else None, rv2 if running else None)
    assert float(stats.abs().max()) == 0.0, f"{tag}: bn_finalize_fwd must hand the whole slot buffer back zeroed"
    close("bn_finalize_fwd", "mean", sm2); close("bn_finalize_fwd", "invstd", si2)
    if running:
        close("bn_finalize_fwd", "rm", rm2); close("bn_finalize_fwd", "rv", rv2)
    # evaluation mode: running statistics in, nothing updated, no atomics -> two calls agree to the bit
    rm0, rv0 = G.inp(inp["rm0"]), G.inp(inp["rv0"])
    ye, ye2 = G.out(M, Cc), G.out(M, Cc)
    lib.bn_act_eval(x, rm0, rv0, gamma, beta, res, act, M, C, eps, ye)
    lib.bn_act_eval(x, rm0, rv0, gamma, beta, res, act, M, C, eps, ye2)
    close("bn_act_eval", "y_eval", ye)
    _layer_equal("bn_act_eval", ye2, ye, f"{tag}: bn_act_eval twice")
    # backward: the ReLU mask is the forward's own where fp32 cannot tell the sign
    if act == 1:
        ref, mid = bn_contract_ref(inp, act, eps, mom, mask=_relu_mask(mid["z"], y, tag))
    use_y = act == 1 and (y_given or residual)
    if act == 1 and not use_y:
        _refuses("bn_act_bwd", lambda: lib.bn_act_bwd(gy, None, x, sm, si, gamma, None, 1, M, C, stats, y, None, None, None), G, tag + " act 1 without y and beta")
    dxo, dres = G.out(M, Cc), (G.out(M, Cc) if residual else None)
    dgm, dbt = G.out(Cc), G.out(Cc)
    for rep in range(2):
        dgm.fill_(0.5); dbt.fill_(-0.25); dxo.fill_(_CANARY[torch.float32])
        lib.bn_act_bwd(gy, y if use_y else None, x, sm, si, gamma, beta, act, M, C, stats, dxo, dres, dgm, dbt)
        _slots_clean(stats, C, f"{tag}: bn_act_bwd must hand the slots and arrival counters back zeroed (call {rep + 1})")
        close("bn_act_bwd", "dx", dxo)
        _close_ref("bn_act_bwd", ref, "dgamma", dgm.cpu().double() - 0.5, tag, 0.5); _close_ref("bn_act_bwd", ref, "dbeta", dbt.cpu().double() + 0.25, tag, 0.25)
        if residual:
            _layer_equal("bn_act_bwd", dres, mid["g"].float(), f"{tag}: dres = g")
    lib.bn_act_bwd(gy, y if use_y else None, x, sm, si, gamma, beta, act, M, C, stats, dxo, None, None, None)      # dgamma / dbeta may be NULL
    close("bn_act_bwd", "dx", dxo)
    # the apply half alone (C <= 512): g is the masked gradient, the first slot of red holds (sum g, sum g xhat)
    g32 = G.inp(mid["g"].float())
    red_fill = torch.zeros(nst)
    red_fill[:2 * C] = torch.cat([ref["dbeta"][2], ref["dgamma"][2]]).float()
    dxa = G.out(M, Cc)
    if expect["bn_bwd_apply"]:
        for rep in range(2):
            stats.copy_(red_fill); dgm.fill_(0.5); dbt.fill_(-0.25)
            lib.bn_bwd_apply(g32, x, sm, si, gamma, M, C, stats, dxa, dgm, dbt)
            _slots_clean(stats, C, f"{tag}: bn_bwd_apply must hand the slots and arrival counters back zeroed")
            close("bn_bwd_apply", "dx", dxa)
            _close_ref("bn_bwd_apply", ref, "dgamma", dgm.cpu().double() - 0.5, tag, 0.5); _close_ref("bn_bwd_apply", ref, "dbeta", dbt.cpu().double() + 0.25, tag, 0.25)
    else:
        _refuses("bn_bwd_apply", lambda: lib.bn_bwd_apply(g32, x, sm, si, gamma, M, C, stats, dxa, dgm, dbt), G, tag)
    G.intact(tag)
    return dict(expect)


def bn_stem_contract_inputs(N, H, W, C, seed):
    gen = torch.Generator().manual_seed(seed)
    Cc = max(4, (C + 3) // 4 * 4)
    x = torch.randn(N, H, W, Cc, generator=gen) * 1.5 + 0.3
    gamma = 1 + 0.1 * torch.randn(Cc, generator=gen); beta = 0.1 * torch.randn(Cc, generator=gen) - 0.3     # plenty of ReLU zeros: ties
    gamma[1] = 2e-4; beta[1] = 0.05                      # a near-zero scale (positive shift: every tap passes the ReLU)
    gamma[2] = -0.8                                      # a negative scale: the winner is the SMALLEST x of the window
    rm0, rv0 = torch.randn(Cc, generator=gen) * 0.1, 1 + 0.1 * torch.rand(Cc, generator=gen)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, OH, OW, Cc, generator=gen)
    return dict(x=x.reshape(-1, Cc), gamma=gamma, beta=beta, res=None, rm0=rm0, rv0=rv0, gy=gy)


def _pool_scatter(gy, tap, N, H, W, k, s, p):
    """dz[N][H][W][C] (float64) = the pooled gradient gy[N][OH][OW][C] scattered to the winning taps (tap = r * k + s bytes)."""
    OH, OW, C = gy.shape[1], gy.shape[2], gy.shape[3]
    t = tap.cpu().reshape(N, OH, OW, C).long()
    oh = torch.arange(OH).view(1, OH, 1, 1); ow = torch.arange(OW).view(1, 1, OW, 1)
    ih, iw = oh * s - p + t // k, ow * s - p + t % k
    assert bool(((ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)).all()), "a winning tap outside the image"
    n = torch.arange(N).view(N, 1, 1, 1).expand_as(t); c = torch.arange(C).view(1, 1, 1, C).expand_as(t)
    dz = torch.zeros(N, H, W, C, dtype=torch.float64)
    dz.index_put_((n, ih.expand_as(t), iw.expand_as(t), c), gy.double(), accumulate=True)
    return dz, (n, ih.expand_as(t), iw.expand_as(t), c)


def bn_stem_contract_case(lib, device, N, H, W, C, seed=0, eps=1e-5, mom=0.1):
    """hifihr_bn_relu_maxpool_fwd / _bwd / _bwd_y: MaxPool2d(3, 2, 1)(relu(bn(x))).  The forward equals bn_act_fwd + maxpool2d_fwd of the same
    library bit for bit and the float64 reference within the bound; the winning taps are the kernel's own, each checked to hold its window's
    float64 maximum to the bound of y (fp32 cannot order closer values), and the backward reference scatters through them."""
    accepted = bn_stem_contract_expect(N, H, W, C)
    assert lib.bn_relu_maxpool_supported(N, H, W, C) == accepted, f"bn_relu_maxpool_supported({N}, {H}, {W}, {C})"
    inp = bn_stem_contract_inputs(N, H, W, C, seed)
    Cc, M = inp["x"].shape[1], N * H * W
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    tag = f"bn stem {N}x{H}x{W}x{C}"
    G = Guards(device)
    x, gamma, beta, gy = (G.inp(inp[k]) for k in ("x", "gamma", "beta", "gy"))
    nst = max(lib.bn_stats_floats(C), lib.bn_stats_floats(Cc))
    stats = G.out(nst, fill=0.0)
    y, tap = G.out(N, OH, OW, Cc), G.out(N * OH * OW * Cc, dtype=torch.uint8)
    sm, si, rm, rv = G.out(Cc), G.out(Cc), G.out(Cc), G.out(Cc)
    dx, dgm, dbt = G.out(N, H, W, Cc), G.out(Cc), G.out(Cc)
    if not accepted:
        _refuses("bn_relu_maxpool_fwd", lambda: lib.bn_relu_maxpool_fwd(x, stats, gamma, beta, N, H, W, C, eps, mom, y, tap, sm, si, rm, rv), G, tag)
        _refuses("bn_relu_maxpool_bwd", lambda: lib.bn_relu_maxpool_bwd(gy, tap, x, gamma, beta, gamma, beta, N, H, W, C, stats, dx, dgm, dbt), G, tag)
        _refuses("bn_relu_maxpool_bwd_y", lambda: lib.bn_relu_maxpool_bwd_y(gy, y, tap, x, gamma, beta, gamma, beta, N, H, W, C, stats, dx, dgm, dbt), G, tag)
        return False
    ref, mid = bn_contract_ref(dict(inp, gy=torch.zeros(M, Cc)), 1, eps, mom)
    close = lambda entry, name, got: _close_ref(entry, ref, name, got, tag)
    for rep in range(2):
        lib.bn_stats(x, M, C, stats)
        stats2 = stats.clone()
        rm.copy_(inp["rm0"]); rv.copy_(inp["rv0"])
        lib.bn_relu_maxpool_fwd(x, stats, gamma, beta, N, H, W, C, eps, mom, y, tap, sm, si, rm, rv)
        assert float(stats.abs().max()) == 0.0, f"{tag}: the fused stem forward must hand the whole slot buffer back zeroed"
        for name, got in (("mean", sm), ("invstd", si), ("rm", rm), ("rv", rv)):
            close("bn_relu_maxpool_fwd", name, got)
    # the unfused pair of the same library: the same bits
    yf, sm2, si2 = G.out(M, Cc), G.out(Cc), G.out(Cc)
    lib.bn_act_fwd(x, stats2, gamma, beta, None, 1, M, C, eps, mom, yf, sm2, si2, None, None)
    y2, tap2 = G.out(N, OH, OW, Cc), G.out(N * OH * OW * Cc, dtype=torch.uint8)
    lib.maxpool2d_fwd(yf, N, H, W, C, 3, 2, 1, y2, tap2)
    _layer_equal("bn_relu_maxpool_fwd", torch.cat([sm, si]), torch.cat([sm2, si2]), f"{tag}: batch statistics vs bn_act_fwd")
    _layer_equal("bn_relu_maxpool_fwd", y, y2, f"{tag}: pooled vs bn_act_fwd + maxpool2d_fwd")
    _layer_equal("bn_relu_maxpool_fwd", tap, tap2, f"{tag}: taps vs bn_act_fwd + maxpool2d_fwd")
    # float64: each winning tap holds its window's maximum of relu(z), the pooled value is that maximum
    import torch.nn.functional as F
    a64 = torch.relu(mid["z"]).reshape(N, H, W, Cc)
    pooled64 = F.max_pool2d(a64.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    _layer_close("bn_relu_maxpool_fwd", "bn_y", y, pooled64, 1, f"{tag}: pooled", ref["y"][3])
    _, where = _pool_scatter(inp["gy"], tap, N, H, W, 3, 2, 1)
    slack = layer_bound("bn_y", a64, 1, ref["y"][3])
    assert float((pooled64 - a64[where]).abs().max()) <= 2 * slack + 1e-300, f"{tag}: a winning tap does not hold its window's maximum"
    # backward: scatter through the kernel's taps, ReLU mask as in bn_contract_case, then the batch-norm backward in float64
    dz, _ = _pool_scatter(inp["gy"], tap, N, H, W, 3, 2, 1)
    full = dict(inp, gy=dz.reshape(M, Cc))
    mask = _relu_mask(mid["z"], yf, tag)
    refb, _ = bn_contract_ref(full, 1, eps, mom, mask=mask)
    for entry, call in (("bn_relu_maxpool_bwd", lambda: lib.bn_relu_maxpool_bwd(gy, tap, x, sm, si, gamma, beta, N, H, W, C, stats, dx, dgm, dbt)),
                        ("bn_relu_maxpool_bwd_y", lambda: lib.bn_relu_maxpool_bwd_y(gy, y, tap, x, sm, si, gamma, beta, N, H, W, C, stats, dx, dgm, dbt))):
        for rep in range(2):
            dx.fill_(_CANARY[torch.float32]); dgm.fill_(0.5); dbt.fill_(-0.25)
            call()
            _slots_clean(stats, C, f"{tag}: {entry} must hand the slots and arrival counters back zeroed")
            _close_ref(entry, refb, "dx", dx, tag)
            _close_ref(entry, refb, "dgamma", dgm.cpu().double() - 0.5, tag, 0.5)
            _close_ref(entry, refb, "dbeta", dbt.cpu().double() + 0.25, tag, 0.25)
    G.intact(tag)
    return True


# ---- pooling -----------------------------------------------------------------------------------------------------------------------
POOL_KSP = ((3, 2, 1), (3, 1, 1), (2, 2, 0))


def pool_contract_expect(N, H, W, C, k, s, p):
    """include/hifihr.h: C % 4 == 0; the tapped entries take (k, s, p) in {(3,2,1), (3,1,1), (2,2,0)}, the inference pool (3,2,0) alone;
    the padded image must hold one window."""
    ok = min(N, H, W) > 0 and C >= 4 and C % 4 == 0 and H + 2 * p >= k and W + 2 * p >= k
    tapped = ok and (k, s, p) in POOL_KSP
    return {"maxpool2d_fwd": tapped, "maxpool2d_bwd": tapped, "maxpool2d_bwd_relu": tapped, "maxpool2d_fwd_flat": tapped,
            "maxpool2d_bwd_flat": tapped, "maxpool2d_fwd_notap": ok and (k, s, p) == (3, 2, 0)}


def _taps_of(idx, OH, OW, W, k, s, p):
    """ATen's flat winner index [N][C][OH][OW] -> the tap byte r * k + s in [N][OH][OW][C] order."""
    oh = torch.arange(OH).view(1, 1, OH, 1); ow = torch.arange(OW).view(1, 1, 1, OW)
    r, c = idx // W - (oh * s - p), idx % W - (ow * s - p)
    return (r * k + c).permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def _same_values(got, want):
    got, want = got.cpu(), want.cpu()
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


def pool_contract_case(lib, device, N, H, W, C, k, s, p, mode="random", seed=0):
    """The six max-pool entries on one geometry.  mode: random / ties (post-ReLU zeros) / special (a window of -inf, a NaN: forward only,
    ATen's `(val > max) || isnan(val)` rule and index).  Values, taps, the flat forms and a second call: bit-identical."""
    import torch.nn.functional as F
    expect = pool_contract_expect(N, H, W, C, k, s, p)
    gen = torch.Generator().manual_seed(seed)
    Cc = max(4, (C + 3) // 4 * 4)
    tag = f"pool {N}x{H}x{W}x{C} ({k},{s},{p}) {mode}"
    z = torch.randn(N, H, W, Cc, generator=gen)
    x = torch.relu(z) if mode == "ties" else z.clone()
    if mode == "special":
        x[:, :min(H, 3), :min(W, 3), :] = float("-inf")          # the first window(s): every in-range tap -inf
        x[-1, H // 2, W // 2, 1] = float("nan")
        x[0, -1, -1, 2] = float("nan")
    OHt, OWt = (H + 2 * p - k) // s + 1 if s > 0 else 0, (W + 2 * p - k) // s + 1 if s > 0 else 0        # the documented size (floor; may be <= 0)
    OHa, OWa = max(OHt, 1), max(OWt, 1)                                                                 # buffers for refused calls
    G = Guards(device)
    xd = G.inp(x)
    y, tap = G.out(N, OHa, OWa, Cc), G.out(N * OHa * OWa * Cc, dtype=torch.uint8)
    yflat, tapf = G.out(N, Cc * OHa * OWa), G.out(N * OHa * OWa * Cc, dtype=torch.uint8)
    dx, dxf, dxr = G.out(N, H, W, Cc), G.out(N, H, W, Cc), G.out(N, H, W, Cc)
    gy_t = torch.randn(N, OHa, OWa, Cc, generator=gen)
    gy = G.inp(gy_t)
    gyflat = G.inp(gy_t.permute(0, 3, 1, 2).reshape(N, -1))
    tap_in = G.inp(torch.zeros(N * OHa * OWa * Cc, dtype=torch.uint8))
    ypos = G.inp(torch.ones(N, OHa, OWa, Cc))
    calls = {"maxpool2d_fwd": lambda: lib.maxpool2d_fwd(xd, N, H, W, C, k, s, p, y, tap),
             "maxpool2d_fwd_flat": lambda: lib.maxpool2d_fwd_flat(xd, N, H, W, C, k, s, p, yflat, tapf),
             "maxpool2d_bwd": lambda: lib.maxpool2d_bwd(gy, tap_in, N, H, W, C, k, s, p, dx),
             "maxpool2d_bwd_flat": lambda: lib.maxpool2d_bwd_flat(gyflat, tap_in, N, H, W, C, k, s, p, dxf),
             "maxpool2d_bwd_relu": lambda: lib.maxpool2d_bwd(gy, tap_in, N, H, W, C, k, s, p, dxr, relu_y=ypos)}
    ynt = G.out(N, OHa, OWa, Cc)
    if expect["maxpool2d_fwd_notap"]:
        ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
        for rep in range(2):
            ynt.fill_(_CANARY[torch.float32])
            lib.maxpool2d_fwd_notap(xd, N, H, W, C, k, s, p, ynt)
            _layer_log("maxpool2d_fwd_notap", True)
            assert _same_values(ynt, ref.float()), f"{tag}: maxpool2d_fwd_notap values"
        ynt.fill_(_CANARY[torch.float32])                      # (a NaN output would make the refusals' before / after comparison fail)
    else:
        _refuses("maxpool2d_fwd_notap", lambda: lib.maxpool2d_fwd_notap(xd, N, H, W, C, k, s, p, ynt), G, tag)
    if not expect["maxpool2d_fwd"]:
        for e, call in calls.items():
            _refuses(e, call, G, f"{tag}: {e}")
        G.intact(tag)
        return expect
    assert (OHt, OWt) == (OHa, OWa)
    ref, idx = F.max_pool2d(x.double().permute(0, 3, 1, 2), k, s, p, return_indices=True)
    ref, taps = ref.permute(0, 2, 3, 1).float(), _taps_of(idx, OHt, OWt, W, k, s, p)
    for rep in range(2):
        y.fill_(_CANARY[torch.float32]); yflat.fill_(_CANARY[torch.float32])
        calls["maxpool2d_fwd"](); calls["maxpool2d_fwd_flat"]()
        _layer_log("maxpool2d_fwd", True); _layer_log("maxpool2d_fwd_flat", True)
        assert _same_values(y, ref), f"{tag}: maxpool2d_fwd values"
        assert torch.equal(tap.cpu().view(N, OHt, OWt, Cc), taps), f"{tag}: winning taps (ATen's rule and index)"
        assert _same_values(yflat, ref.permute(0, 3, 1, 2).reshape(N, -1)), f"{tag}: maxpool2d_fwd_flat values"
        assert torch.equal(tapf, tap), f"{tag}: maxpool2d_fwd_flat taps"
    if mode != "special":
        # float64 autograd of the pool; with ties ATen's winner is the tap the kernels recorded (checked above)
        xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.max_pool2d(xr, k, s, p).backward(gy_t.double().permute(0, 3, 1, 2))
        refdx = xr.grad.permute(0, 2, 3, 1)
        zr = z.double().permute(0, 3, 1, 2).clone().requires_grad_(True)          # pool(relu(z)): x = relu(z) is the pool's input
        F.max_pool2d(torch.relu(zr), k, s, p).backward(gy_t.double().permute(0, 3, 1, 2))
        refdz = zr.grad.permute(0, 2, 3, 1)
        xrelu = G.inp(torch.relu(z))
        yr, tapr = G.out(N, OHt, OWt, Cc), G.out(N * OHt * OWt * Cc, dtype=torch.uint8)
        lib.maxpool2d_fwd(xrelu, N, H, W, C, k, s, p, yr, tapr)
        Ldx = ((k + s - 1) // s) ** 2
        for rep in range(2):
            for t in (dx, dxf, dxr):
                t.fill_(_CANARY[torch.float32])                                     # overwritten, not accumulated
            lib.maxpool2d_bwd(gy, tap, N, H, W, C, k, s, p, dx)
            lib.maxpool2d_bwd_flat(gyflat, tap, N, H, W, C, k, s, p, dxf)
            lib.maxpool2d_bwd(gy, tapr, N, H, W, C, k, s, p, dxr, relu_y=yr)
            _layer_close("maxpool2d_bwd", "pool_dx", dx, refdx, Ldx, f"{tag}: maxpool2d_bwd")
            _layer_equal("maxpool2d_bwd_flat", dxf, dx, f"{tag}: maxpool2d_bwd_flat vs maxpool2d_bwd")
            _layer_close("maxpool2d_bwd_relu", "pool_dx", dxr, refdz, Ldx, f"{tag}: maxpool2d_bwd_relu vs autograd of max_pool2d(relu(z))")
    G.intact(tag)
    return expect


def mmpool_contract_expect(B, HW, C):
    return B > 0 and HW > 0 and C >= 4 and C % 4 == 0


def mmpool_contract_ref(x, p0, gy, dt=torch.float64, drop_pixel=None):
    """MMPool((1, 1)) on x[B][HW][C] and its backward, written out; the argmax is the first maximum in scan order."""
    x, gy = x.to(dt), gy.to(dt)
    B, HW, C = x.shape
    w = torch.sigmoid(torch.tensor(p0, dtype=dt))
    xmax, am = x.max(1)
    am = (x == xmax.unsqueeze(1)).to(torch.int64).argmax(1)          # first maximum (torch.max's choice among ties is not specified)
    xs = x if drop_pixel is None else torch.cat([x[:, :drop_pixel], x[:, drop_pixel + 1:]], 1)
    xavg = xs.sum(1) / HW
    y = xmax * w + xavg * (1 - w)
    dx = (gy * (1 - w) / HW).unsqueeze(1).expand(B, HW, C).clone()
    dx.scatter_add_(1, am.unsqueeze(1), (gy * w).unsqueeze(1))
    S = (gy * (xmax - xavg)).sum()
    dp = S * w * (1 - w)                                              # (1 - w cancels for large p: the term S w is what fp32 rounds)
    return {"y": ("mm_y", HW, y), "xavg": ("mm_y", HW, xavg), "xmax": xmax, "argmax": am, "dx": ("mm_dx", 1, dx), "dp": ("mm_dp", B * C, dp.reshape(1), float((S * w).abs()))}


def mmpool_contract_inputs(B, HW, C, ties, seed):
    gen = torch.Generator().manual_seed(seed)
    Cc = max(4, (C + 3) // 4 * 4)
    x = torch.randn(B, HW, Cc, generator=gen)
    if ties:
        x = torch.relu(x - 0.5)
    return x, torch.randn(B, Cc, generator=gen)


def mmpool_contract_case(lib, device, B, HW, C, p0=0.3, ties=False, seed=0):
    accepted = mmpool_contract_expect(B, HW, C)
    x_t, gy_t = mmpool_contract_inputs(B, HW, C, ties, seed)
    Cc = x_t.shape[2]
    tag = f"mmpool B={B} HW={HW} C={C} p={p0} ties={ties}"
    G = Guards(device)
    x, gy, pd = G.inp(x_t), G.inp(gy_t), G.inp(torch.tensor([p0]))
    y, am, xmax, xavg = G.out(B, Cc), G.out(B, Cc, dtype=torch.int32), G.out(B, Cc), G.out(B, Cc)
    dx, dp = G.out(B, HW, Cc), G.out(1)
    if not accepted:
        _refuses("mmpool_fwd", lambda: lib.mmpool_fwd(x, pd, B, HW, C, y, am, xmax, xavg), G, tag)
        _refuses("mmpool_bwd", lambda: lib.mmpool_bwd(gy, pd, G.inp(torch.zeros(B, Cc, dtype=torch.int32)), gy, gy, B, HW, C, dx, dp), G, tag)
        return False
    ref = mmpool_contract_ref(x_t, p0, gy_t)
    close = lambda entry, name, got: _close_ref(entry, ref, name, got, tag)
    for rep in range(2):
        lib.mmpool_fwd(x, pd, B, HW, C, y, am, xmax, xavg)
        close("mmpool_fwd", "y", y); close("mmpool_fwd", "xavg", xavg)
        _layer_equal("mmpool_fwd", xmax, ref["xmax"].float(), f"{tag}: xmax")
        _layer_equal("mmpool_fwd", am.long(), ref["argmax"], f"{tag}: argmax (first maximum in scan order)")
        dx.fill_(_CANARY[torch.float32]); dp.fill_(0.25)
        lib.mmpool_bwd(gy, pd, am, xmax, xavg, B, HW, C, dx, dp)
        close("mmpool_bwd", "dx", dx); _close_ref("mmpool_bwd", ref, "dp", dp.cpu().double() - 0.25, tag, 0.25)
    dx2 = G.out(B, HW, Cc)
    lib.mmpool_bwd(gy, pd, am, xmax, xavg, B, HW, C, dx2, None)                  # dp_acc may be NULL
    _layer_equal("mmpool_bwd", dx2, dx, f"{tag}: dx with dp_acc NULL")
    G.intact(tag)
    return True


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------
def dw_same_geom(N, H, W, C, K, stride):
    """TensorFlow 'same' padding for this very input size: (N, H, W, C, K, stride, pad_top, pad_left, OH, OW)."""
    OH, OW = -(-H // stride), -(-W // stride)
    ph, pw = max((OH - 1) * stride + K - H, 0), max((OW - 1) * stride + K - W, 0)
    return (N, H, W, C, K, stride, ph // 2, pw // 2, OH, OW)


def dw_pad_geom(N, H, W, C, K, stride, pad):
    """Symmetric explicit padding `pad` as nn.Conv2d counts the output (floor)."""
    return (N, H, W, C, K, stride, pad, pad, (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1)


def dw_contract_expect(N, H, W, C, K, stride, pt, pl, OH, OW):
    """include/hifihr.h: C % 4 == 0, K 3 or 5, stride 1 or 2, 0 <= pad_top <= K - 1 and the implied bottom pad
    (OH - 1) stride + K - H - pad_top within [-(stride - 1), K - 1] (columns alike).  All five entries take the same set."""
    def axis(I, O, pad):
        return I > 0 and O > 0 and 0 <= pad <= K - 1 and -(stride - 1) <= (O - 1) * stride + K - I - pad <= K - 1
    return N > 0 and C >= 4 and C % 4 == 0 and K in (3, 5) and stride in (1, 2) and axis(H, OH, pt) and axis(W, OW, pl)


def dw_contract_inputs(N, H, W, C, K, OH, OW, seed):
    gen = torch.Generator().manual_seed(seed)
    Cc, Kc, OHc, OWc = max(4, (C + 3) // 4 * 4), max(K, 1), max(OH, 1), max(OW, 1)
    x = torch.randn(N, H, W, Cc, generator=gen) * 1.5 + 0.3
    w = torch.randn(Cc, Kc, Kc, generator=gen) / Kc
    gy = torch.randn(N, OHc, OWc, Cc, generator=gen)
    mean, invstd = 0.3 + 0.2 * torch.randn(Cc, generator=gen), 1 / (1.5 + 0.2 * torch.rand(Cc, generator=gen))
    gamma, beta = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen) * 0.3
    return dict(x=x, w=w, gy=gy, mean=mean, invstd=invstd, gamma=gamma, beta=beta)


def dw_contract_ref(inp, geom, pre, dt=torch.float64, drop_tap=False):
    """F.pad with the implied bottom / right padding + grouped F.conv2d in `dt`, gradients by autograd.  pre: the input is
    swish(x * sc + sh) with sc = invstd gamma, sh = beta - mean sc (batch-norm + swish on load).  drop_tap: one filter tap is zeroed
    (detection check)."""
    import torch.nn.functional as F
    N, H, W, C, K, stride, pt, pl, OH, OW = geom
    x = inp["x"].to(dt).permute(0, 3, 1, 2)
    w = inp["w"].to(dt).clone()
    if drop_tap:
        w[:, pt, pl] = 0                                          # the tap that meets pixel (0, 0) at output (0, 0): in range on every geometry
    wr = w.reshape(C, 1, K, K).requires_grad_(True)
    if pre:
        sc = inp["invstd"].to(dt) * inp["gamma"].to(dt)
        sh = inp["beta"].to(dt) - inp["mean"].to(dt) * sc
        z = x * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1)
        a = z * torch.sigmoid(z)
    else:
        a = x
    a = a.detach().requires_grad_(True)
    pb, pr = (OH - 1) * stride + K - H - pt, (OW - 1) * stride + K - W - pl
    y = F.conv2d(F.pad(a, (pl, max(pr, 0), pt, max(pb, 0))), wr, None, stride, 0, 1, C)
    assert y.shape[2:] == (OH, OW), (y.shape, geom)
    y.backward(inp["gy"].to(dt).permute(0, 3, 1, 2))
    yn = y.detach().permute(0, 2, 3, 1)
    flat = yn.reshape(-1, C)
    Ly = N * OH * OW
    return {"y": ("dw_pre" if pre else "dw_fwd", K * K, yn), "sum": ("bn_sum", Ly, flat.sum(0)), "sumsq": ("bn_sum", Ly, (flat * flat).sum(0)),
            "dx": ("dw_dgrad", K * K, a.grad.permute(0, 2, 3, 1)), "dw": ("dw_wgrad_pre" if pre else "dw_wgrad", Ly, wr.grad.reshape(C, K, K))}


def dw_contract_case(lib, device, N, H, W, C, K, stride, pt, pl, OH, OW, seed=0):
    """The five depthwise entries on one geometry.  Returns accepted."""
    geom = (N, H, W, C, K, stride, pt, pl, OH, OW)
    accepted = dw_contract_expect(*geom)
    inp = dw_contract_inputs(N, H, W, C, K, OH, OW, seed)
    Cc, OHc, OWc = inp["x"].shape[3], inp["gy"].shape[1], inp["gy"].shape[2]
    tag = "dw " + "x".join(map(str, geom))
    G = Guards(device)
    x, w, gy, mean, invstd, gamma, beta = (G.inp(inp[k]) for k in ("x", "w", "gy", "mean", "invstd", "gamma", "beta"))
    y, dx, dw = G.out(N, OHc, OWc, Cc), G.out(N, H, W, Cc), G.out(*inp["w"].shape)
    stats = G.out(lib.bn_stats_floats(Cc), fill=0.0)
    a = (N, H, W, C, OH, OW, K, stride, pt, pl)
    calls = {"dwconv2d_fwd": lambda st=None: lib.dwconv2d_fwd(x, w, y, *a, stats=st),
             "dwconv2d_fwd_bnswish": lambda st=None: lib.dwconv2d_fwd_bnswish(x, mean, invstd, gamma, beta, w, y, *a, stats=st),
             "dwconv2d_bwd_data": lambda: lib.dwconv2d_bwd_data(gy, w, dx, *a),
             "dwconv2d_bwd_weight": lambda: lib.dwconv2d_bwd_weight(x, gy, dw, *a),
             "dwconv2d_bwd_weight_bnswish": lambda: lib.dwconv2d_bwd_weight_bnswish(x, mean, invstd, gamma, beta, gy, dw, *a)}
    if not accepted:
        for e, call in calls.items():
            _refuses(e, call, G, f"{tag}: {e}")
        assert float(stats.abs().max()) == 0.0
        return False
    for pre, fwd, wgrad in ((False, "dwconv2d_fwd", "dwconv2d_bwd_weight"), (True, "dwconv2d_fwd_bnswish", "dwconv2d_bwd_weight_bnswish")):
        ref = dw_contract_ref(inp, geom, pre)
        close = lambda entry, name, got: _close_ref(entry, ref, name, got, tag)
        y.fill_(_CANARY[torch.float32])
        calls[fwd]()                                                        # statistics NULL
        close(fwd, "y", y)
        y0 = y.clone()
        for rep in range(2):                                                # statistics given: the same y bits, sums added to zeroed slots
            y.fill_(_CANARY[torch.float32])
            calls[fwd](stats)
            _layer_equal(fwd, y, y0, f"{tag}: {fwd} with and without statistics")
            sl = bn_slots(stats, C).sum(0).cpu()
            close(fwd, "sum", sl[0]); close(fwd, "sumsq", sl[1])
            stats.zero_()
        for rep in range(2):
            dw.fill_(0.25)                                                  # accumulates
            calls[wgrad]()
            _close_ref(wgrad, ref, "dw", dw.cpu().double() - 0.25, tag, 0.25)
        if not pre:
            for rep in range(2):
                dx.fill_(_CANARY[torch.float32])                            # overwritten
                calls["dwconv2d_bwd_data"]()
                close("dwconv2d_bwd_data", "dx", dx)
            dx0 = dx.clone()
            calls["dwconv2d_bwd_data"]()
            _layer_equal("dwconv2d_bwd_data", dx, dx0, f"{tag}: dwconv2d_bwd_data twice")
    G.intact(tag)
    return True


# ---- squeeze-excite --------------------------------------------------------------------------------------------------------------
def se_contract_expect(B, HW, C, SQ):
    """include/hifihr.h: the three plain entries take any C % 4 == 0; the fused MLP pair C <= 4096 and SQ <= 256."""
    plain = B > 0 and HW > 0 and C >= 4 and C % 4 == 0
    mlp = B > 0 and C >= 4 and C % 4 == 0 and C <= 4096 and 1 <= SQ <= 256
    return {"se_pool": plain, "se_scale": plain, "se_bwd_gate": plain, "se_mlp_fwd": mlp, "se_mlp_bwd": mlp}


def se_contract_inputs(B, HW, C, SQ, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    Cc = max(4, (C + 3) // 4 * 4)
    return dict(x=rnd(B, HW, Cc), gy=rnd(B, HW, Cc), gate=torch.sigmoid(rnd(B, Cc)), add=rnd(B, Cc), mean=rnd(B, Cc) * 0.5,
                w1=rnd(SQ, Cc) / Cc ** 0.5, b1=rnd(SQ) * 0.1, w2=rnd(Cc, SQ) / SQ ** 0.5, b2=rnd(Cc) * 0.1, dgate=rnd(B, Cc))


def se_plain_ref(inp, dt=torch.float64, drop_pixel=None):
    x, gy, gate, add = (inp[k].to(dt) for k in ("x", "gy", "gate", "add"))
    HW = x.shape[1]
    keep = slice(None) if drop_pixel is None else [i for i in range(HW) if i != drop_pixel]
    return {"pool": ("se_pool", HW, x[:, keep].sum(1) / HW), "bwd_gate": ("se_pool", HW, (gy * x)[:, keep].sum(1)),
            "scale": ("se_y", 1, x * gate.unsqueeze(1)), "scale_add": ("se_y", 1, gy * gate.unsqueeze(1) + add.unsqueeze(1) / HW)}


def se_mlp_fwd_ref(inp, dt=torch.float64):
    mean, w1, b1, w2, b2 = (inp[k].to(dt) for k in ("mean", "w1", "b1", "w2", "b2"))
    C, SQ = w1.shape[1], w1.shape[0]
    z1 = mean @ w1.t() + b1
    h1 = z1 * torch.sigmoid(z1)
    gate = torch.sigmoid(h1 @ w2.t() + b2)
    return {"mean": ("se_mlp", 1, mean), "z1": ("se_mlp", C, z1), "h1": ("se_mlp", C, h1), "gate": ("se_mlp", SQ, gate)}


def se_mlp_bwd_ref(inp, gate, z1, h1, mean, dt=torch.float64, drop_sample=None):
    """The MLP backward from the forward's saved tensors (gate, z1, h1, mean as the kernel wrote them)."""
    dgate, w1, w2 = (inp[k].to(dt) for k in ("dgate", "w1", "w2"))
    gate, z1, h1, mean = (t.detach().cpu().to(dt) for t in (gate, z1, h1, mean))
    B, C, SQ = dgate.shape[0], w1.shape[1], w1.shape[0]
    dz2 = dgate * gate * (1 - gate)
    s = torch.sigmoid(z1)
    dz1 = (dz2 @ w2) * (s + z1 * s * (1 - s))
    keep = slice(None) if drop_sample is None else [i for i in range(B) if i != drop_sample]
    return {"dz2": ("se_grad", 1, dz2), "dz1": ("se_grad", C, dz1), "dmean": ("se_grad", SQ, dz1 @ w1),
            "dw1": ("se_grad", B, dz1[keep].t() @ mean[keep]), "db1": ("se_grad", B, dz1[keep].sum(0)),
            "dw2": ("se_grad", B, dz2[keep].t() @ h1[keep]), "db2": ("se_grad", B, dz2[keep].sum(0))}


def se_contract_case(lib, device, B, HW, C, SQ, seed=0):
    """se_pool / se_scale / se_bwd_gate and the fused MLP pair on one geometry.  Returns {entry: accepted}."""
    expect = se_contract_expect(B, HW, C, SQ)
    assert lib.se_mlp_supported(C, SQ) == (C >= 4 and C % 4 == 0 and C <= 4096 and 1 <= SQ <= 256), f"se_mlp_supported({C}, {SQ})"
    inp = se_contract_inputs(B, HW, C, max(SQ, 1), seed)
    Cc, SQc = inp["x"].shape[2], inp["w1"].shape[0]
    tag = f"se B={B} HW={HW} C={C} SQ={SQ}"
    G = Guards(device)
    x, gy, gate, add = (G.inp(inp[k]) for k in ("x", "gy", "gate", "add"))
    acc, yo = G.out(B, Cc, fill=0.0), G.out(B, HW, Cc)
    if not expect["se_pool"]:
        _refuses("se_pool", lambda: lib.se_pool(x, B, HW, C, acc), G, tag)
        _refuses("se_bwd_gate", lambda: lib.se_bwd_gate(gy, x, B, HW, C, acc), G, tag)
        _refuses("se_scale", lambda: lib.se_scale(x, gate, None, 0.0, B, HW, C, yo), G, tag)
    else:
        ref = se_plain_ref(inp)
        close = lambda entry, name, got: _close_ref(entry, ref, name, got, tag)
        for rep in range(2):
            acc.zero_(); lib.se_pool(x, B, HW, C, acc); close("se_pool", "pool", acc)
            acc.zero_(); lib.se_bwd_gate(gy, x, B, HW, C, acc); close("se_bwd_gate", "bwd_gate", acc)
        yo2 = G.out(B, HW, Cc)
        lib.se_scale(x, gate, None, 0.0, B, HW, C, yo); close("se_scale", "scale", yo)
        lib.se_scale(x, gate, None, 0.0, B, HW, C, yo2); _layer_equal("se_scale", yo2, yo, f"{tag}: se_scale twice")
        lib.se_scale(gy, gate, add, 1.0 / HW, B, HW, C, yo); close("se_scale", "scale_add", yo)
    # the fused MLP pair, on means given directly (its own bound, independent of the pooling error)
    w1, b1, w2t, b2, dgate = G.inp(inp["w1"]), G.inp(inp["b1"]), G.inp(inp["w2"].t().contiguous()), G.inp(inp["b2"]), G.inp(inp["dgate"])
    macc = G.out(B, Cc, fill=0.0)
    mean, z1, h1, g2 = G.out(B, Cc), G.out(B, SQc), G.out(B, SQc), G.out(B, Cc)
    dacc = G.out(B, Cc, fill=0.0)
    dz2, dz1, dmean = G.out(B, Cc), G.out(B, SQc), G.out(B, Cc)
    fw1, fb1, fw2, fb2 = G.out(SQc, Cc), G.out(SQc), G.out(Cc, SQc), G.out(Cc)
    if not expect["se_mlp_fwd"]:
        _refuses("se_mlp_fwd", lambda: lib.se_mlp_fwd(macc, w1, b1, w2t, b2, B, C, SQ, mean, z1, h1, g2), G, tag)
        _refuses("se_mlp_bwd", lambda: lib.se_mlp_bwd(dacc, gate, z1, h1, gate, w1, w2t, B, C, SQ, dz2, dz1, dmean, fw1, fb1, fw2, fb2), G, tag)
        assert float(macc.abs().max()) == 0.0 and float(dacc.abs().max()) == 0.0
        G.intact(tag)
        return expect
    ref = se_mlp_fwd_ref(inp)
    first = None
    for rep in range(2):
        macc.copy_(inp["mean"])
        lib.se_mlp_fwd(macc, w1, b1, w2t, b2, B, C, SQ, mean, z1, h1, g2)
        assert float(macc.abs().max()) == 0.0, f"{tag}: se_mlp_fwd hands the accumulator back zeroed"
        for name, got in (("mean", mean), ("z1", z1), ("h1", h1), ("gate", g2)):
            _close_ref("se_mlp_fwd", ref, name, got, tag)
        now = torch.cat([t.reshape(-1) for t in (mean, z1, h1, g2)]).clone()
        if first is not None:
            _layer_equal("se_mlp_fwd", now, first, f"{tag}: se_mlp_fwd twice")
        first = now
    refb = se_mlp_bwd_ref(inp, g2, z1, h1, mean)
    first = None
    for rep in range(2):
        dacc.copy_(inp["dgate"])
        for t in (fw1, fb1, fw2, fb2):
            t.fill_(0.25)                                                   # += semantics
        lib.se_mlp_bwd(dacc, g2, z1, h1, mean, w1, w2t, B, C, SQ, dz2, dz1, dmean, fw1, fb1, fw2, fb2)
        assert float(dacc.abs().max()) == 0.0, f"{tag}: se_mlp_bwd hands the accumulator back zeroed"
        for name, got in (("dz2", dz2), ("dz1", dz1), ("dmean", dmean), ("dw1", fw1.cpu().double() - 0.25), ("db1", fb1.cpu().double() - 0.25),
                          ("dw2", fw2.cpu().double() - 0.25), ("db2", fb2.cpu().double() - 0.25)):
            _close_ref("se_mlp_bwd", refb, name, got, tag, 0.25 if name[1] in "wb" else 0.0)
        now = torch.cat([t.reshape(-1) for t in (dz2, dz1, dmean, fw1, fw2, fb2)]).clone()          # (db1 goes through float atomics)
        if first is not None:
            _layer_equal("se_mlp_bwd", now, first, f"{tag}: se_mlp_bwd twice (every element summed by one thread in a fixed order)")
        first = now
    G.intact(tag)
    return expect


def drop_connect_contract_case(lib, device, B, per_sample, keep, with_skip, seed=0):
    """out = x / keep * floor(keep + u[b]) (+ skip); u chosen so that both branches of the floor occur when B > 1."""
    accepted = B > 0 and per_sample > 0 and per_sample % 4 == 0 and keep > 0
    gen = torch.Generator().manual_seed(seed)
    n = max(4, (per_sample + 3) // 4 * 4)
    x_t, skip_t = torch.randn(B, n, generator=gen), torch.randn(B, n, generator=gen)
    u_t = torch.rand(B, generator=gen)
    u_t[0] = 0.999                                              # kept for every keep > 0.001
    if B > 1:
        u_t[1] = 0.0                                            # dropped whenever keep < 1
    tag = f"drop_connect B={B} per_sample={per_sample} keep={keep} skip={with_skip}"
    G = Guards(device)
    x, skip, u, out = G.inp(x_t), (G.inp(skip_t) if with_skip else None), G.inp(u_t), G.out(B, n)
    call = lambda: lib.drop_connect_add(x, skip, u, keep, B, per_sample, out)
    if not accepted:
        _refuses("drop_connect_add", call, G, tag)
        return False
    m = torch.floor(torch.tensor(keep, dtype=torch.float32) + u_t).double()         # the mask is decided in fp32, as the entry documents
    if B > 1 and keep < 1:
        assert set(m.tolist()) == {0.0, 1.0}
    ref = x_t.double() / float(torch.tensor(keep, dtype=torch.float32)) * m.unsqueeze(1) + (skip_t.double() if with_skip else 0)
    call()
    _layer_close("drop_connect_add", "se_y", out, ref, 1, tag)
    out2 = G.out(B, n)
    lib.drop_connect_add(x, skip, u, keep, B, per_sample, out2)
    _layer_equal("drop_connect_add", out2, out, tag + " twice")
    G.intact(tag)
    return True


# ---- SSIM ------------------------------------------------------------------------------------------------------------------------
SSIM_TILE = 32


def ssim_contract_inputs(planes, H, W, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(1, planes, H, W, generator=gen)
    if kind == "random":
        b = (a + 0.3 * torch.rand(1, planes, H, W, generator=gen)).clamp(0, 1)
    elif kind == "identical":
        b = a.clone()
    elif kind == "constants":
        a, b = torch.full_like(a, 0.25), torch.full_like(a, 0.75)
    elif kind == "masked":                                      # a render-like pair: the image times a mask against the image
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        mask = (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) <= (0.35 * max(H, W, 2)) ** 2).float()
        b, a = a.clone(), a * mask
    else:
        raise ValueError(kind)
    return a, b


def _ssim_window_tensor(dt):
    import math
    g = torch.Tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    return (g / g.sum()).to(dt)                                 # the fp32 taps the kernels are handed, exact in float64


def ssim_contract_ref(a, b, grad_out, dt=torch.float64, drop_tile=False):
    """pytorch_ssim.ssim written out in `dt` with the three derivative maps the kernels save (d s / d mu1 in total, d s / d E[x^2],
    d s / d E[xy]), the per-tile partial sums and the gradient d(grad_out * mean SSIM) / d img1 by autograd."""
    import torch.nn.functional as F
    a, b = a.to(dt), b.to(dt)
    _, P, H, W = a.shape
    g = _ssim_window_tensor(dt)
    w = (g.unsqueeze(1) @ g.unsqueeze(0)).view(1, 1, 11, 11).expand(P, 1, 11, 11).contiguous()
    ar = a.clone().requires_grad_(True)
    conv = lambda t: F.conv2d(t, w, padding=5, groups=P)
    mu1, mu2 = conv(ar), conv(b)
    e11, e22, e12 = conv(ar * ar), conv(b * b), conv(ar * b)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    a1, a2 = 2 * mu1 * mu2 + C1, 2 * (e12 - mu1 * mu2) + C2
    b1, b2 = mu1 * mu1 + mu2 * mu2 + C1, (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    s = a1 * a2 / (b1 * b2)
    val = s.mean()
    (val * grad_out).backward()
    sd, m1, m2 = s.detach(), mu1.detach(), mu2.detach()
    a1, a2, b1, b2 = a1.detach(), a2.detach(), b1.detach(), b2.detach()
    dA = 2 * m2 * (a2 - a1) / (b1 * b2) - 2 * m1 * sd / b1 + 2 * m1 * sd / b2
    dB = -sd / b2
    dC = 2 * a1 / (b1 * b2)
    th, tw = -(-H // SSIM_TILE), -(-W // SSIM_TILE)
    sp = F.pad(sd[0], (0, tw * SSIM_TILE - W, 0, th * SSIM_TILE - H))
    part = sp.view(P, th, SSIM_TILE, tw, SSIM_TILE).sum((2, 4)).reshape(-1)
    total = part.sum() if not drop_tile else part[1:].sum()
    n = P * H * W
    # first-order size of the rounding of s = a1 a2 / (b1 b2) per pixel, in units of eps: a2 and b2 are differences of window moments
    e11d, e22d, e12d = e11.detach(), e22.detach(), e12.detach()
    cs = a1.abs() * 2 * (e12d.abs() + (m1 * m2).abs()) / (b1 * b2) + sd.abs() * (e11d + m1 * m1 + e22d + m2 * m2) / b2
    cpart = F.pad(cs[0], (0, tw * SSIM_TILE - W, 0, th * SSIM_TILE - H)).view(P, th, SSIM_TILE, tw, SSIM_TILE).sum((2, 4))
    return {"value": ("ssim_val", n, (total / n).reshape(1), float(cs.mean())), "partial": ("ssim_part", SSIM_TILE * SSIM_TILE, part, float(cpart.max())), "dA": ("ssim_map", 121, dA[0]),
            "dB": ("ssim_map", 121, dB[0]), "dC": ("ssim_map", 121, dC[0]), "grad": ("ssim_grad", 121, ar.grad[0])}


def ssim_contract_case(lib, device, planes, H, W, kind="random", seed=0, misaligned=True):
    """ssim_fwd / ssim_bwd / ssim_bwd_scaled / ssim_finish / ssim_partial_count on one image size.  On W % 4 == 0 the whole call is repeated
    with every plane shifted by one float (the scalar staging form): value, partials, maps and gradient must be the aligned call's bits."""
    from hifihr_amd.ops import _ssim_window
    win = _ssim_window()
    a_t, b_t = ssim_contract_inputs(planes, H, W, kind, seed)
    gout, lam = 2.0, 0.37
    tag = f"ssim {planes}x{H}x{W} {kind}"
    count = lib.ssim_partial_count(planes, H, W)
    assert count == planes * (-(-H // SSIM_TILE)) * (-(-W // SSIM_TILE)), f"{tag}: ssim_partial_count"
    assert lib.ssim_partial_count(0, H, W) == 0 and lib.ssim_partial_count(planes, 0, W) == 0
    ref = ssim_contract_ref(a_t, b_t, gout)
    close = lambda entry, name, got: _close_ref(entry, ref, name, got, tag)
    G = Guards(device)
    n = planes * H * W
    results = []
    for off in ((0, 1) if (misaligned and W % 4 == 0) else (0,)):
        a, b = G.inp(a_t, offset_floats=off), G.inp(b_t, offset_floats=off)
        part = G.out(count)
        maps = [G.out(1, planes, H, W, offset_floats=off) for _ in range(3)]
        g1, g2, out = G.out(1, planes, H, W), G.out(1, planes, H, W), G.out(1)
        go = G.inp(torch.full((1,), gout))
        for rep in range(2):
            part.fill_(_CANARY[torch.float32])
            lib.ssim_fwd(win, a, b, part, maps[0], maps[1], maps[2])
            close("ssim_fwd", "partial", part)
            close("ssim_fwd", "value", part.cpu().double().sum().reshape(1) / n)
            for name, m in zip(("dA", "dB", "dC"), maps):
                close("ssim_fwd", name, m)
            g1.fill_(_CANARY[torch.float32])
            lib.ssim_bwd(win, a, b, maps[0], maps[1], maps[2], go, g1)
            close("ssim_bwd", "grad", g1)
            lib.ssim_bwd_scaled(win, a, b, maps[0], maps[1], maps[2], go, -lam, g2)
            _layer_close("ssim_bwd_scaled", "ssim_grad", g2, -lam * ref["grad"][2], 121, f"{tag}: ssim_bwd_scaled")
            lib.ssim_finish(part, 1.0 / n, 0.0, out)
            close("ssim_finish", "value", out)
            now = torch.cat([t.reshape(-1).clone() for t in (part, maps[0], maps[1], maps[2], g1, g2, out)])
            results.append(now)
        part2 = G.out(count)
        lib.ssim_fwd(win, a, b, part2, None, None, None)                   # without the derivative maps
        _layer_equal("ssim_fwd", part2, part, f"{tag}: partials without the maps")
        _refuses("ssim_fwd", lambda: lib.ssim_fwd(win, a, b, part2, maps[0], None, maps[2]), G, tag + " two of three maps")
    for r in results[1:]:
        _layer_equal("ssim_fwd", r, results[0], f"{tag}: a second call / the planes shifted by one float (scalar staging) give the same bits")
    G.intact(tag)
    return True


def ssim_finish_contract_case(lib, device, count, seed=0):
    """out = offset + scale * sum(partial[0 .. count)) against a float64 sum (L = count)."""
    gen = torch.Generator().manual_seed(seed)
    p_t = torch.rand(count, generator=gen) * 1024              # partials of a 32 x 32 tile lie in [0, 1024]
    G = Guards(device)
    p, out = G.inp(p_t), G.out(1)
    for scale, offset in ((1.0 / (1024.0 * count), 0.0), (-0.37 / (1024.0 * count), 0.37)):
        ref = float(torch.tensor(offset, dtype=torch.float32)) + float(torch.tensor(scale, dtype=torch.float32)) * p_t.double().sum()
        lib.ssim_finish(p, scale, offset, out)
        sref = (float(torch.tensor(scale, dtype=torch.float32)) * p_t.double().sum()).reshape(1)
        # the bound is on the scaled sum (the offset lambda cancels most of it in the loss term)
        err, bound = layer_err(out, ref.reshape(1)), layer_bound("ssim_val", sref, count) + 6e-8 * max(abs(offset), float(ref.abs()))
        _layer_log("ssim_finish", True, err / bound)
        assert err <= bound, f"ssim_finish count={count}: err {err:.3e} vs bound {bound:.3e}"
    _refuses("ssim_finish", lambda: lib.ssim_finish(p[:0], 1.0, 0.0, out), G, "ssim_finish count 0")
    G.intact(f"ssim_finish {count}")
    return True


# ------------------------------------------------------------------------------------------------
# The GEMM contract: the batched products of csrc/gemm.hip and hifihr_weight_transpose on fixed shape lists
# (tests/test_hostsim_gemm_contract.py; the GPU half in tests/test_gpu_gemm.py), in the layer contract's form: an entry refuses
# (HIFIHR_EINVAL, outputs untouched) or matches torch.matmul in float64 inside NaN / canary guard bands, twice on the same workspace with
# identical bits.  Two input families: randn (bound c sqrt(L) max|ref|, kinds gemm_nt / gemm_tn below) and small integers, whose products
# and partial sums are all exact in fp32 -- the result then equals the float64 reference BIT FOR BIT whatever the summation order, so a
# dropped, repeated or permuted k-step or a share boundary off by one fails at any tolerance.
# ------------------------------------------------------------------------------------------------
GEMM_CONTRACT_ENTRIES = ("bgemm", "weight_transpose", "weight_prep", "linear", "wino", "_wino", "_weight_prep")      # prefixes of the entries this contract logs (LAYER_CONTRACT_LOG)
GEMM_CONTRACT_KINDS = ("gemm_nt", "gemm_tn", "lin_y", "lin_stat", "lin_bn_y", "lin_dw", "lin_dx")
LAYER_CONTRACT_C.update({
    # kind: (c, cap)                  fp32 torch's worst ratio (tools/layer_contract_c.py) x 4; the quantities and L; (where cap comes from)
    "gemm_nt": (2.2e-7, 2e-6),        # 5.41e-08 x 4   hifihr_bgemm_nt c, L = K       (bgemm_case: 2e-6 sqrt(K); c <= 2e-6 keeps c sqrt(L) below it at every K >= 1)
    "gemm_tn": (1.9e-7, 2e-6),        # 4.70e-08 x 4   hifihr_bgemm_tn slabs (L = rows of the slab) and their sum (L = T)   (bgemm_tn_case: 2e-6 sqrt(T))
    #                                  (the emulator's worst err / bound is 0.59, above one half, on the 259-row slabs of 256 x 256 x 777: the kernel adds its
    #                                  k-steps to ONE accumulator in t order, whose rounding grows with the running sum, where fp32 torch -- the
    #                                  measure of c -- sums in blocks; the next shapes sit at 0.35 and below)
})
GEMM_INT_A, GEMM_INT_B = 30, 26        # |a| <= 30, |b| <= 26 in the integer family: 780 L < 2^24 for every L <= 21 509


def gemm_operands(fill, batch, rows_a, rows_b, L, seed, transposed):
    """a[batch][rows_a][L], b[batch][rows_b][L] (transposed: [batch][L][rows]) -- randn, or integers that differ from row to row and from
    k to k with different periods in a and b (61 and 53: the pair (a, b) at one k repeats after 3233 steps only)."""
    if fill == "randn":
        gen = torch.Generator().manual_seed(seed)
        a, b = torch.randn(batch, rows_a, L, generator=gen), torch.randn(batch, rows_b, L, generator=gen)
    else:
        p = torch.arange(batch).view(-1, 1, 1)
        k = torch.arange(L).view(1, 1, -1)
        ra, rb = torch.arange(rows_a).view(1, -1, 1), torch.arange(rows_b).view(1, -1, 1)
        a = ((ra * 7 + k * 13 + p * 3 + seed) % (2 * GEMM_INT_A + 1) - GEMM_INT_A).float()
        b = ((rb * 11 + k * 17 + p * 5 + seed) % (2 * GEMM_INT_B + 1) - GEMM_INT_B).float()
    if transposed:
        a, b = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()
    return a, b


def gemm_ints_exact(L):
    """every partial sum of the integer family is an integer below 2^24: exact in fp32"""
    return GEMM_INT_A * GEMM_INT_B * L < 2 ** 24


def bgemm_nt_expect(M, N, K, batch):
    """include/hifihr.h: K % 32 == 0, N % 64 == 0, any M > 0, batch > 0, operands below 2^31 elements per problem."""
    return M > 0 and batch > 0 and K >= 32 and K % 32 == 0 and N >= 64 and N % 64 == 0 and M * K < 2 ** 31 and N * K < 2 ** 31


def bgemm_tn_expect(M, N, T, batch):
    return T > 0 and batch > 0 and M >= 64 and M % 64 == 0 and N >= 64 and N % 64 == 0


def bgemm_tn_slab_rows(T, parts, z):
    """include/hifihr.h: slab z of `parts` holds rows 32 cps z <= t < min(T, 32 cps (z + 1)), cps = ceil(ceil(T / 32) / parts)."""
    cps = -(-(-(-T // 32)) // parts)
    return 32 * cps * z, min(T, 32 * cps * (z + 1))


def bgemm_nt_contract_case(lib, device, M, N, K, batch, ws_mode="full", seed=0, fills=("randn", "ints"), drop=None):
    """hifihr_bgemm_nt / _workspace_bytes / _describe_batch on one shape.  ws_mode: "full" (what the query asks for), "short" (one float
    less: the per-tile fallback, workspace untouched), "none".  -> (accepted, workspace bytes the shape asks for)."""
    what = f"bgemm_nt {M}x{N}x{K}x{batch} ({ws_mode})"
    if not bgemm_nt_expect(M, N, K, batch):
        G = Guards(device)
        small = M * K < 2 ** 31 and N * K < 2 ** 31          # (beyond 32-bit offsets: the predicate path alone, nothing large is allocated)
        a = G.inp(torch.zeros(max(batch, 1), max(M, 1) if small else 1, max(K, 1)))
        b = G.inp(torch.zeros(max(batch, 1), max(N, 1) if small else 1, max(K, 1)))
        c = G.out(max(batch, 1), max(M, 1) if small else 1, max(N, 1))
        _refuses("bgemm_nt", lambda: lib.bgemm_nt(a, b, c, M, N, K, batch), G, what)
        if small:
            assert lib.bgemm_nt_workspace_bytes(M, N, K, batch) == 0, f"{what}: a workspace for a refused shape"
            assert batch <= 0 or lib.bgemm_describe(False, M, N, K, batch) == "", f"{what}: a kernel name for a refused shape"
        return False, 0
    nb = lib.bgemm_nt_workspace_bytes(M, N, K, batch)
    assert nb % 4 == 0
    assert lib.bgemm_describe(False, M, N, K, batch) != ""
    G = Guards(device)
    c = G.out(batch, M, N)
    nws = {"full": nb // 4, "short": nb // 4 - 1, "none": 0}[ws_mode]
    ws = G.out(nws, fill=0.0) if nws > 0 else None                       # ONE workspace for every run of the case
    for fill in fills:
        a, b = gemm_operands(fill, batch, M, N, K, seed, False)
        ref = torch.matmul(a.double(), b.double().transpose(1, 2))
        ad, bd = G.inp(a), G.inp(b)
        first = None
        for rep in range(2 if fill == fills[0] else 1):                   # the first family twice: identical bits
            c.fill_(_CANARY[torch.float32])
            lib.bgemm_nt(ad, bd, c, M, N, K, batch, ws=ws)
            tag = f"{what} {fill} rep {rep}"
            G.intact(tag)
            assert ws is None or float(ws.abs().max()) == 0.0, f"{tag}: workspace not handed back all zero"
            if fill == "ints":
                assert gemm_ints_exact(K)
                _layer_equal("bgemm_nt", c, ref.float(), tag)
            else:
                _layer_close("bgemm_nt", "gemm_nt", c, ref, K, tag)
            assert first is None or torch.equal(first, c), f"{what} {fill}: two runs differ"
            first = c.clone()
    c.fill_(_CANARY[torch.float32])
    for args in ((None, bd, c), (ad, None, c), (ad, bd, None)):
        _refuses("bgemm_nt", lambda: lib.bgemm_nt(*args, M, N, K, batch), G, f"{what}: null pointer")
    return True, nb


def bgemm_tn_contract_case(lib, device, M, N, T, batch, seed=0, fills=("randn", "ints")):
    """hifihr_bgemm_tn / _tn_parts / _describe_batch on one shape: every slab against the rows the header gives it, and the slabs' sum.
    -> slab count (0: refused)."""
    what = f"bgemm_tn {M}x{N}x{T}x{batch}"
    parts = lib.bgemm_tn_parts(M, N, T, batch)
    if not bgemm_tn_expect(M, N, T, batch):
        assert parts == 0, f"{what}: slabs for a refused shape"
        G = Guards(device)
        a = G.inp(torch.zeros(max(batch, 1), max(T, 1), max(M, 1)))
        b = G.inp(torch.zeros(max(batch, 1), max(T, 1), max(N, 1)))
        c = G.out(2, max(batch, 1), max(M, 1), max(N, 1))
        for p in (1, 2):
            _refuses("bgemm_tn", lambda: lib.bgemm_tn(a, b, c, M, N, T, batch, p), G, what)
        assert batch <= 0 or lib.bgemm_describe(True, M, N, T, batch) == "", f"{what}: a kernel name for a refused shape"
        return 0
    assert parts >= 1 and lib.bgemm_describe(True, M, N, T, batch) != ""
    rows = [bgemm_tn_slab_rows(T, parts, z) for z in range(parts)]
    assert all(lo < hi for lo, hi in rows) and rows[-1][1] == T, f"{what}: {parts} slabs leave one empty or rows uncovered ({rows})"
    G = Guards(device)
    cp = G.out(parts + 1, batch, M, N)                                           # (one slab more than asked for: room for the refused calls below)
    for fill in fills:
        a, b = gemm_operands(fill, batch, M, N, T, seed, True)                   # a[batch][T][M], b[batch][T][N]
        a64, b64 = a.double(), b.double()
        ad, bd = G.inp(a), G.inp(b)
        first = None
        for rep in range(2 if fill == fills[0] else 1):                           # the first family twice: identical bits
            cp.fill_(_CANARY[torch.float32])
            lib.bgemm_tn(ad, bd, cp, M, N, T, batch, parts)
            tag = f"{what} {fill} ({parts} slabs) rep {rep}"
            G.intact(tag)
            assert _is_canary(cp[parts]), f"{tag}: wrote behind the last slab"
            assert first is None or torch.equal(first, cp), f"{what} {fill}: two runs differ"
            first = cp.clone()
        for z, (lo, hi) in enumerate(rows):
            ref = torch.matmul(a64[:, lo:hi].transpose(1, 2), b64[:, lo:hi])
            if fill == "ints":
                assert gemm_ints_exact(T)
                _layer_equal("bgemm_tn", cp[z], ref.float(), f"{tag} slab {z} (rows {lo}..{hi})")
            else:
                _layer_close("bgemm_tn", "gemm_tn", cp[z], ref, hi - lo, f"{tag} slab {z} (rows {lo}..{hi})")
        if fill == "randn":
            full = torch.matmul(a64.transpose(1, 2), b64)
            _layer_close("bgemm_tn", "gemm_tn", cp[:parts].double().sum(0), full, T, f"{tag} sum of the slabs")
    cp.fill_(_CANARY[torch.float32])
    for p in (parts + 1, 0, -1):
        _refuses("bgemm_tn", lambda: lib.bgemm_tn(ad, bd, cp, M, N, T, batch, p), G, f"{what}: parts = {p}, the plan's {parts}")
    for args in ((None, bd, cp), (ad, None, cp), (ad, bd, None)):
        _refuses("bgemm_tn", lambda: lib.bgemm_tn(*args, M, N, T, batch, parts), G, f"{what}: null pointer")
    return parts


def weight_transpose_contract_case(lib, device, K, RS, C, seed=0):
    """hifihr_weight_transpose: [K][RS][C] -> [C][RS][K], a copy (bit for bit), any positive sizes."""
    what = f"weight_transpose {K}x{RS}x{C}"
    G = Guards(device)
    if not (K > 0 and RS > 0 and C > 0):
        w, wt = G.inp(torch.zeros(max(K, 1), max(RS, 1), max(C, 1))), G.out(max(C, 1), max(RS, 1), max(K, 1))
        _refuses("weight_transpose", lambda: lib.weight_transpose(w, wt, K, RS, C), G, what)
        return False
    w = torch.randn(K, RS, C, generator=torch.Generator().manual_seed(seed))
    wd, wt = G.inp(w), G.out(C, RS, K)
    for rep in range(2):
        wt.fill_(_CANARY[torch.float32])
        lib.weight_transpose(wd, wt, K, RS, C)
        G.intact(what)
        _layer_equal("weight_transpose", wt, w.permute(2, 1, 0).contiguous(), what)
    for args in ((None, wt), (wd, None)):
        _refuses("weight_transpose", lambda: lib.weight_transpose(*args, K, RS, C), G, f"{what}: null pointer")
    return True


# ---- fully connected (csrc/mlp.hip) ------------------------------------------------------------------------------------------------
# Reference: nn.Linear, BatchNorm1d (training mode) and the activation under float64 autograd.  Quantities -> (kind, L, tensor[, cond]):
#   lin_y   y / z without batch-norm, L = I;      lin_stat  save_mean / save_invstd / running statistics;      lin_bn_y  y behind batch-norm
#   lin_dw  dW / db (L = B), dgamma / dbeta (L = B);      lin_dx  dx, L = O
# Batch-norm puts  amp = max |gamma| invstd  in front of the rounding of z (c sqrt(I) max|z|) and of the cancellation g - mean g -
# xhat mean(g xhat) of its backward: those sizes are the `cond` of the quantities behind it (layer_bound), and tools/layer_contract_c.py
# measures fp32 torch against the same expression.
LAYER_CONTRACT_C.update({
    "lin_y": (2.9e-7, 3e-5),          # 7.06e-08 x 4   (linear_case: 3e-5 max(1, max|y|))
    "lin_stat": (2.0e-7, 1e-5),       # 4.82e-08 x 4   (linear_case: running_mean rtol 1e-5)
    "lin_bn_y": (7.1e-8, 3e-5),       # 1.77e-08 x 4   (linear_case: 3e-5)
    "lin_dw": (7.3e-7, 2e-4),         # 1.82e-07 x 4   (linear_case: 2e-4)
    "lin_dx": (4.1e-7, 2e-4),         # 1.01e-07 x 4   (linear_case: 2e-4)
})
LINEAR_MAX_GROUP, LINEAR_BN_MAX_B = 6, 64


def linear_contract_expect(B, I, O, act, bn):
    """include/hifihr.h: any B, I, O > 0, act 0..3; batch-norm at B <= 64 and act 0 / 1 only."""
    return B > 0 and I > 0 and O > 0 and 0 <= act <= 3 and not (bn and (B > LINEAR_BN_MAX_B or act >= 2))


def linear_contract_inputs(B, I, O, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    return {"x": rnd(B, I), "w": rnd(O, I) / I ** 0.5, "b": rnd(O) * 0.1, "gamma": 1 + 0.2 * rnd(O), "beta": 0.1 * rnd(O), "rm0": 0.1 * rnd(O),
            "rv0": 1 + 0.1 * torch.rand(O, generator=gen), "gy": rnd(B, O)}


def linear_contract_ref(inp, act, bn, eps=1e-5, mom=0.1, dt=torch.float64, mask=None, drop_row=None, drop_k=None, drop_o=None):
    """Float64 (or dt) autograd of act(BatchNorm1d?(x W^T + b)).  mask: the ReLU decisions to use instead of the reference's own (the
    kernel's, where z is zero to rounding).  drop_row / drop_k: the detection check's reference without one batch row of the reductions
    over B / one input feature of the reductions over I / one output feature of the reduction over O (dx)."""
    import torch.nn.functional as Fn
    t = {k: v.to(dt) for k, v in inp.items()}
    x, w, gy = t["x"], t["w"], t["gy"]
    if drop_k is not None:
        x = x.clone(); x[:, drop_k] = 0
    if drop_row is not None:
        gy = gy.clone(); gy[drop_row] = 0
    if drop_o is not None:
        gy = gy.clone(); gy[:, drop_o] = 0
    xr, wr, br, gr, ber = (v.clone().requires_grad_(True) for v in (x, w, t["b"], t["gamma"], t["beta"]))
    z = Fn.linear(xr, wr, br)
    B, I = x.shape
    O = w.shape[0]
    out = {"z": ("lin_y", I, z.detach())}
    pre, amp = z, 0.0
    zmax = float(z.detach().abs().max())
    if bn:
        rm, rv = t["rm0"].clone(), t["rv0"].clone()
        mu, var = z.mean(0), z.var(0, unbiased=False)
        invstd = (var + eps).rsqrt()
        pre = (z - mu) * invstd * gr + ber
        amp = float((gr.detach().abs() * invstd.detach()).max())
        ismax = float(invstd.detach().max())
        zerr = I ** 0.5 * zmax                                 # the size c multiplies for z itself
        unb = var * (B / (B - 1)) if B > 1 else var            # (B = 1: the biased value, as bn.hip's M = 1 rule)
        out.update({"save_mean": ("lin_stat", 1, mu.detach(), zerr), "save_invstd": ("lin_stat", 1, invstd.detach(), ismax ** 2 * zerr),
                    "running_mean": ("lin_stat", 1, ((1 - mom) * rm + mom * mu).detach(), mom * zerr),
                    "running_var": ("lin_stat", 1, ((1 - mom) * rv + mom * unb).detach(), mom * 2 * float(var.detach().max()) ** 0.5 * zerr)})
    if act == 1:
        m = (pre.detach() > 0) if mask is None else mask
        y = pre * m.to(dt)
    elif act == 2:
        y = pre * torch.sigmoid(pre)
    elif act == 3:
        y = torch.sigmoid(pre)
    else:
        y = pre
    out["y"] = ("lin_bn_y", I, y.detach(), amp * I ** 0.5 * zmax) if bn else ("lin_y", I, y.detach())
    y.backward(gy)
    gmax, xmax, wmax = float(gy.abs().max()), float(x.abs().max()), float(w.abs().max())
    A = amp * gmax * (B ** 0.5 if bn else 0.0)                 # batch-norm's backward: g - mean g - xhat mean(g xhat), sums over B, times gamma invstd
    if bn:                                                    # ... and the forward's rounding of z reaches it through xhat and the statistics
        A += amp * ismax * gmax * I ** 0.5 * zmax * B ** 0.5
    out.update({"dW": ("lin_dw", B, wr.grad, B ** 0.5 * A * xmax), "db": ("lin_dw", B, br.grad, B ** 0.5 * A),
                "dx": ("lin_dx", O, xr.grad, O ** 0.5 * A * wmax)})
    if bn:
        xh = float(((z - mu) * invstd).detach().abs().max())
        out.update({"dgamma": ("lin_dw", B, gr.grad, B ** 0.5 * gmax * (xh + ismax * I ** 0.5 * zmax)), "dbeta": ("lin_dw", B, ber.grad)})
    return out


def _lin_q(ref, name):
    q = ref[name]
    return q[0], q[1], q[2], (q[3] if len(q) > 3 else 0.0)


def linear_contract_case(lib, device, B, I, O, act, bn, running=True, need_dx=True, seed=0, eps=1e-5, mom=0.1):
    """hifihr_linear_fwd / _bwd on one shape: forward outputs, saved statistics, running statistics (both or neither), the ACCUMULATE
    semantics of dW / db / dgamma / dbeta on a non-zero prefill, dx overwritten or skipped; twice, identical bits.  -> accepted."""
    from hifihr_amd._lib import _fp, _stream_of
    what = f"linear {B}x{I}x{O} act {act} bn {bn}"
    G = Guards(device)
    ok = linear_contract_expect(B, I, O, act, bn)
    inp = linear_contract_inputs(max(B, 1), max(I, 1), max(O, 1), seed)
    Bq, Oq, Iq = max(B, 1), max(O, 1), max(I, 1)
    x, w, b, gy = (G.inp(inp[k]) for k in ("x", "w", "b", "gy"))
    gamma, beta = G.inp(inp["gamma"]), G.inp(inp["beta"])
    y, z, sm, si = G.out(Bq, Oq), G.out(Bq, Oq), G.out(Oq), G.out(Oq)
    rm, rv = G.out(Oq), G.out(Oq)
    rm.copy_(inp["rm0"]); rv.copy_(inp["rv0"])
    dz, dW, db, dg, dbt, dx = G.out(Bq, Oq), G.out(Oq, Iq, fill=0.5), G.out(Oq, fill=-0.25), G.out(Oq, fill=0.125), G.out(Oq, fill=2.0), G.out(Bq, Iq)

    def fwd(Bc=B, Ic=I, Oc=O, actc=act, with_bn=bn, rmc=rm, rvc=rv, zc=z, **over):
        a = dict(x=x, w=w, y=y)
        a.update(over)
        # (the binding takes its sizes from the tensors: the C entry itself, for explicit B, I, O)
        lib.check(lib.c.hifihr_linear_fwd(_fp(a["x"]), _fp(a["w"]), _fp(b), Bc, Ic, Oc, int(actc), _fp(gamma if with_bn else None), _fp(beta if with_bn else None),
                                          float(eps), float(mom), _fp(rmc if with_bn else None), _fp(rvc if with_bn else None), _fp(a["y"]),
                                          _fp(zc if (with_bn or actc == 2) else None), _fp(sm if with_bn else None), _fp(si if with_bn else None),
                                          _stream_of(x)), "hifihr_linear_fwd")

    def bwd(Bc=B, Ic=I, Oc=O, actc=act, with_bn=bn, dxc=dx, dzc=dz, **over):
        a = dict(dy=gy, x=x, w=w, y=y)
        a.update(over)
        lib.check(lib.c.hifihr_linear_bwd(_fp(a["dy"]), _fp(a["y"]), _fp(a["x"]), _fp(a["w"]), Bc, Ic, Oc, int(actc), _fp(gamma if with_bn else None),
                                          _fp(z if (with_bn or actc == 2) else None), _fp(sm if with_bn else None), _fp(si if with_bn else None),
                                          _fp(dzc), _fp(dW), _fp(db), _fp(dg if with_bn else None), _fp(dbt if with_bn else None), _fp(dxc),
                                          _stream_of(x)), "hifihr_linear_bwd")

    if not ok:
        _refuses("linear_fwd", fwd, G, what)
        _refuses("linear_bwd", bwd, G, what)
        return False
    rm_on = running and bn
    first = None
    for rep in range(2):
        for t_ in (y, z, sm, si, dz, dx):
            t_.fill_(_CANARY[torch.float32])
        rm.copy_(inp["rm0"]); rv.copy_(inp["rv0"])
        dW.fill_(0.5); db.fill_(-0.25); dg.fill_(0.125); dbt.fill_(2.0)
        fwd(rmc=rm if rm_on else None, rvc=rv if rm_on else None)
        tag = f"{what} rep {rep}"
        G.intact(tag)
        mask = None
        if act == 1:            # the kernel's ReLU decisions; they may differ from float64's only where the pre-activation is zero to rounding
            mask = (y.cpu() > 0)
            kind, L, pre64, cond = _lin_q(linear_contract_ref(inp, 0, bn, eps, mom), "y")
            flips = mask != (pre64 > 0)
            assert not bool(flips.any()) or float(pre64.abs()[flips].max()) <= layer_bound(kind, pre64, L, cond), f"{tag}: ReLU mask differs where z is not zero to rounding"
        ref = linear_contract_ref(inp, act, bn, eps, mom, mask=mask)
        for name, got in (("y", y),) + ((("z", z),) if (bn or act == 2) else ()) + ((("save_mean", sm), ("save_invstd", si)) if bn else ()) + \
                ((("running_mean", rm), ("running_var", rv)) if rm_on else ()):
            kind, L, r, cond = _lin_q(ref, name)
            _layer_close("linear_fwd", kind, got, r, L, f"{tag} {name}", cond)
        if not (bn or act == 2):
            assert _is_canary(z), f"{tag}: z written without batch-norm or swish"
        if not bn:
            assert _is_canary(sm) and _is_canary(si), f"{tag}: statistics written without batch-norm"
        if not rm_on:
            assert torch.equal(rm.cpu(), inp["rm0"]) and torch.equal(rv.cpu(), inp["rv0"]), f"{tag}: running statistics touched"
        bwd(dxc=dx if need_dx else None)
        G.intact(tag)
        for name, got, pre in (("dW", dW, 0.5), ("db", db, -0.25)) + ((("dgamma", dg, 0.125), ("dbeta", dbt, 2.0)) if bn else ()):
            kind, L, r, cond = _lin_q(ref, name)
            _layer_close("linear_bwd", kind, got.cpu().double() - pre, r, L, f"{tag} {name} (accumulated onto {pre})", cond + abs(pre))
        if need_dx:
            kind, L, r, cond = _lin_q(ref, "dx")
            _layer_close("linear_bwd", kind, dx, r, L, f"{tag} dx", cond)
        else:
            assert _is_canary(dx), f"{tag}: dx written although NULL was passed"
        if not bn:
            assert float((dg - 0.125).abs().max()) == 0 and float((dbt - 2.0).abs().max()) == 0
        # (dx at O > 64 is summed over 64-feature splits with fp32 atomics -- include/hifihr.h: the same bits only up to their order)
        now = [t_.clone() for t_ in (y, z, sm, si, rm, rv, dW, db, dg, dbt) + ((dx,) if O <= 64 else ())]
        assert first is None or all(torch.equal(p, q) for p, q in zip(first, now)), f"{what}: two runs differ"
        first = now
    # refusals on the accepted shape: null pointers, a bad act, sizes, the batch-norm rules
    keep = [t_.clone() for t_ in G.wholes()]
    for over in ({"x": None}, {"w": None}, {"y": None}):
        _refuses("linear_fwd", lambda: fwd(**over), G, f"{what}: null pointer")
    for over in ({"dy": None}, {"x": None}, {"w": None}):
        _refuses("linear_bwd", lambda: bwd(**over), G, f"{what}: null pointer")
    for kw in ({"actc": -1}, {"actc": 4}, {"Bc": 0}, {"Ic": 0}, {"Oc": 0}):
        _refuses("linear_fwd", lambda: fwd(**kw), G, f"{what}: {kw}")
        _refuses("linear_bwd", lambda: bwd(**kw), G, f"{what}: {kw}")
    if act == 1:
        _refuses("linear_bwd", lambda: bwd(y=None), G, f"{what}: act 1 without y")
    if act == 2:
        _refuses("linear_fwd", lambda: fwd(zc=None), G, f"{what}: swish without z")
    _refuses("linear_bwd", lambda: bwd(dzc=None), G, f"{what}: dx without dz_scratch")
    if bn:
        _refuses("linear_fwd", lambda: fwd(rvc=None), G, f"{what}: running_mean without running_var")
        _refuses("linear_fwd", lambda: fwd(rmc=None), G, f"{what}: running_var without running_mean")
    assert all(torch.equal(p, q) for p, q in zip(keep, G.wholes()))
    return True


def linear_group_contract_case(lib, device, members, seed=0):
    """hifihr_linear_fwd_group / _bwd_group: members = [(B, I, O, act, with_dx)], 1..6 of them, act 0 / 1: every member bit-identical to its
    single launch (hifihr_linear_fwd / _bwd), accumulators on a non-zero prefill.  -> accepted."""
    what = f"linear group {members}"
    G = Guards(device)
    ok = 1 <= len(members) <= LINEAR_MAX_GROUP and all(m[3] in (0, 1) and min(m[:3]) > 0 for m in members)
    grp, single = [], []
    for i, (B, I, O, act, with_dx) in enumerate(members):
        inp = linear_contract_inputs(max(B, 1), max(I, 1), max(O, 1), seed + i)
        Bq, Iq, Oq = max(B, 1), max(I, 1), max(O, 1)
        both = []
        for _ in range(2):
            both.append({"x": G.inp(inp["x"]), "w": G.inp(inp["w"]), "b": G.inp(inp["b"]) if i % 2 == 0 else None, "dy": G.inp(inp["gy"]), "act": act,
                         "y": G.out(Bq, Oq), "dz": G.out(Bq, Oq), "dW": G.out(Oq, Iq, fill=0.5) if i != 1 else None,
                         "db": G.out(Oq, fill=-0.25) if i != 1 else None, "dx": G.out(Bq, Iq) if with_dx else None})
        if min(B, I, O) <= 0:                                  # (the descriptor takes its sizes from the tensors: a refused size goes in by hand below)
            both[0]["sizes"] = (B, I, O)
        grp.append(both[0]); single.append(both[1])

    def descs():
        arr = lib._descs(grp)
        for d, m in zip(arr, grp):
            if "sizes" in m:
                d.B, d.I, d.O = m["sizes"]
        return arr

    from hifihr_amd._lib import _stream_of
    call = lambda name, n=None: lib.check(getattr(lib.c, name)(descs(), len(grp) if n is None else n, _stream_of(grp[0]["x"])), name)
    if not ok:
        _refuses("linear_fwd_group", lambda: call("hifihr_linear_fwd_group"), G, what)
        _refuses("linear_bwd_group", lambda: call("hifihr_linear_bwd_group"), G, what)
        return False
    for rep in range(2):
        for m in grp + single:
            for k, pre in (("y", None), ("dz", None), ("dx", None), ("dW", 0.5), ("db", -0.25)):
                if m[k] is not None:
                    m[k].fill_(_CANARY[torch.float32] if pre is None else pre)
        call("hifihr_linear_fwd_group")
        call("hifihr_linear_bwd_group")
        G.intact(what)
        for i, (g, s) in enumerate(zip(grp, single)):
            lib.linear_fwd(s["x"], s["w"], s["b"], s["act"], s["y"])
            lib.linear_bwd(s["dy"], s["y"], s["x"], s["w"], s["act"], s["dz"], s["dW"], s["db"], s["dx"])
            _layer_equal("linear_fwd_group", g["y"], s["y"], f"{what} member {i} y")
            for k in ("dW", "db", "dx"):
                if g[k] is not None and not (k == "dx" and members[i][2] > 64):
                    _layer_equal("linear_bwd_group", g[k], s[k], f"{what} member {i} {k}")
            if g["dx"] is not None and members[i][2] > 64:      # (fp32 atomics over the 64-feature splits: equal up to their order)
                ref = linear_contract_ref(linear_contract_inputs(*members[i][:3], seed + i), members[i][3], False, mask=(g["y"].cpu() > 0) if members[i][3] else None)
                kind, L, r, cond = _lin_q(ref, "dx")
                _layer_close("linear_bwd_group", kind, g["dx"], r, L, f"{what} member {i} dx", cond)
    G.intact(what)
    for n in (0, -1, LINEAR_MAX_GROUP + 1):
        _refuses("linear_fwd_group", lambda: call("hifihr_linear_fwd_group", n), G, f"{what}: n = {n}")
        _refuses("linear_bwd_group", lambda: call("hifihr_linear_bwd_group", n), G, f"{what}: n = {n}")
    return True

# ---- Winograd F(2x2, 3x3) / F(4x4, 3x3) transforms (csrc/wino.hip, wino4.hip) --------------------------------------------------------
# The oracle is float64 conv2d and its autograd, never the transform matrices: the kernel's own transforms are chained around a FLOAT64
# matmul in the test (kernel V and U cast to float64, product in torch, result cast to fp32 and handed to the kernel's output transform), so
# every channel count the transforms take (C % 4 == 0) is covered, not only those the library's GEMM takes; where it does take them the
# library product runs as well, into a canary-filled M / dU_parts, and must match the float64 product (kinds gemm_nt / gemm_tn).
WINO_CONTRACT_KINDS = ("wino_fwd", "wino4_fwd", "wino_wgrad", "wino4_wgrad")
LAYER_CONTRACT_C.update({
    # fwd kinds also hold backward-data (the same pipeline on dy, L = 9 K)
    "wino_fwd": (1.6e-7, 3e-5),       # 4.00e-08 x 4   F(2x2) y / dx, L = 9 C / 9 K: fp32 conv2d against float64             (wino_case 3e-5)
    "wino4_fwd": (4.9e-6, 5e-5),      # 1.23e-06 x 4   F(4x4) y / dx: the test's chain with an FP32 product on the emulator (fp32 direct convolution is another
    #                                                  algorithm: F(4x4)'s interpolation points amplify the rounding of V and U); the CAP, not c, binds from
    #                                                  C = 12 on (c sqrt(9 C) > 5e-5)                                   (wino_case 5e-5)
    "wino_wgrad": (1.6e-7, 1e-4),     # 3.93e-08 x 4   F(2x2) dw, L = N H W: fp32 conv2d autograd against float64                (wino_case 1e-4)
    "wino4_wgrad": (5.5e-6, 1e-4),    # 1.38e-06 x 4   F(4x4) dw: the chain with an fp32 product, as wino4_fwd; the cap binds from N H W = 331 on   (wino_case 1e-4)
})


def wino_contract_expect(N, H, W, C, K, m):
    """include/hifihr.h: m 2 or 4, C % 4 == 0 and K % 4 == 0 (the transforms move channels four at a time), any N, H, W > 0."""
    return m in (2, 4) and min(N, H, W) > 0 and C >= 4 and C % 4 == 0 and K >= 4 and K % 4 == 0


def wino_contract_inputs(N, H, W, C, K, seed):
    gen = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(N, C, H, W, generator=gen), "w": torch.randn(K, C, 3, 3, generator=gen) / (9 * C) ** 0.5,
            "gy": torch.randn(N, K, H, W, generator=gen), "bias": torch.randn(K, generator=gen) * 0.3}


def wino_contract_ref(inp, dt=torch.float64, drop_tap=False, drop_pixel=False):
    """conv2d (3x3, stride 1, pad 1) and its autograd in NHWC: name -> (L, tensor) for y, dx, dw.  drop_tap / drop_pixel: the detection
    check's reference without the filter's centre tap (y, dx) / without one output pixel's contribution (dw)."""
    import torch.nn.functional as Fn
    x, w, gy = (inp[k].to(dt) for k in ("x", "w", "gy"))
    if drop_tap:
        w = w.clone(); w[:, :, 1, 1] = 0
    if drop_pixel:
        gy = gy.clone(); gy[0, :, 0, 0] = 0
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = Fn.conv2d(xr, wr, None, 1, 1)
    y.backward(gy)
    N, C, H, W = x.shape
    K = w.shape[0]
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    return {"y": (9 * C, nhwc(y)), "dx": (9 * K, nhwc(xr.grad)), "dw": (N * H * W, nhwc(wr.grad))}


def _wino_fused_and_refused(lib, G, ent, what, N, H, W, C, K, m, P, T, w, wt, U, U2, V, V2, Yt, dUp, dw):
    """hifihr_weight_prep against the separate launches (bit for bit) and the refusals of the entries the chain only ever accepts."""
    from hifihr_amd._lib import _stream_of
    import ctypes
    # the per-step re-layout in one launch: transpose, U and U' of this layer == hifihr_weight_transpose / hifihr_wino_weight_transform
    kinds = (0, 1, 2) if m == 2 else (0, 3, 4)
    dsts = [G.out(C, 9, K), G.out(P, K, C), G.out(P, C, K)]
    table = lib.prep_jobs([(w, d, K, C, 9, k) for d, k in zip(dsts, kinds)], w.device)
    for blocks in (1, 3):
        for d in dsts:
            d.fill_(_CANARY[torch.float32])
        lib.weight_prep(table, 3, blocks)
        G.intact(what)
        for d, want, name in zip(dsts, (wt, U, U2), ("transpose", "U", "U' (flipped)")):
            _layer_equal(ent("weight_prep"), d.reshape(-1), want.reshape(-1), f"{what}: weight_prep {name}, {blocks} workgroups per job")
    for args in ((None, 3, 1), (table, 0, 1), (table, -1, 1), (table, 3, 0)):
        tb, nj, bl = args
        _refuses(ent("weight_prep"), lambda: lib.check(lib.c.hifihr_weight_prep(ctypes.c_void_p(tb.data_ptr() if tb is not None else 0), nj, bl, _stream_of(w)), "hifihr_weight_prep"),
                 G, f"{what}: weight_prep {('null table', nj, bl)}")
    # the weight-gradient transforms: a channel count that is no multiple of 4, no filters, no slabs, no jobs
    if m == 2:
        for Kb, Cb in ((K, C + 2), (0, C), (K, 0)):
            _refuses(ent("wino_dw_transform"), lambda: lib.wino_dw_transform(dUp[0], dw, Kb, Cb), G, f"{what}: wino_dw_transform K {Kb} C {Cb}")
        _refuses(ent("wino_dw_transform"), lambda: lib.wino_dw_transform(None, dw, K, C), G, f"{what}: wino_dw_transform null dU")
    else:
        for job in ((dUp, 2, dw, K, C + 2), (dUp, 0, dw, K, C), (dUp, 2, dw, 0, C), (dUp, 2, dw, K, 0)):
            _refuses(ent("wino4_dw_transform_multi"), lambda: lib.wino4_dw_transform_multi([(dUp, 2, dw, K, C), job]), G, f"{what}: multi, bad job {job[1:2] + job[3:]}")
        _refuses(ent("wino4_dw_transform_multi"), lambda: lib.check(lib.c.hifihr_wino4_dw_transform_multi(None, 1, _stream_of(w)), "hifihr_wino4_dw_transform_multi"), G, f"{what}: multi, null jobs")
        raw = ctypes.create_string_buffer(32)
        _refuses(ent("wino4_dw_transform_multi"), lambda: lib.check(lib.c.hifihr_wino4_dw_transform_multi(ctypes.cast(raw, ctypes.c_void_p), 0, _stream_of(w)), "hifihr_wino4_dw_transform_multi"), G, f"{what}: multi, no jobs")
        raw = ctypes.create_string_buffer(32)                                   # (a job of null pointers)
        _refuses(ent("wino4_dw_transform_multi"), lambda: lib.check(lib.c.hifihr_wino4_dw_transform_multi(ctypes.cast(raw, ctypes.c_void_p), 1, _stream_of(w)), "hifihr_wino4_dw_transform_multi"), G, f"{what}: multi, null pointers in a job")
        # the pair launch: its predicate answers 1 only where both products are the library's; the launch refuses other channel counts, a slab
        # count that is not the plan's, null pointers
        lib._pair_ok.pop((N, H, W, C, K), None)
        parts = lib.wino_wgrad_parts(N, H, W, C, K, 4)
        can = C % 64 == 0 and K % 64 == 0
        assert not lib.wino4_bwd_gemm_pair_supported(N, H, W, C, K) or (can and parts > 0), f"{what}: pair predicate on channels the products refuse"
        assert can == (parts > 0), f"{what}: hifihr_wino_wgrad_parts {parts}"
        M2, dUq = G.out(P, T, C), G.out(max(parts, 1) + 1, P, K, C)
        bad = [(V2, U2, M2, V, Yt, dUq, parts + 1), (V2, U2, M2, V, Yt, dUq, 0)] + ([] if can else [(V2, U2, M2, V, Yt, dUq, 1)])
        bad += [(None, U2, M2, V, Yt, dUq, max(parts, 1)), (V2, U2, None, V, Yt, dUq, max(parts, 1)), (V2, U2, M2, V, Yt, None, max(parts, 1))]
        for a in bad:
            _refuses(ent("wino4_bwd_gemm_pair"), lambda: lib.wino4_bwd_gemm_pair(*a[:6], N, H, W, C, K, a[6]), G, f"{what}: pair launch, parts {a[6]} / null pointer")


def wino_chain_contract_case(lib, device, N, H, W, C, K, m, seed=0, product=torch.float64, log=True):
    """Every transform entry of one layer around a float64 (product=...) matmul; -> accepted.  Buffers between the stages are prefilled
    with the canary in the first run and NaN in the second: results must not depend on it."""
    what = f"wino {N}x{H}x{W} C {C} K {K} m {m}"
    P = (m + 2) ** 2 if m > 0 else 16
    ok = wino_contract_expect(N, H, W, C, K, m)
    nan = float("nan")
    Nq, Hq, Wq, Cq, Kq = (max(v, 1) for v in (N, H, W, C, K))
    inp = wino_contract_inputs(Nq, Hq, Wq, Cq, Kq, seed)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    if not ok:
        G = Guards(device)
        Tq = Nq * Hq * Wq
        x, w, gy = G.inp(nhwc(inp["x"])), G.inp(nhwc(inp["w"])), G.inp(nhwc(inp["gy"]))
        U, V, Mm, Yt, y, dw = G.out(36, Kq, Cq), G.out(36, Tq, Cq), G.out(36, Tq, Kq), G.out(36, Tq, Kq), G.out(Nq, Hq, Wq, Kq), G.out(Kq, 3, 3, Cq)
        Vk = G.out(36, Tq, Kq)
        assert m in (2, 4) or (lib.wino_tiles(N, H, W, m) == 0 and lib.wino_tiles_computed(N, H, W, m) == 0 and lib.wino_wgrad_parts(N, H, W, 64, 64, m) == 0
                               and lib.wino_gemm_workspace_bytes(N, H, W, 64, 64, m) == 0), f"{what}: a query answers for an m that is refused"
        geo_ok, c_ok, k_ok = m in (2, 4) and min(N, H, W) > 0, C >= 4 and C % 4 == 0, K >= 4 and K % 4 == 0
        calls = {}
        if not (geo_ok and c_ok):                                            # the entries that see C ...
            calls.update({"wino_input_transform": lambda: lib.wino_input_transform(x, V, N, H, W, C, m)})
        if not (m in (2, 4) and c_ok and K > 0):
            calls.update({"wino_weight_transform": lambda: lib.wino_weight_transform(w, U, K, C, 0, m),
                          "wino_dw_transform_parts": lambda: lib.wino_dw_transform_parts(U, 1, dw, K, C, m)})
        if not (geo_ok and k_ok):                                            # ... and those that see K
            calls.update({"wino_output_transform": lambda: lib.wino_output_transform(Mm, y, None, N, H, W, K, m=m),
                          "wino_output_transform_act": lambda: lib.wino_output_transform(Mm, y, None, N, H, W, K, act=1, m=m),
                          "wino_dy_transform": lambda: lib.wino_dy_transform(gy, Yt, N, H, W, K, m),
                          "wino_input_dy_transform": lambda: lib.wino_input_dy_transform(gy, Vk, Yt, N, H, W, K, m)})
        if m not in (2, 4):                                                  # (a bad m: the products too; sizes the products would take)
            calls["wino_gemm"] = lambda: lib.wino_gemm(V, U, Mm, N, H, W, C, K, m=m)
            calls["wino_wgrad_gemm_parts"] = lambda: lib.wino_wgrad_gemm_parts(V, Yt, U, N, H, W, C, K, 1, m)
        for e, call in calls.items():
            _refuses(e, call, G, f"{what}: {e}")
        return False
    T, Tr = lib.wino_tiles(N, H, W, m), lib.wino_tiles_computed(N, H, W, m)
    assert 0 < Tr <= T
    ref = wino_contract_ref(inp)
    fk, wk = ("wino4_fwd", "wino4_wgrad") if m == 4 else ("wino_fwd", "wino_wgrad")
    ent = lambda e: e if log else "_" + e
    results = []
    for prefill in (None, nan):
        G = Guards(device)
        x, w, gy, bias = G.inp(nhwc(inp["x"])), G.inp(nhwc(inp["w"])), G.inp(nhwc(inp["gy"])), G.inp(inp["bias"])
        U, V = G.out(P, K, C, fill=prefill), G.out(P, T, C, fill=prefill)
        lib.wino_weight_transform(w, U, K, C, 0, m)
        lib.wino_input_transform(x, V, N, H, W, C, m)
        G.intact(what)
        assert not bool(torch.isnan(V[:, :Tr]).any()) and not bool((V[:, :Tr] == _CANARY[torch.float32]).any()), f"{what}: a computed row of V is unwritten"
        assert T == Tr or float(V[:, Tr:].abs().max()) == 0.0, f"{what}: the rows of V behind the last mosaic tile are not zero"
        Mm = torch.matmul(V.cpu().to(product), U.cpu().to(product).transpose(1, 2)).float()      # [P][T][K]
        Mm[:, Tr:] = nan                                                        # (unread by the output transform)
        Md = G.inp(Mm)
        y = G.out(N, H, W, K)
        stats = G.out(lib.bn_stats_floats(K), fill=0.0)
        lib.wino_output_transform(Md, y, stats, N, H, W, K, m=m)
        G.intact(what)
        _layer_close(ent("wino_output_transform"), fk, y, ref["y"][1], ref["y"][0], f"{what} y")
        flat = ref["y"][1].reshape(-1, K)
        st = bn_slots(stats, K).sum(0).cpu()
        _layer_close(ent("wino_output_transform"), "bn_sum", st[0], flat.sum(0), N * H * W, f"{what} statistics: sum", cond=float(flat.abs().sum(0).max()) * layer_bound(fk, torch.ones(1), ref["y"][0]) / LAYER_CONTRACT_C["bn_sum"][0])
        # the consumer (include/hifihr.h "SELF-CLEANING"): hifihr_bn_act_fwd folds the slots this producer filled and hands the slots and
        # arrival counters back all zero; its batch mean is the mean of the y just compared
        gam, bet = G.inp(torch.ones(K)), G.inp(torch.zeros(K))
        ybn, smean, sinv = G.out(N, H, W, K), G.out(K), G.out(K)
        lib.bn_act_fwd(y, stats, gam, bet, None, 0, N * H * W, K, 1e-5, 0.1, ybn, smean, sinv, None, None)
        G.intact(what)
        _slots_clean(stats, K, f"{what}: statistics slots / counters not handed back zeroed by their consumer")
        stats.zero_()                                                          # (the 2 K scratch floats behind them are not part of the promise)
        assert layer_err(smean, flat.mean(0)) <= layer_bound(fk, ref["y"][1], ref["y"][0]) + 1e-6 * float(flat.abs().max()), f"{what}: batch mean from the slots"
        y0 = G.out(N, H, W, K)
        lib.wino_output_transform(Md, y0, None, N, H, W, K, m=m)
        assert torch.equal(y0, y), f"{what}: y depends on whether statistics are taken"
        for act in (0, 1):
            ya = G.out(N, H, W, K)
            lib.wino_output_transform(Md, ya, None, N, H, W, K, bias=bias, act=act, m=m)
            ra = ref["y"][1] + inp["bias"].double()
            _layer_close(ent("wino_output_transform_act"), fk, ya, torch.relu(ra) if act else ra, ref["y"][0], f"{what} bias, act {act}", cond=float(ref["y"][1].abs().max()))
        _refuses(ent("wino_output_transform_act"), lambda: lib.wino_output_transform(Md, ya, None, N, H, W, K, bias=bias, act=2, m=m), G, f"{what}: act 2")
        # backward-data: the same pipeline on dy with the transposed, rotated filter
        wt = G.out(C, 3, 3, K, fill=prefill)
        lib.weight_transpose(w, wt, K, 9, C)
        U2, V2 = G.out(P, C, K, fill=prefill), G.out(P, T, K, fill=prefill)
        lib.wino_weight_transform(wt, U2, C, K, 1, m)
        lib.wino_input_transform(gy, V2, N, H, W, K, m)
        V2b, Ytb, Yt = G.out(P, T, K, fill=prefill), G.out(P, T, K, fill=prefill), G.out(P, T, K, fill=prefill)
        lib.wino_input_dy_transform(gy, V2b, Ytb, N, H, W, K, m)
        lib.wino_dy_transform(gy, Yt, N, H, W, K, m)
        G.intact(what)
        _layer_equal(ent("wino_input_dy_transform"), V2b[:, :Tr], V2[:, :Tr], f"{what}: dual dy transform, V")
        _layer_equal(ent("wino_input_dy_transform"), Ytb[:, :Tr], Yt[:, :Tr], f"{what}: dual dy transform, Y'")
        assert T == Tr or (float(V2b[:, Tr:].abs().max()) == 0.0 and float(Ytb[:, Tr:].abs().max()) == 0.0 and float(Yt[:, Tr:].abs().max()) == 0.0), \
            f"{what}: the rows of V / Y' behind the last mosaic tile are not zero"
        M2 = torch.matmul(V2.cpu().to(product), U2.cpu().to(product).transpose(1, 2)).float()
        M2[:, Tr:] = nan
        dx = G.out(N, H, W, C)
        lib.wino_output_transform(G.inp(M2), dx, None, N, H, W, C, m=m)
        _layer_close(ent("wino_output_transform"), fk, dx, ref["dx"][1], ref["dx"][0], f"{what} dx")
        # backward-weight: dU = Y'^T V per position, in two slabs, accumulated onto a prefilled dw
        dU = torch.matmul(Yt.cpu().to(product).transpose(1, 2), V.cpu().to(product))                # [P][K][C]
        half = (dU * 0.5).float()
        dUp = G.inp(torch.stack([half, (dU - half.to(product)).float()]))
        dw = G.out(K, 3, 3, C, fill=0.5)
        lib.wino_dw_transform_parts(dUp, 2, dw, K, C, m)
        G.intact(what)
        _layer_close(ent("wino_dw_transform_parts"), wk, dw.cpu().double() - 0.5, ref["dw"][1], ref["dw"][0], f"{what} dw (slabs)", cond=0.5)
        if m == 4:                                                              # several layers in one launch: the per-layer call's bits
            dwm, dwn = G.out(K, 3, 3, C, fill=0.5), G.out(K, 3, 3, C, fill=-1.0)
            lib.wino4_dw_transform_multi([(dUp, 2, dwm, K, C), (dUp[1:], 1, dwn, K, C)])
            dws = G.out(K, 3, 3, C, fill=-1.0)
            lib.wino_dw_transform_parts(dUp[1:], 1, dws, K, C, m)
            _layer_equal(ent("wino4_dw_transform_multi"), dwm, dw, f"{what}: multi, job 0")
            _layer_equal(ent("wino4_dw_transform_multi"), dwn, dws, f"{what}: multi, job 1")
        else:                                                                   # the atomics form: dU read, then handed back all zero
            dUa, dwa = G.out(P, K, C), G.out(K, 3, 3, C, fill=0.5)
            dUa.copy_(dU.float())
            lib.wino_dw_transform(dUa, dwa, K, C)
            assert float(dUa.abs().max()) == 0.0, f"{what}: the dU accumulator must come back zeroed"
            _layer_close(ent("wino_dw_transform"), "wino_wgrad", dwa.cpu().double() - 0.5, ref["dw"][1], ref["dw"][0], f"{what} dw (atomics form)", cond=0.5)
        G.intact(what)
        results.append([t.clone() for t in (U, V[:, :Tr], y, dx, dw, Yt[:, :Tr])])
        if prefill is None:
            _wino_fused_and_refused(lib, G, ent, what, N, H, W, C, K, m, P, T, w, wt, U, U2, V, V2, Yt, dUp, dw)
        # the library's own products, where it takes the channel counts: into canary-filled M / dU_parts
        if prefill is None and C % 32 == 0 and K % 64 == 0 and C % 64 == 0 and product == torch.float64:
            nb = lib.wino_gemm_workspace_bytes(N, H, W, C, K, m)
            ws = G.out(nb // 4, fill=0.0) if nb else None
            Ml = G.out(P, T, K)
            lib.wino_gemm(V, U, Ml, N, H, W, C, K, ws=ws, m=m)
            G.intact(what)
            assert ws is None or float(ws.abs().max()) == 0.0
            _layer_close(ent("wino_gemm"), "gemm_nt", Ml[:, :Tr], torch.matmul(V[:, :Tr].cpu().double(), U.cpu().double().transpose(1, 2)), C, f"{what} M")
            parts = lib.wino_wgrad_parts(N, H, W, C, K, m)
            if parts > 0:
                dUl = G.out(parts + 1, P, K, C)
                lib.wino_wgrad_gemm_parts(V, Yt, dUl, N, H, W, C, K, parts, m)
                G.intact(what)
                assert _is_canary(dUl[parts])
                _layer_close(ent("wino_wgrad_gemm_parts"), "gemm_tn", dUl[:parts].double().sum(0), dU.double(), T, f"{what} dU slabs")
                _refuses(ent("wino_wgrad_gemm_parts"), lambda: lib.wino_wgrad_gemm_parts(V, Yt, dUl, N, H, W, C, K, parts + 1, m), G, f"{what}: parts + 1")
                if m == 4:                                                      # both backward products in one launch: the separate launches' bits
                    M2a, M2b, dUq = G.out(P, T, C), G.out(P, T, C), G.out(parts, P, K, C)
                    lib.wino_gemm(V2, U2, M2a, N, H, W, K, C, ws=None, m=m)
                    lib.wino4_bwd_gemm_pair(V2, U2, M2b, V, Yt, dUq, N, H, W, C, K, parts)
                    G.intact(what)
                    _layer_equal(ent("wino4_bwd_gemm_pair"), M2b[:, :Tr], M2a[:, :Tr], f"{what}: pair launch, M2")
                    _layer_equal(ent("wino4_bwd_gemm_pair"), dUq, dUl[:parts], f"{what}: pair launch, dU slabs")
                    # (rows behind the last mosaic tile: unread by the output transform; the row-share kernel skips them, the per-tile
                    # kernels write the product of V's zero rows)
                    pad_ok = lambda t: _is_canary(t) or float(t.abs().max()) == 0.0
                    assert T == Tr or (pad_ok(M2b[:, Tr:]) and pad_ok(Ml[:, Tr:])), f"{what}: rows of M behind the last mosaic tile are neither untouched nor zero"
    assert all(torch.equal(a, b) for a, b in zip(*results)), f"{what}: a result depends on the prefill of a buffer between two stages"
    return True



# ---- batch-norm fused into the F(4x4, 3x3) transforms (csrc/wino4_bn.hip) ---------------------------------------------------------------
def wino_bn_contract_expect(C, m):
    """include/hifihr.h: m = 4, C % 4 == 0, C <= 512 (hifihr_wino_bn_input_supported)."""
    return m == 4 and C >= 4 and C % 4 == 0 and C <= 512


def wino_bn_contract_case(lib, device, N, H, W, C, m, residual, addend, seed=0):
    """hifihr_wino_bn_input_transform, hifihr_wino_output_transform_bnred and hifihr_wino_bn_bwd_dual_transform inside guard bands: refused
    (HIFIHR_EINVAL, nothing written), or bit-identical to the separate launches they replace -- hifihr_bn_act_fwd + input transform,
    output transform (+ addend) + the masking of hifihr_bn_act_bwd, hifihr_bn_bwd_apply + dual dy transform -- each of which has its own
    contract against float64; statistics and reduction buffers handed back zeroed; twice, identical bits.  -> accepted."""
    what = f"wino_bn {N}x{H}x{W} C {C} m {m} residual {residual} addend {addend}"
    ok = wino_bn_contract_expect(C, m)
    assert lib.wino_bn_input_supported(C, m) == ok, f"{what}: hifihr_wino_bn_input_supported"
    gen = torch.Generator().manual_seed(seed)
    G = Guards(device)
    Cq, M = max(C, 4), N * H * W
    T = lib.wino_tiles(N, H, W, 4)
    x = G.inp(torch.randn(N, H, W, Cq, generator=gen) * 1.3 + 0.2)
    res = G.inp(torch.randn(N, H, W, Cq, generator=gen)) if residual else None
    gadd = G.inp(torch.randn(N, H, W, Cq, generator=gen)) if addend else None
    gamma, beta = G.inp(1 + 0.1 * torch.randn(Cq, generator=gen)), G.inp(0.1 * torch.randn(Cq, generator=gen))
    Mm = G.inp(torch.randn(36, T, Cq, generator=gen))
    nst = lib.bn_stats_floats(Cq)
    st, red = G.out(nst, fill=0.0), G.out(nst, fill=0.0)
    V1, out1, g1 = G.out(36, T, Cq), (G.out(N, H, W, Cq) if residual else None), G.out(N, H, W, Cq)
    sm1, si1, rm1, rv1 = G.out(Cq), G.out(Cq), G.out(Cq, fill=0.0), G.out(Cq, fill=1.0)
    V2, Y2, dg2, db2 = G.out(36, T, Cq), G.out(36, T, Cq), G.out(Cq, fill=0.5), G.out(Cq, fill=-0.25)
    fused_in = lambda Cc=C, mm=m, o=out1, r=res: lib.wino_bn_input_transform(x, st, gamma, beta, r, o, V1, N, H, W, Cc, mm, 1e-5, 0.1, sm1, si1, rm1, rv1)
    fused_red = lambda Cc=C, mm=m: lib.wino_output_transform_bnred(Mm, x, out1, gadd, sm1, si1, gamma, beta, red, g1, N, H, W, Cc, mm)
    fused_dual = lambda Cc=C, mm=m: lib.wino_bn_bwd_dual_transform(g1, x, sm1, si1, gamma, red, V2, Y2, N, H, W, Cc, mm, dg2, db2)
    if not ok:
        for e, call in (("wino_bn_input_transform", fused_in), ("wino_output_transform_bnred", fused_red), ("wino_bn_bwd_dual_transform", fused_dual)):
            _refuses(e, call, G, f"{what}: {e}")
        return False
    # the separate launches (plain buffers: their own contracts guard them)
    d0 = lambda *s: torch.empty(*s, device=device)
    st0 = torch.zeros(nst, device=device)
    lib.bn_stats(x, M, C, st0)
    a0, sm0, si0, rm0, rv0 = d0(N, H, W, C), d0(C), d0(C), torch.zeros(C, device=device), torch.ones(C, device=device)
    lib.bn_act_fwd(x, st0, gamma, beta, res, 1, M, C, 1e-5, 0.1, a0, sm0, si0, rm0, rv0)
    V0 = d0(36, T, C)
    lib.wino_input_transform(a0, V0, N, H, W, C, 4)
    dA = d0(N, H, W, C)
    lib.wino_output_transform(Mm, dA, None, N, H, W, C, m=4)
    dA = dA + gadd if addend else dA
    red0 = torch.zeros(nst, device=device)
    dx0, dres0, dg0, db0 = d0(N, H, W, C), d0(N, H, W, C), torch.zeros(C, device=device), torch.zeros(C, device=device)
    lib.bn_act_bwd(dA, a0 if residual else None, x, sm0, si0, gamma, beta, 1, M, C, red0, dx0, dres0, dg0, db0)
    first = None
    for rep in range(2):
        for t in (V1, g1, V2, Y2, sm1, si1) + ((out1,) if residual else ()):
            t.fill_(_CANARY[torch.float32])
        rm1.fill_(0.0); rv1.fill_(1.0); dg2.fill_(0.5); db2.fill_(-0.25)
        lib.bn_stats(x, M, C, st)
        fused_in()
        G.intact(what)
        _slots_clean(st, C, f"{what}: statistics not handed back zeroed")
        _layer_equal("wino_bn_input_transform", V1, V0, f"{what}: V")
        for got, want, n in ((sm1, sm0, "save_mean"), (si1, si0, "save_invstd"), (rm1, rm0, "running_mean"), (rv1, rv0, "running_var")) + (((out1, a0, "out"),) if residual else ()):
            _layer_equal("wino_bn_input_transform", got, want, f"{what}: {n}")
        fused_red()
        G.intact(what)
        _layer_equal("wino_output_transform_bnred", g1, dres0, f"{what}: masked gradient")
        # the sums the fused reduction left in `red`, through both of their consumers: hifihr_bn_bwd_apply, and the dual transform on a copy
        red_copy = red.clone()
        dx1, dg1, db1 = d0(N, H, W, C), torch.full((C,), 0.5, device=device), torch.full((C,), -0.25, device=device)
        lib.bn_bwd_apply(g1, x, sm1, si1, gamma, M, C, red, dx1, dg1, db1)
        _slots_clean(red, C, f"{what}: reduction buffer not handed back zeroed by hifihr_bn_bwd_apply")
        err = float((dx1 - dx0).abs().max())                                  # (the reductions add in another order: wino_bn_bwd_case's tolerance)
        assert err <= 2e-5 * float(dx0.abs().max()) + 1e-7, f"{what}: dx through the fused reduction: {err}"
        red.copy_(red_copy)
        fused_dual()
        G.intact(what)
        _slots_clean(red, C, f"{what}: reduction buffer not handed back zeroed by the dual transform")
        V0b, Y0b = d0(36, T, C), d0(36, T, C)
        lib.wino_input_dy_transform(dx1, V0b, Y0b, N, H, W, C, 4)
        _layer_equal("wino_bn_bwd_dual_transform", V2, V0b, f"{what}: V of dx")
        _layer_equal("wino_bn_bwd_dual_transform", Y2, Y0b, f"{what}: Y' of dx")
        _layer_equal("wino_bn_bwd_dual_transform", dg2, dg1, f"{what}: dgamma (accumulated onto 0.5)")
        _layer_equal("wino_bn_bwd_dual_transform", db2, db1, f"{what}: dbeta (accumulated onto -0.25)")
        red.zero_()
        now = [t.clone() for t in (V1, g1, V2, Y2, sm1, si1, rm1, rv1, dg2, db2)]
        assert first is None or all(torch.equal(a, b) for a, b in zip(first, now)), f"{what}: two runs differ"
        first = now
    # refusals on the accepted shape: the other tile edge, residual without out (and the reverse), null pointers
    for e, call in (("wino_bn_input_transform", fused_in), ("wino_output_transform_bnred", fused_red), ("wino_bn_bwd_dual_transform", fused_dual)):
        _refuses(e, lambda: call(mm=2), G, f"{what}: {e} at m = 2")
        _refuses(e, lambda: call(Cc=C + 2), G, f"{what}: {e} at C + 2")
    _refuses("wino_bn_input_transform", (lambda: fused_in(o=None)) if residual else (lambda: fused_in(o=g1)), G, f"{what}: residual and out: both or neither")
    return True


# ---- the lists of the GEMM contract (tests/test_hostsim_gemm_contract.py, the GPU halves, tools/layer_contract_c.py, tools/asan_hostsim.py) ----
import os as _os

# ---- routing: name -> environment (every HIFIHR_GEMM_* switch not named is removed for the case) -------------------------------------------
GEMM_SWITCHES = ("HIFIHR_GEMM_CUS", "HIFIHR_GEMM_NT_TILE", "HIFIHR_GEMM_TN_TILE", "HIFIHR_GEMM_WS", "HIFIHR_GEMM_TN_PARTS", "HIFIHR_GEMM_SK")
GEMM_ROUTES = {
    "default": {},
    "cus16": {"HIFIHR_GEMM_CUS": "16"},                                           # a multiple of 8 workgroups: the XCD-coherent TN schedule
    "t128": {"HIFIHR_GEMM_NT_TILE": "128128", "HIFIHR_GEMM_TN_TILE": "128128", "HIFIHR_GEMM_WS": "0"},      # the 4-wave kernels
    "t128x64": {"HIFIHR_GEMM_NT_TILE": "128064", "HIFIHR_GEMM_TN_TILE": "128064"},
    "t64x128": {"HIFIHR_GEMM_NT_TILE": "64128", "HIFIHR_GEMM_TN_TILE": "64128"},
    "t64": {"HIFIHR_GEMM_NT_TILE": "64064", "HIFIHR_GEMM_TN_TILE": "64064"},
    "ws1": {"HIFIHR_GEMM_NT_TILE": "128128", "HIFIHR_GEMM_TN_TILE": "128128", "HIFIHR_GEMM_WS": "1"},       # wave-specialised, 1 / 2 / 4 loader waves
    "ws2": {"HIFIHR_GEMM_NT_TILE": "128128", "HIFIHR_GEMM_TN_TILE": "128128", "HIFIHR_GEMM_WS": "2"},
    "ws4": {"HIFIHR_GEMM_NT_TILE": "128128", "HIFIHR_GEMM_TN_TILE": "128128", "HIFIHR_GEMM_WS": "4"},
    "ws2p3": {"HIFIHR_GEMM_TN_TILE": "128128", "HIFIHR_GEMM_WS": "2", "HIFIHR_GEMM_TN_PARTS": "3"},         # a slab count of the caller's
}

# ---- NT: (M, N, K, batch, route, workspace) -------------------------------------------------------------------------------------------------
# M in {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300}, N in {64, 128, 192, 256, 576 (K = 128: ragged N on the row-share kernel)},
# K in {32, 64, 96, 160, 512}, batch in {1, 2, 5, 36}
NT_SHAPES = [
    (1, 64, 32, 1, "default", "full"), (15, 128, 32, 2, "default", "full"), (16, 128, 64, 1, "default", "full"), (17, 192, 96, 2, "default", "full"),
    (63, 256, 32, 5, "default", "full"), (64, 64, 160, 1, "default", "full"), (65, 128, 96, 2, "default", "full"), (127, 128, 160, 2, "default", "full"),
    (128, 256, 64, 1, "default", "full"), (129, 64, 512, 1, "default", "full"), (17, 128, 512, 2, "default", "full"), (1, 128, 512, 5, "default", "full"),
    (16, 192, 32, 36, "default", "full"), (17, 128, 32, 36, "default", "full"), (17, 256, 160, 5, "default", "full"), (63, 192, 64, 1, "default", "full"), (127, 64, 96, 5, "default", "full"),
    (128, 192, 160, 2, "default", "full"), (65, 256, 512, 1, "default", "full"), (300, 256, 96, 2, "default", "full"), (300, 64, 64, 2, "default", "full"),
    (15, 576, 128, 1, "default", "full"), (129, 576, 128, 2, "default", "full"), (300, 576, 128, 1, "default", "full"), (1, 576, 128, 5, "default", "full"),
    (129, 128, 64, 2, "t128", "full"), (300, 256, 32, 1, "t128", "full"), (1, 128, 96, 1, "t128", "full"),
    (65, 64, 64, 2, "t128x64", "full"), (300, 192, 32, 1, "t128x64", "full"), (63, 128, 96, 2, "t64x128", "full"), (129, 256, 32, 1, "t64x128", "full"),
    (17, 128, 32, 5, "t64", "full"), (127, 256, 64, 1, "t64", "full"),
    (127, 128, 160, 2, "ws1", "full"), (300, 256, 32, 1, "ws2", "full"), (129, 128, 96, 2, "ws4", "full"),
    # 128x128 tiles over >= 3 rounds of the 4 workgroups: the persistent stream-K kernel with its workspace, the per-tile fallback without
    (300, 128, 96, 5, "ws2", "full"), (300, 128, 64, 5, "ws4", "full"), (300, 128, 96, 5, "ws1", "full"),
    (300, 128, 96, 5, "ws2", "short"), (300, 128, 96, 5, "ws4", "none"),
    # refused: K in {0, 16, 48}, N in {0, 32, 96}, M = 0, batch = 0
    (17, 128, 0, 1, "default", "none"), (17, 128, 16, 1, "default", "none"), (17, 128, 48, 1, "default", "none"),
    (17, 0, 32, 1, "default", "none"), (17, 32, 32, 1, "default", "none"), (17, 96, 32, 1, "default", "none"),
    (0, 128, 32, 1, "default", "none"), (17, 128, 32, 0, "default", "none"), (17, 96, 128, 1, "default", "none"),
    # beyond 32-bit element offsets (M K = 2^31, N K = 2^31): the predicate alone, nothing large is allocated
    (2 ** 26, 64, 32, 1, "default", "none"), (1, 2 ** 26, 32, 1, "default", "none"),
]

# ---- TN: (M, N, T, batch, route) ---------------------------------------------------------------------------------------------------------------
# M, N in {64, 128, 192, 256, 320}, T in {1, 4, 31, 32, 33, 63, 64, 65, 96, 777} (+ 256: the T-split on 4 compute units), batch in {1, 2, 16, 36}
TN_SHAPES = [
    (64, 64, 1, 1, "default"), (64, 128, 4, 2, "default"), (128, 64, 31, 1, "default"), (128, 128, 32, 2, "default"), (192, 64, 33, 1, "default"),
    (64, 192, 63, 2, "default"), (256, 128, 64, 1, "default"), (64, 256, 65, 16, "default"), (320, 320, 33, 1, "default"), (64, 64, 777, 1, "default"),
    (256, 256, 777, 1, "default"), (64, 64, 32, 36, "default"), (256, 320, 31, 2, "default"), (192, 192, 96, 1, "default"), (64, 128, 1, 36, "default"),
    # the row-share kernel, complete products in one slab: N % 128 == 0, T % 32 == 0, T >= 64, eight 16-row blocks per compute unit
    (128, 128, 64, 16, "default"), (320, 128, 96, 2, "default"), (192, 256, 96, 2, "default"), (64, 128, 64, 36, "default"), (320, 256, 64, 2, "default"),
    (128, 128, 256, 2, "default"),                                   # too few blocks, 8 chunks: the T-split, two slabs
    (256, 128, 64, 16, "cus16"),                                     # the XCD-coherent schedule
    (128, 128, 65, 2, "t128"), (256, 128, 777, 1, "t128"), (128, 64, 96, 2, "t128x64"), (256, 192, 33, 1, "t128x64"), (64, 128, 63, 2, "t64x128"),
    (192, 256, 4, 1, "t64x128"), (128, 128, 96, 1, "t64"),
    (128, 256, 96, 2, "ws1"), (256, 128, 33, 1, "ws2"), (128, 128, 777, 1, "ws4"), (128, 128, 777, 1, "ws2p3"),
    # refused
    (0, 64, 32, 1, "default"), (32, 64, 32, 1, "default"), (96, 64, 32, 1, "default"), (64, 0, 32, 1, "default"), (64, 96, 32, 1, "default"),
    (64, 64, 0, 1, "default"), (64, 64, 32, 0, "default"),
]

# ---- hifihr_weight_transpose: (K, RS, C) -----------------------------------------------------------------------------------------------------
TRANSPOSE_SHAPES = [(1, 1, 1), (3, 9, 5), (64, 9, 3), (7, 1, 64), (33, 9, 31), (64, 49, 4), (130, 1, 257), (256, 9, 64),
                    (0, 9, 4), (4, 0, 4), (4, 9, 0), (-1, 9, 4)]

# ---- fully connected: (B, I, O, act, bn, running, need_dx) -------------------------------------------------------------------------------------
# B in {1, 2, 31, 32, 33, 63, 64, 65, 70, 129} (32- and 64-row blocks of the forward, one to three of them), I in {1, 3, 4, 31, 32, 33, 36, 72,
# 128, 1038, 1100} (16-byte loads at I % 4 == 0, the 32-wide chunks), O in {1, 3, 20, 33, 48, 300}, act 0..3; batch-norm at B in {1, 2, 64}
LINEAR_SHAPES = [
    (1, 1, 1, 0, False, False, True), (2, 3, 3, 1, False, False, True), (31, 4, 20, 2, False, False, True), (32, 31, 33, 3, False, False, True),
    (33, 32, 48, 1, False, False, False), (63, 33, 300, 0, False, False, True), (64, 36, 1, 1, False, False, True), (65, 72, 3, 2, False, False, False),
    (70, 128, 20, 3, False, False, True), (129, 1038, 33, 1, False, False, True), (2, 1100, 48, 0, False, False, True), (32, 128, 300, 1, False, False, True),
    (129, 4, 3, 0, False, False, True), (1, 1038, 300, 2, False, False, True), (64, 1100, 20, 3, False, False, False),
    (1, 36, 20, 1, True, True, True), (2, 72, 33, 1, True, True, True), (64, 128, 48, 1, True, True, True), (64, 33, 300, 0, True, False, True),
    (2, 3, 1, 0, True, True, False), (1, 1100, 3, 0, True, False, True), (32, 31, 20, 1, True, True, True),
    # refused: batch-norm above 64 rows, batch-norm with swish / sigmoid
    (65, 36, 20, 1, True, True, True), (32, 36, 20, 2, True, True, True), (32, 36, 20, 3, True, True, True),
]
# groups: members (B, I, O, act, with_dx); 1..6 members, different sizes in one launch, with and without dx
LINEAR_GROUPS = [
    [(32, 36, 20, 1, True)],
    [(2, 3, 1, 0, True), (33, 128, 48, 1, False)],
    [(1, 1, 3, 1, True), (64, 72, 20, 0, True), (65, 33, 33, 1, False), (31, 4, 300, 0, True), (129, 32, 3, 1, True), (70, 1038, 20, 0, False)],
    [(32, 128, 48, 1, True), (32, 128, 48, 0, True), (32, 1100, 1, 1, False)],
    # refused: 7 members, act 2 / 3
    [(2, 4, 4, 0, True)] * 7, [(2, 4, 4, 0, True), (2, 4, 4, 2, True)], [(2, 4, 4, 3, True)],
]

# ---- Winograd transforms: (N, H, W, C, K), each at m = 2 and m = 4 ----------------------------------------------------------------------------
# H, W in {1, 2, 3, 4, 5, 6, 7, 9, 13, 14} (images below one tile, ragged last tiles, non-square), N in {1, 2, 3, 16, 17, 32} (at m = 4 the
# tiles of 16 square images with H % 4 in {1, 2} are cut from 4 x 4-image mosaics: those and their plain neighbours), C, K in {4, 8, 24, 32, 64,
# 100} for the transforms alone and 64 / 128 where the library's own products run as well
WINO_LAYERS = [
    (1, 1, 1, 4, 8), (1, 2, 3, 8, 4), (2, 3, 1, 24, 32), (1, 4, 2, 32, 24), (1, 5, 6, 100, 8), (3, 6, 5, 8, 100), (1, 7, 9, 64, 4), (2, 9, 7, 4, 64),
    (1, 13, 14, 8, 8), (1, 14, 13, 24, 4),
    (16, 5, 5, 4, 4), (16, 6, 6, 8, 4), (17, 5, 5, 4, 8), (16, 5, 6, 4, 4), (32, 5, 5, 4, 4), (16, 13, 13, 4, 4), (16, 14, 14, 4, 4), (16, 7, 7, 4, 4),
    (1, 4, 4, 64, 64), (2, 7, 5, 128, 64), (3, 9, 9, 8, 24), (16, 6, 6, 64, 64),
]
WINO_GEOMS = [g + (m,) for g in WINO_LAYERS for m in (2, 4)]
WINO_GEOMS += [(1, 4, 4, 8, 8, 0), (1, 4, 4, 8, 8, 3), (1, 4, 4, 8, 8, 8), (2, 5, 5, 64, 64, 3),               # refused: m
               (1, 4, 4, 6, 8, 2), (1, 4, 4, 6, 8, 4), (1, 4, 4, 8, 6, 2), (1, 4, 4, 8, 6, 4), (1, 4, 4, 0, 8, 4),      # refused: C, K
               (0, 4, 4, 8, 8, 4), (1, 0, 4, 8, 8, 2), (1, 4, 0, 8, 8, 4)]                                           # refused: N, H, W

# the F(4x4) layer whose two backward products the emulator takes as ONE launch (hifihr_wino4_bwd_gemm_pair_supported) wants 16 compute units
WINO_LAYERS.append((16, 5, 5, 128, 128))
WINO_LAYERS.append((1, 4, 4, 176, 192))                    # K C / 4 > 8192: the weight-gradient transform's second kernel
WINO_GEOMS[:0] = [g + (m,) for g in WINO_LAYERS[-2:] for m in (2, 4)]


def wino_route(g):
    return "cus16" if tuple(g[3:5]) == (128, 128) else "default"


# ---- batch-norm fused into the F(4x4) transforms: (N, H, W, C, m, residual, addend) --------------------------------------------------------------
WINO_BN_GEOMS = [(1, 1, 1, 4, 4, False, False), (1, 5, 6, 8, 4, True, True), (2, 3, 7, 24, 4, False, True), (16, 5, 5, 64, 4, True, False),
                 (16, 6, 6, 4, 4, False, False), (1, 9, 13, 100, 4, True, True), (3, 4, 4, 260, 4, False, False), (2, 3, 3, 512, 4, True, True),
                 (1, 14, 2, 512, 4, False, True),
                 (2, 3, 3, 516, 4, True, True), (1, 4, 4, 516, 4, False, False), (1, 4, 4, 6, 4, False, True), (1, 5, 6, 8, 2, True, True),      # refused
                 (1, 5, 6, 8, 0, False, False), (1, 5, 6, 1024, 4, False, False)]


class gemm_route:
    """The HIFIHR_GEMM_* switches of one route, for the duration of a case (the library re-reads them on every call)."""

    def __init__(self, name):
        self.env = GEMM_ROUTES[name]

    def __enter__(self):
        self.saved = {k: _os.environ.pop(k, None) for k in GEMM_SWITCHES}
        _os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            _os.environ.pop(k, None)
            if v is not None:
                _os.environ[k] = v


# ------------------------------------------------------------------------------------------------
# The tail contract: the entries behind the network's heads -- Procrustes (csrc/eval.hip), the two data paths (csrc/augment.hip), Adam
# (csrc/adam.hip), texture PCA (csrc/texpca.hip), the fused losses (csrc/losses.hip), MANO / LBS (csrc/mano_lbs.hip, csrc/lbs.hip) -- on
# the lists of tests/test_hostsim_tail_contract.py (the GPU half: tests/test_gpu_tail.py, tests/test_gpu_mano.py), in the layer contract's
# form: refused with HIFIHR_EINVAL, nothing launched, nothing written -- or a float64 reference inside guard bands, a second call on the
# same buffers (identical bits where include/hifihr.h says deterministic), accumulate / overwrite as the header states them, every
# optional pointer NULL at least once.  Pixels, gathers, masks and integer outputs: bit for bit.
# ------------------------------------------------------------------------------------------------
TAIL_CONTRACT_ENTRIES = ("procrustes_error", "ho3d_batch", "freihand_augment", "freihand_batch", "freihand_batch_step", "adam_step", "adam_step_dyn",
                         "adam_step_counted", "texture_pca_fwd", "texture_pca_bwd", "geom_loss_fwd", "geom_loss_bwd", "joint_terms_fwd", "joint_terms_bwd",
                         "photo_loss_fwd", "photo_loss_bwd", "sil_post", "loss_total_fwd", "loss_total_bwd", "light_split_fwd", "light_split_bwd",
                         "mano_lbs_fwd", "mano_lbs_bwd", "mano_joints_fwd", "mano_joints_bwd", "mano_full_fwd", "mano_full_bwd", "lbs_fwd", "lbs_bwd")
# kind: (c, cap) as in LAYER_CONTRACT_C: c = 4 x the worst err / (sqrt(L) max|ref| + cond) of the float64 references run in float32 (plain fp32
# torch on the CPU) over the lists of tests/test_hostsim_tail_contract.py, printed by tools/layer_contract_c.py.  The older cases' tolerances
# are absolute or mixed, so they are applied as such (TAIL_LEGACY below, never exceeded); cap repeats their relative part where they have one.
TAIL_CONTRACT_C = {
    # kind: (c, cap)                   fp32 torch's worst ratio x 4; the quantities and L
    "adam_p": (1.7e-7, 1e-5),          # 4.22e-08 x 4   parameters after a step, L = 1                     (adam_case rtol 1e-5, with its 2e-6: adam_passes)
    "adam_m": (3.3e-7, 3.3e-7),        # 8.22e-08 x 4   exp_avg, L = 1                                     (no older case looks at the moments)
    "adam_v": (3.8e-7, 3.8e-7),        # 9.48e-08 x 4   exp_avg_sq, L = 1
    "tex_fwd": (1.7e-7, 1e-5),         # 4.18e-08 x 4   tex, L = K + 1                                     (texture_pca_case 1e-5)
    "tex_bwd": (1.7e-7, 2e-5),         # 4.04e-08 x 4   dcoef, L = n                                       (texture_pca_case 2e-5 max(1, sqrt(n / 4096)))
    "geom_out": (1.8e-7, 2e-5),        # 4.31e-08 x 4   each of the five terms, L = its element count      (geom_loss_case 2e-5)
    "geom_grad": (4.5e-7, 2e-5),       # 1.10e-07 x 4   gj / gshape / gpose (L = 1), gv (L = 1 + edges at the vertex)   (geom_loss_case 2e-5)
    "photo_out": (7.3e-8, 3e-5),       # 1.82e-08 x 4   texture, mrgb, sil, mean difference, L = B 3 H W (sil: B H W)   (photo_loss_case 3e-5)
    "photo_img": (1.5e-9, 1e-6),       # 3.72e-10 x 4   re_img_m, L = 1: exact wherever alpha > 0          (photo_loss_case 1e-6 absolute)
    "photo_grad": (4.3e-7, 2e-5),      # 1.07e-07 x 4   grad_rgba, L = 1                                   (photo_loss_case 2e-5)
    "joint_out": (8.8e-8, 2e-5),       # 2.19e-08 x 4   joint_2d, bone_direc, bone_direc_3d, L = their element counts   (joint_terms_case 2e-5)
    "joint_grad": (8.6e-7, 1e-5),      # 2.13e-07 x 4   g_j2d / g_joints per sample, L = 6 (the wrist's five bones and the base term)   (joint_terms_case 1e-5)
    "total": (7.2e-8, 1e-6),           # 1.79e-08 x 4   the sum of the selected terms, L = their number, cond = sum |term|   (loss_total_case 1e-6)
    "mano_v": (1.3e-6, 5e-5),          # 3.21e-07 x 4   verts / jtr / verts_cam, L = 16 joints' transforms  (mano_*_case 5e-6 absolute on ~0.1: TAIL_LEGACY)
    "mano_j": (2.3e-8, 2e-5),          # 5.55e-09 x 4   joints_rel / verts_rel / root, L = 778              (mano_joints_case 2e-6 absolute)
    "mano_g": (2.9e-7, 3e-4),          # 7.08e-08 x 4   gpose / gbeta, L = 778                              (mano_*_case 3e-4 of the largest gradient)
    "mano_gv": (9.2e-8, 2e-4),         # 2.29e-08 x 4   gverts of the regression, L = 22                    (mano_joints_case 2e-4 absolute)
    "lbs_v": (7.1e-7, 2e-5),           # 1.75e-07 x 4   verts / posed joints, L = J                         (lbs_case 2e-6 max(1, max|ref| / 0.1))
    "lbs_g": (1.4e-7, 2e-4),           # 3.36e-08 x 4   gtheta / gbeta / the scratch, L = V                 (lbs_case 2e-4)
}
TAIL_CONTRACT_KINDS = tuple(TAIL_CONTRACT_C)
LAYER_CONTRACT_C.update(TAIL_CONTRACT_C)
_CANARY[torch.int64] = -1234567890123
_POISON[torch.int64] = 0x7FFFFFFFFFFFFFF0
TAIL_LAUNCHED = set()                 # kernels the emulator launched under the tail cases (the coverage test reads it)


def _tail_drain(lib, device):
    """What the emulator launched since the last look (None on a GPU: the product library keeps no log)."""
    if device != "cpu":
        return None
    names = [k.replace(" ", "") for k in launch_log(lib)]
    TAIL_LAUNCHED.update(names)
    return names


def _tail_refuses(entry, lib, device, call, guards, what):
    """HIFIHR_EINVAL, every output and guard untouched, nothing launched."""
    _tail_drain(lib, device)
    _refuses(entry, call, guards, f"{entry}: {what}")
    left = _tail_drain(lib, device)
    assert not left, f"{entry}: {what}: refused but launched {left}"


def _raw(lib, name, *args):
    """The C entry itself (the wrappers of hifihr_amd._lib derive sizes from tensor shapes; refused sizes need them spelled out)."""
    lib.check(getattr(lib.c, name)(*args), name)


def _vp(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _tail_ratio(entry, err, bound):
    _layer_log(entry, True, (err / bound) if bound > 0 else (0.0 if err == 0 else float("inf")))


# ---- Procrustes (csrc/eval.hip) ------------------------------------------------------------------------------------------------------
# float64 inside, fp32 out: aligned within 2^-23 max|ref aligned| of the sample (twice the storage rounding), the per-point distances
# | aligned_n - gt_n | within the same (a distance moves by at most sqrt(3) x the largest component error, sqrt(3) 2^-24 < 2^-23), err_sum
# within 2^-23 ref + floor.  Floor: 4 x the largest difference, over the emulator list, between two float64 evaluations of the reference
# (numpy svd of M against the eigen route of M^T M completed by cross products; tools/layer_contract_c.py prints both figures): 7.28e-12,
# met on points of 1e3 units -- and, since such a difference grows with the size of the data, never more than 4 x the largest difference
# relative to N max|gt| (2.52e-16) times the sample's own N max|gt|: 1e-15 of the summed magnitudes for a hand in metres.
PROCRUSTES_FLOOR = 3.0e-11            # 7.28e-12 x 4
PROCRUSTES_FLOOR_REL = 1.1e-15        # 2.52e-16 x 4
PROCRUSTES_UNIQUE = 1e-12             # smallest / largest singular value of the reference below which R is not unique (include/hifihr.h)
PROCRUSTES_FAMILIES = ("generic", "similar", "reflect", "gt_planar", "gt_planar_fp32", "gt_thin_1e-2", "gt_thin_1e-4", "gt_thin_1e-6",
                       "gt_thin_1e-8", "gt_line", "gt_point", "pred_planar", "pred_line", "pred_point", "both_planar", "both_line_planar",
                       "both_point", "offset100", "extent1e-3", "extent1e3")


def procrustes_contract_expect(B, N):
    return B > 0 and N > 0


def procrustes_contract_inputs(family, B, N, seed):
    """(pred, gt) fp32 [B, N, 3]; points of 0.05 units (a hand in metres) unless the family says otherwise."""
    rng = np.random.default_rng(seed)
    ext = 0.05
    generic = lambda: rng.normal(0, ext, (B, N, 3))
    line = lambda: rng.integers(-50, 51, (B, N, 1)) / 256.0 * (np.array([1.0, 2.0, -1.0]) / 8)        # exact in fp32: exactly collinear
    point = lambda: np.broadcast_to(np.array([0.1, -0.2, 0.6]), (B, N, 3)).copy()

    def planar(t=0.0):
        x = generic()
        x[..., 2] = t * rng.normal(0, ext, (B, N))
        return x
    gt, pred = generic(), generic() + rng.normal(0, 0.1, (B, 1, 3))
    if family in ("similar", "reflect"):
        q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(B)])
        for b in range(B):
            if (np.linalg.det(q[b]) < 0) != (family == "reflect"):
                q[b, :, 0] *= -1
        pred = 1.7 * gt @ q.transpose(0, 2, 1) + rng.normal(0, 0.1, (B, 1, 3))
    elif family == "gt_planar":
        gt = planar()
    elif family == "gt_planar_fp32":                                     # one depth, stored in fp32: planar to an ulp
        z = np.float32(0.6)
        gt[..., 2] = np.stack([np.nextafter(z, np.float32(-1)), z, np.nextafter(z, np.float32(2))]).astype(np.float64)[rng.integers(0, 3, (B, N))]
    elif family.startswith("gt_thin_"):
        gt = planar(float(family[8:]))
    elif family == "gt_line":
        gt = line()
    elif family == "gt_point":
        gt = point()
    elif family == "pred_planar":
        pred = planar() + 0.3
    elif family == "pred_line":
        pred = line() + 0.25
    elif family == "pred_point":
        pred = point()
    elif family == "both_planar":
        gt, pred = planar(), 2.0 * planar() + 0.3
    elif family == "both_line_planar":
        gt, pred = line(), planar()
    elif family == "both_point":
        gt, pred = point(), point() * 0.5
    elif family == "offset100":
        gt, pred = gt + 100.0, pred + 100.0
    elif family.startswith("extent"):
        gt, pred = gt * float(family[6:]) / ext, pred * float(family[6:]) / ext
    else:
        assert family == "generic", family
    return torch.from_numpy(pred.astype(np.float32)), torch.from_numpy(gt.astype(np.float32))


def _polar_by_eigen(M):
    """The orthogonal polar factor and the singular values of a 3x3 M by the eigen route: V from M^T M, the two leading left vectors from
    M V, the missing direction(s) completed by cross products (float64 numpy; the second evaluation behind PROCRUSTES_FLOOR)."""
    lam, V = np.linalg.eigh(M.T @ M)
    V = V[:, ::-1]
    W = M @ V
    w = np.linalg.norm(W, axis=0)
    if not w[0] > 0:
        return np.eye(3), w
    u1 = W[:, 0] / w[0]
    if w[1] > 1e-14 * w[0]:
        u2 = W[:, 1] - (W[:, 1] @ u1) * u1
    else:
        u2 = np.eye(3)[int(np.abs(u1).argmin())]
        u2 = u2 - (u2 @ u1) * u1
    u2 = u2 / np.linalg.norm(u2)
    u3 = np.cross(u1, u2)
    if w[2] > 1e-14 * w[0] and w[1] > 1e-14 * w[0]:
        u3 = u3 if W[:, 2] @ u3 >= 0 else -u3
    return np.stack([u1, u2, u3], 1) @ V.T, w


def procrustes_contract_ref(pred, gt, route="svd", drop_point=None):
    """align_w_scale (reference utils/train_utils.py:267-290 around scipy.linalg.orthogonal_procrustes) restated in float64 numpy.
    -> aligned [B, N, 3], dist [B, N], err_sum [B], unique [B] (R is determined: the smallest singular value of M above 1e-12 of the
    largest).  drop_point: err_sum without that point's distance (the detection check)."""
    P, G = pred.double().numpy(), gt.double().numpy()
    aligned, unique = np.empty_like(P), np.empty(P.shape[0], bool)
    for b in range(P.shape[0]):
        t1, t2 = G[b].mean(0), P[b].mean(0)
        A, Bm = G[b] - t1, P[b] - t2
        s1 = np.linalg.norm(A) + 1e-8
        A = A / s1
        s2 = np.linalg.norm(Bm) + 1e-8
        Bm = Bm / s2
        M = A.T @ Bm                                                    # orthogonal_procrustes(A, Bm): u w vt = svd((Bm^T A)^T), R = u vt
        if route == "svd":
            u, w, vt = np.linalg.svd(M)
            R = u @ vt
        else:
            R, w = _polar_by_eigen(M)
        aligned[b] = (Bm @ R.T) * w.sum() * s1 + t1
        unique[b] = bool(w.max() > 0 and w.min() > PROCRUSTES_UNIQUE * w.max())
    dist = np.linalg.norm(aligned - G, axis=2)
    keep = np.ones(P.shape[1], bool)
    if drop_point is not None:
        keep[drop_point] = False
    return {"aligned": aligned, "dist": dist, "err_sum": dist[:, keep].sum(1), "unique": unique}


def procrustes_err_bound(ref_err, N, gt_max):
    return 2.0 ** -23 * float(ref_err) + min(PROCRUSTES_FLOOR, PROCRUSTES_FLOOR_REL * N * float(gt_max))


def procrustes_err_passes(got, ref_err, N, gt_max):
    return all(abs(float(g) - float(r)) <= procrustes_err_bound(r, N, m) for g, r, m in zip(got, ref_err, gt_max))


def procrustes_contract_case(lib, device, B, N, family, seed=0):
    from hifihr_amd._lib import _fp
    e, what = "procrustes_error", f"procrustes {(B, N, family)}"
    Bs, Ns = max(B, 1), max(N, 1)
    pred, gt = procrustes_contract_inputs(family, Bs, Ns, seed)
    G = Guards(device)
    p, g, al, err = G.inp(pred), G.inp(gt), G.out(Bs, Ns, 3), G.out(Bs)
    if not procrustes_contract_expect(B, N):
        _tail_refuses(e, lib, device, lambda: _raw(lib, "hifihr_procrustes_error", _fp(p), _fp(g), B, N, _fp(al), _fp(err), None), G, what)
        return False
    for k, args in enumerate(((None, g, err), (p, None, err), (p, g, None))):
        _tail_refuses(e, lib, device, lambda: _raw(lib, "hifihr_procrustes_error", _fp(args[0]), _fp(args[1]), B, N, _fp(al), _fp(args[2]), None),
                      G, f"{what} NULL argument {k}")
    ref = procrustes_contract_ref(pred, gt)
    lib.procrustes_error(p, g, al, err)
    G.intact(what)
    got_al, got_err = al.cpu().double().numpy(), err.cpu().double().numpy()
    assert np.isfinite(got_al).all() and np.isfinite(got_err).all(), f"{what}: not finite"
    for b in range(B):
        tol = 2.0 ** -23 * float(np.abs(ref["aligned"][b]).max())
        if ref["unique"][b]:
            d = float(np.abs(got_al[b] - ref["aligned"][b]).max())
            _tail_ratio(e, d, tol)
            assert d <= tol, f"{what} sample {b}: aligned off by {d:.3e}, bound {tol:.3e}"
        d = float(np.abs(np.linalg.norm(got_al[b] - gt[b].double().numpy(), axis=1) - ref["dist"][b]).max())
        _tail_ratio(e, d, tol)
        assert d <= tol, f"{what} sample {b}: per-point distances off by {d:.3e}, bound {tol:.3e}"
        d, bound = abs(got_err[b] - ref["err_sum"][b]), procrustes_err_bound(ref["err_sum"][b], N, gt[b].abs().max())
        _tail_ratio(e, d, bound)
        assert d <= bound, f"{what} sample {b}: err_sum {got_err[b]!r} vs {ref['err_sum'][b]!r}, bound {bound:.3e}"
    first = (al.clone(), err.clone())
    lib.procrustes_error(p, g, al, err)                                 # deterministic: the same bits again
    _layer_equal(e, al, first[0], f"{what}: aligned, second call")
    _layer_equal(e, err, first[1], f"{what}: err_sum, second call")
    err2 = G.out(B)
    lib.procrustes_error(p, g, None, err2)                              # aligned NULL: the same err_sum bits
    _layer_equal(e, err2, first[1], f"{what}: err_sum without aligned")
    G.intact(what)
    _tail_drain(lib, device)
    return True


# ---- HO-3D crop + resize (csrc/augment.hip) ------------------------------------------------------------------------------------------
HO3D_MAX_WINDOW = 800                 # HIFIHR_HO3D_MAX_WINDOW (include/hifihr.h)


def ho3d_contract_frames(n, FH, FW):
    """Frames and hand masks that make a dropped filter tap visible: a ramp, a one-pixel checker (every resampled value sits at 127.5, the
    mask's rounding threshold) crossed with coarse blocks, and isolated bright / dark pixels -- not noise, whose outermost taps average out."""
    y, x = np.mgrid[:FH, :FW]
    frames = np.zeros((n, FH, FW, 4), np.uint8)
    masks = np.zeros((n, FH, FW), np.uint8)
    for k in range(n):
        spots = ((x * 7 + y * 13 + k * 5) % 37 == 0)
        frames[k, :, :, 0] = (x + 3 * k) * 255 // max(FW + 3 * k - 1, 1)
        frames[k, :, :, 1] = (((x + y + k) & 1) ^ ((x // 9 + y // 5) & 1)) * 255
        frames[k, :, :, 2] = np.where(spots, 255, (y * 40 // max(FH, 1)))
        frames[k, :, :, 3] = 77                                          # the X byte must not reach an output
        masks[k] = ((((x + y + k) & 1) ^ ((x // 7 + y // 11) & 1)) ^ spots) * 255
    return frames, masks


def ho3d_contract_expect(FH, FW, out_size, boxes, mode="ok"):
    return mode == "ok" and len(boxes) > 0 and FH > 0 and FW > 0 and 0 < out_size <= 256


def ho3d_contract_ref(frames, masks, idx, boxes, out_size, max_taps=None):
    """Pillow's crop + resize (oracle/ho3d_oracle.py, no tap limit unless max_taps cuts the tables) per sample -> img u8 [B, S, S, 3],
    mask u8 [B, S, S]; a box that is empty, inverted or above HO3D_MAX_WINDOW on an edge: zeros (include/hifihr.h)."""
    from oracle import ho3d_oracle as ho
    S = out_size
    img, msk = np.zeros((len(boxes), S, S, 3), np.uint8), np.zeros((len(boxes), S, S), np.uint8)
    for b, (x0, y0, x1, y1) in enumerate(boxes):
        if x1 - x0 <= 0 or y1 - y0 <= 0 or max(x1 - x0, y1 - y0) > HO3D_MAX_WINDOW:
            continue
        img[b] = ho.pil_resize_u8(ho.pil_crop_u8(frames[idx[b], :, :, :3], (x0, y0, x1, y1)), S, S, "bilinear", max_taps)
        msk[b] = ho.pil_resize_u8(ho.pil_crop_u8(masks[idx[b]], (x0, y0, x1, y1)), S, S, "bicubic", max_taps)
    return img, msk


def ho3d_taps_needed(boxes, out_size):
    """The most taps any output element of the case takes, per filter: (bilinear, bicubic), counted on Pillow's own tables."""
    from oracle import ho3d_oracle as ho
    need = [0, 0]
    for x0, y0, x1, y1 in boxes:
        if min(x1 - x0, y1 - y0) <= 0 or max(x1 - x0, y1 - y0) > HO3D_MAX_WINDOW:
            continue
        for k, name in enumerate(("bilinear", "bicubic")):
            for edge in {x1 - x0, y1 - y0} - {out_size}:
                need[k] = max(need[k], int(ho.precompute_coeffs(edge, 0.0, float(edge), out_size, name)[1][:, 1].max()))
    return tuple(need)


def ho3d_pixels_match(got_img, got_mask, ref_img, ref_mask):
    """The comparator (the detection check feeds it a reference made with cut tables): u8 / 255 and round(u8 / 255), bit for bit."""
    want_i = torch.from_numpy(ref_img).permute(0, 3, 1, 2).float().div(255)
    want_m = torch.round(torch.from_numpy(ref_mask).float().div(255)).unsqueeze(1)
    return torch.equal(got_img.cpu(), want_i), torch.equal(got_mask.cpu(), want_m)


def ho3d_contract_case(lib, device, FH, FW, out_size, boxes, mode="ok", seed=0):
    """mode: "ok", or what is wrong with the call -- "short_ws", "no_<source>" (an output given without its source); B = len(boxes)."""
    from oracle import ho3d_oracle as ho
    e, what = "ho3d_batch", f"ho3d {(FH, FW, out_size, boxes, mode)}"
    rng = np.random.default_rng(seed)
    B, S, n = len(boxes), out_size, 3
    Bs, Ss = max(B, 1), min(max(S, 1), 256)
    frames, masks = ho3d_contract_frames(n, max(FH, 1), max(FW, 1))
    idx = [(2 * b + 1) % n for b in range(Bs)]                             # batch order != cache order
    bx = np.asarray(list(boxes) if B else [(0, 0, 4, 4)], np.int32).reshape(Bs, 4)
    center = rng.uniform(50, 400, (Bs, 2)).astype(np.float32)
    scale = rng.uniform(0.3, 5.0, Bs).astype(np.float32)
    packed = np.concatenate([np.asarray(idx, np.int32), bx.reshape(-1), np.concatenate([center, scale[:, None]], 1).reshape(-1).view(np.int32)])
    Ks = (np.tile(np.array([[600.0, 0, 320], [0, 610.0, 240], [0, 0, 1]], np.float32), (n, 1, 1)) + rng.normal(0, 1, (n, 3, 3))).astype(np.float32)
    uv, xyz = rng.uniform(0, 640, (n, 21, 2)).astype(np.float32), rng.normal(size=(n, 21, 3)).astype(np.float32)
    G = Guards(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    fr = G.inp(t(frames).view(torch.int32).reshape(n, max(FH, 1), max(FW, 1)))
    mk, Kd, uvd, xyzd, pk = G.inp(t(masks)), G.inp(t(Ks)), G.inp(t(uv)), G.inp(t(xyz)), G.inp(t(packed))
    nws = lib.ho3d_workspace_bytes(Bs, Ss)
    assert nws > 0 and nws % 4 == 0, what
    assert lib.ho3d_workspace_bytes(B, S) == (nws if B > 0 and 0 < S <= 256 else 0), f"{what}: hifihr_ho3d_workspace_bytes"
    ws = G.out(nws // 4, dtype=torch.int32)
    ws_guard = G.outs.pop()                                                  # scratch: "any contents", only its surroundings are watched
    out = lambda: {"img_crop": G.out(Bs, 3, Ss, Ss), "hand_mask_crop": G.out(Bs, 1, Ss, Ss), "K_crop": G.out(Bs, 3, 3), "uv21_crop": G.out(Bs, 21, 2),
                   "xyz21": G.out(Bs, 21, 3)}
    o = out()
    names = ("img_crop", "hand_mask_crop", "K_crop", "uv21_crop", "xyz21")

    def call(o, src=(fr, mk, Kd, uvd, xyzd), ws_bytes=nws, ws_t=ws, packed_t=pk):
        from hifihr_amd._lib import _fp, _ip
        import ctypes
        _raw(lib, "hifihr_ho3d_batch", _vp(src[0]), _vp(src[1]), _fp(src[2]), _fp(src[3]), _fp(src[4]), FH, FW, _ip(packed_t), B, S, _vp(ws_t),
             ctypes.c_size_t(ws_bytes), *[_fp(o.get(k)) for k in names], None)
    if not ho3d_contract_expect(FH, FW, S, boxes, mode):
        G.outs.append(ws_guard)                                               # a refused call leaves the scratch alone too
        if mode == "short_ws":
            _tail_refuses(e, lib, device, lambda: call(o, ws_bytes=nws - 4), G, what)
        elif mode.startswith("no_"):
            k = names.index(mode[3:])
            _tail_refuses(e, lib, device, lambda: call(o, src=tuple(None if i == k else s for i, s in enumerate((fr, mk, Kd, uvd, xyzd)))), G, what)
        elif mode == "no packed":
            _tail_refuses(e, lib, device, lambda: call(o, packed_t=None), G, what)
        elif mode == "no ws":
            _tail_refuses(e, lib, device, lambda: call(o, ws_t=None), G, what)
        else:
            _tail_refuses(e, lib, device, lambda: call(o), G, what)
        return False
    ref_img, ref_mask = ho3d_contract_ref(frames, masks, idx, boxes, S)
    call(o)
    G.intact(what)
    whole, lo, hi, canary = ws_guard
    assert bool((whole[:lo] == canary).all()) and bool((whole[hi:] == canary).all()), f"{what}: wrote outside the workspace"
    ok_i, ok_m = ho3d_pixels_match(o["img_crop"], o["hand_mask_crop"], ref_img, ref_mask)
    _layer_log(e, True, 0.0)
    assert ok_i, f"{what}: frame crop differs from Pillow in {int((o['img_crop'].cpu() != torch.from_numpy(ref_img).permute(0, 3, 1, 2).float().div(255)).sum())} values"
    assert ok_m, f"{what}: mask crop differs from Pillow in {int((o['hand_mask_crop'].cpu()[:, 0] != torch.round(torch.from_numpy(ref_mask).float().div(255))).sum())} pixels"
    for b in range(B):                                                       # the rules of ho3d_batch_case
        uvc, Kc = ho.crop_targets(uv[idx[b]], Ks[idx[b]], {"crop_center": center[b], "scale": scale[b]}, S)
        assert torch.equal(o["uv21_crop"][b].cpu(), torch.from_numpy(uvc)), f"{what}: uv21_crop {b}"
        np.testing.assert_allclose(o["K_crop"][b].cpu().numpy(), Kc, rtol=1e-6, atol=1e-4)
        assert torch.equal(o["xyz21"][b].cpu(), torch.from_numpy(xyz[idx[b]])), f"{what}: xyz21 {b}"
    first = {k: v.clone() for k, v in o.items()}
    call(o)                                                                  # again, on the scratch the first call left
    for k in names:
        _layer_equal(e, o[k], first[k], f"{what}: {k}, second call")
    for k in names:                                                          # each output NULL: the others are the same bits
        o2 = out()
        o2[k] = None
        call(o2)
        for k2 in names:
            if k2 != k:
                _layer_equal(e, o2[k2], first[k2], f"{what}: {k2} with {k} NULL")
    G.intact(what)
    _tail_drain(lib, device)
    return True


# ---- FreiHAND warp and batch assembly (csrc/augment.hip) -----------------------------------------------------------------------------
# name -> the six AFFINE coefficients (a b c; d e f) of Image.transform, output pixel -> input pixel, for an H x W image
FREIHAND_MAPS = {
    "identity": lambda H, W: (1.0, 0.0, 0.0, 0.0, 1.0, 0.0),
    "rotation": lambda H, W: (np.cos(0.5), -np.sin(0.5), W / 2 - np.cos(0.5) * W / 2 + np.sin(0.5) * H / 2,
                              np.sin(0.5), np.cos(0.5), H / 2 - np.sin(0.5) * W / 2 - np.cos(0.5) * H / 2),
    "flip": lambda H, W: (-1.0, 0.0, float(W), 0.0, 1.0, 0.0),
    "half": lambda H, W: (2.0, 0.0, 0.0, 0.0, 2.0, 0.0),                       # a 0.5x scale of the picture
    "triple": lambda H, W: (1 / 3, 0.0, 0.0, 0.0, 1 / 3, 0.0),                 # a 3x scale
    "away": lambda H, W: (1.0, 0.0, W + 5.0, 0.0, 1.0, 0.0),                   # a shift that leaves the image
    "subpixel": lambda H, W: (1.0, 0.0, -0.5, 0.0, 1.0, 0.0),
}


def pil_affine_fixed(coefs):
    """Pillow's six 16.16 integers of (a, b, c, d, e, f) (libImaging/Geometry.c affine_fixed; hifihr_amd.data.pil_affine_fixed_terms)."""
    import math
    a, b, c, d, e, f = (float(v) for v in coefs)
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(a), fix(b), fix(c + a * 0.5 + b * 0.5), fix(d), fix(e), fix(f + d * 0.5 + e * 0.5)]


def pil_affine_nearest_ref(src, idx, fixed):
    """Pillow's fixed-point nearest-neighbour walk from the six integers, restated in numpy: src [n, H, W(, C)] -> [B, H, W(, C)], zero fill."""
    H, W = src.shape[1:3]
    x, y = np.arange(W, dtype=np.int64)[None, :], np.arange(H, dtype=np.int64)[:, None]
    out = np.zeros((len(idx),) + src.shape[1:], src.dtype)
    for b, c in enumerate(np.asarray(fixed, np.int64)):
        xs, ys = c[2] + x * c[0] + y * c[1], c[5] + x * c[3] + y * c[4]
        assert max(int(np.abs(xs).max()), int(np.abs(ys).max())) < 2 ** 31, "the walk leaves 32-bit integers"
        xin, yin = xs >> 16, ys >> 16
        inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
        px = src[idx[b], yin.clip(0, H - 1), xin.clip(0, W - 1)]
        out[b] = np.where(inside.reshape(inside.shape + (1,) * (px.ndim - 2)), px, 0)
    return out


def freihand_contract_case(lib, device, H, W, J, V, seed=0):
    """hifihr_freihand_augment, _batch and _batch_step on every map of FREIHAND_MAPS at once (B = 7 samples gathered from a cache of 3)."""
    from hifihr_amd._lib import _fp, _ip
    what = f"freihand {(H, W, J, V)}"
    rng = np.random.default_rng(seed)
    n, B = 3, len(FREIHAND_MAPS)
    rgbx = rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)
    mk = rng.choice(np.array([0, 127, 128, 255], np.uint8), (n, H, W))                 # both sides of round(u8 / 255)
    idx = rng.integers(0, n, B).astype(np.int32)
    fixed = np.asarray([pil_affine_fixed(m(H, W)) for m in FREIHAND_MAPS.values()], np.int32)
    Ks = (np.tile(np.array([[400.0, 0, 112], [0, 410.0, 108], [0, 0, 1]], np.float32), (n, 1, 1)) + rng.normal(0, 1, (n, 3, 3))).astype(np.float32)
    joints = (rng.normal(0, 0.05, (n, J, 3)) + np.array([0, 0, 0.6])).astype(np.float32)
    verts = (rng.normal(0, 0.05, (n, V, 3)) + np.array([0, 0, 0.6])).astype(np.float32)
    scales = rng.random(n).astype(np.float32)
    ang = rng.uniform(-np.pi, np.pi, B)
    rmat = np.zeros((B, 3, 3), np.float32)
    rmat[:, 0, 0] = np.cos(ang); rmat[:, 0, 1] = -np.sin(ang); rmat[:, 1, 0] = np.sin(ang); rmat[:, 1, 1] = np.cos(ang); rmat[:, 2, 2] = 1
    post = (np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)) + rng.normal(0, 0.1, (B, 3, 3))).astype(np.float32)
    post[:, 2] = (0, 0, 1)
    packed = np.concatenate([idx, fixed.reshape(-1), post.reshape(-1).view(np.int32), rmat.reshape(-1).view(np.int32)])
    # references: pixels bit for bit; the small tensors in float64 under freihand_batch_case's tolerances
    want_img = torch.from_numpy(pil_affine_nearest_ref(rgbx[..., :3], idx, fixed)).permute(0, 3, 1, 2).float().div(255)
    want_m1 = torch.round(torch.from_numpy(pil_affine_nearest_ref(mk, idx, fixed)).float().div(255))
    want_mask = want_m1.unsqueeze(1).repeat(1, 3, 1, 1)
    il = idx.astype(np.int64)
    wK = post.astype(np.float64) @ Ks[il].astype(np.float64)
    rot = lambda pts: pts[il].astype(np.float64) @ rmat.astype(np.float64).transpose(0, 2, 1)
    wj, wv = rot(joints), rot(verts)
    uvw = wj @ wK.transpose(0, 2, 1)
    wj2d = uvw[..., :2] / uvw[..., 2:3]
    close = lambda a, b, tol=2e-6: a.numel() == 0 or float((a.cpu().double() - torch.from_numpy(np.ascontiguousarray(b))).abs().max()) <= tol * max(1.0, float(np.abs(b).max()))
    G = Guards(device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cache = G.inp(t(rgbx).view(torch.int32).reshape(n, H, W))
    mkd, Kd, jd, vd, sd, pk, idxd, fxd = (G.inp(t(a)) for a in (mk, Ks, joints, verts, scales, packed, idx, fixed))

    # ---- hifihr_freihand_augment ----
    e = "freihand_augment"
    aug = lambda img, m, ix, cf, b, h, w, oi, om: _raw(lib, "hifihr_freihand_augment", _vp(img), _vp(m), _ip(ix), _ip(cf), b, h, w, _fp(oi), _fp(om), None)
    oi, om = G.out(B, 3, H, W), G.out(B, 3, H, W)
    aug(cache, mkd, idxd, fxd, B, H, W, oi, om)
    _layer_equal(e, oi, want_img, f"{what}: {e} image")
    _layer_equal(e, om, want_mask, f"{what}: {e} mask")
    aug(cache, mkd, idxd, fxd, B, H, W, oi, om)
    _layer_equal(e, oi, want_img, f"{what}: {e} image, second call")
    oi2, om2 = G.out(B, 3, H, W, offset_floats=1), G.out(B, 3, H, W, offset_floats=1)          # off 16-byte alignment: the one-pixel kernel
    aug(cache, mkd, idxd, fxd, B, H, W, oi2, om2)
    _layer_equal(e, oi2, want_img, f"{what}: {e} image, unaligned")
    _layer_equal(e, om2, want_mask, f"{what}: {e} mask, unaligned")
    oi3, om3 = G.out(B, 3, H, W), G.out(B, 3, H, W)
    aug(cache, None, idxd, fxd, B, H, W, oi3, None)                                            # either output NULL, with its source
    aug(None, mkd, idxd, fxd, B, H, W, None, om3)
    _layer_equal(e, oi3, want_img, f"{what}: {e} image alone")
    _layer_equal(e, om3, want_mask, f"{what}: {e} mask alone")
    G.intact(what)
    for why, call in (("no output", lambda: aug(cache, mkd, idxd, fxd, B, H, W, None, None)),
                      ("image without its source", lambda: aug(None, mkd, idxd, fxd, B, H, W, oi, om)),
                      ("mask without its source", lambda: aug(cache, None, idxd, fxd, B, H, W, oi, om)),
                      ("idx NULL", lambda: aug(cache, mkd, None, fxd, B, H, W, oi, om)), ("coef NULL", lambda: aug(cache, mkd, idxd, None, B, H, W, oi, om)),
                      ("B = 0", lambda: aug(cache, mkd, idxd, fxd, 0, H, W, oi, om)), ("H = 0", lambda: aug(cache, mkd, idxd, fxd, B, 0, W, oi, om)),
                      ("H W = 2^24", lambda: aug(cache, mkd, idxd, fxd, B, 4096, 4096, oi, om))):
        _tail_refuses(e, lib, device, call, G, f"{what}: {why}")

    # ---- hifihr_freihand_batch ----
    e = "freihand_batch"
    names = ("imgs", "masks", "segms_gt", "Ks", "Ps", "joints", "verts", "j2d_gt", "scales", "idxs")
    mk_out = lambda: {"imgs": G.out(B, 3, H, W), "masks": G.out(B, 3, H, W), "segms_gt": G.out(B, H, W, dtype=torch.int64), "Ks": G.out(B, 3, 3),
                      "Ps": G.out(B, 3, 4), "joints": G.out(B, J, 3), "verts": G.out(B, V, 3), "j2d_gt": G.out(B, J, 2), "scales": G.out(B),
                      "idxs": G.out(B, dtype=torch.int64)}

    def batch(o, src=None, b=B, h=H, w=W, j=J, v=V, step=None, sx=None):
        s_ = dict(img=cache, mask=mkd, Ks=Kd, joints=jd, verts=vd, scales=sd, packed=pk)
        s_.update(src or {})
        head = [_vp(s_["img"]), _vp(s_["mask"]), _fp(s_["Ks"]), _fp(s_["joints"]), _fp(s_["verts"]), _fp(s_["scales"]), j, v, _ip(s_["packed"]), b, h, w]
        outs = [_fp(o.get("imgs")), _fp(o.get("masks")), _vp(o.get("segms_gt"))] + [_fp(o.get(k)) for k in names[3:9]] + [_vp(o.get("idxs"))]
        if step is None:
            _raw(lib, "hifihr_freihand_batch", *head, *outs, None)
        else:
            sx = sx or {}
            _raw(lib, "hifihr_freihand_batch_step", *head, *outs, int(step[0]), float(step[1]),
                 *[_fp(sx.get(k)) for k in ("root_xyz", "joints_rel", "verts_rel", "cam_ndc")], None)

    def check_batch(o, tag):
        for k, want in (("imgs", want_img), ("masks", want_mask), ("segms_gt", want_m1.long()), ("idxs", torch.from_numpy(il))):
            if o.get(k) is not None:
                _layer_equal(e, o[k], want, f"{what}: {tag} {k}")
        if o.get("scales") is not None:
            _layer_equal(e, o["scales"], torch.from_numpy(scales[il]), f"{what}: {tag} scales")
        assert o.get("Ks") is None or close(o["Ks"], wK), f"{what}: {tag} Ks"
        assert o.get("joints") is None or close(o["joints"], wj), f"{what}: {tag} joints"
        assert o.get("verts") is None or close(o["verts"], wv), f"{what}: {tag} verts"
        assert o.get("j2d_gt") is None or close(o["j2d_gt"], wj2d, 1e-5), f"{what}: {tag} j2d_gt"
        if o.get("Ps") is not None:
            assert close(o["Ps"][:, :, :3], wK) and float(o["Ps"][:, :, 3].abs().max()) == 0.0, f"{what}: {tag} Ps"
            assert o.get("Ks") is None or torch.equal(o["Ps"][:, :, :3], o["Ks"]), f"{what}: {tag} Ps != [Ks | 0]"
    o = mk_out()
    batch(o)
    check_batch(o, e)
    G.intact(what)
    first = {k: v.clone() for k, v in o.items()}
    batch(o)
    for k in names:
        _layer_equal(e, o[k], first[k], f"{what}: {e} {k}, second call")
    for k in names:                                                      # each output NULL: the others are the same bits
        o2 = mk_out()
        o2[k] = None
        batch(o2)
        for k2 in names:
            if k2 != k:
                _layer_equal(e, o2[k2], first[k2], f"{what}: {e} {k2} with {k} NULL")
    G.intact(what)
    refused = [("img NULL", dict(src={"img": None})), ("mask NULL", dict(src={"mask": None})), ("Ks NULL", dict(src={"Ks": None})),
               ("scales NULL", dict(src={"scales": None})), ("packed NULL", dict(src={"packed": None})), ("B = 0", dict(b=0)), ("W = 0", dict(w=0)),
               ("J < 0", dict(j=-1)), ("V < 0", dict(v=-1)), ("H W = 2^24", dict(h=4096, w=4096))]
    refused += [("joints NULL", dict(src={"joints": None}))] if J > 0 else []
    refused += [("verts NULL", dict(src={"verts": None}))] if V > 0 else []
    for why, kw in refused:
        _tail_refuses(e, lib, device, lambda: batch(o, **kw), G, f"{what}: {why}")

    # ---- hifihr_freihand_batch_step ----
    e = "freihand_batch_step"
    xnames = ("root_xyz", "joints_rel", "verts_rel", "cam_ndc")
    mk_x = lambda: {"root_xyz": G.out(B, 1, 3), "joints_rel": G.out(B, J, 3), "verts_rel": G.out(B, V, 3), "cam_ndc": G.out(B, 4)}
    size = float(max(H, W))
    for root_id in sorted({-1, 0, J - 1} & set(range(-1, J))):
        o3, x = mk_out(), mk_x()
        batch(o3, step=(root_id, size), sx=x)
        for k in names:
            _layer_equal(e, o3[k], first[k], f"{what}: {e} root {root_id} {k}")
        root = first["joints"][:, root_id:root_id + 1] if root_id >= 0 else torch.zeros(B, 1, 3, device=device)
        _layer_equal(e, x["root_xyz"], root, f"{what}: {e} root {root_id} root_xyz")
        _layer_equal(e, x["joints_rel"], first["joints"] - root, f"{what}: {e} root {root_id} joints_rel")
        _layer_equal(e, x["verts_rel"], first["verts"] - root, f"{what}: {e} root {root_id} verts_rel")
        K = first["Ks"].cpu().double()
        cam = torch.stack([-2 * K[:, 0, 0] / size, -2 * K[:, 1, 1] / size, 1 - 2 * K[:, 0, 2] / size, 1 - 2 * K[:, 1, 2] / size], 1)
        assert close(x["cam_ndc"], cam.numpy(), 1e-6), f"{what}: {e} cam_ndc"
        firstx = {k: v.clone() for k, v in x.items()}
        for k in xnames:
            x2 = mk_x()
            x2[k] = None
            batch(mk_out(), step=(root_id, size), sx=x2)
            for k2 in xnames:
                if k2 != k:
                    _layer_equal(e, x2[k2], firstx[k2], f"{what}: {e} {k2} with {k} NULL")
    G.intact(what)
    x = mk_x()
    for why, kw in (("root_id = J", dict(step=(J, size))), ("image_size 0", dict(step=(-1, 0.0))), ("image_size < 0", dict(step=(-1, -4.0))),
                    ("image_size NaN", dict(step=(-1, float("nan")))), ("H W = 2^24", dict(step=(-1, size), h=4096, w=4096)), ("B = 0", dict(step=(-1, size), b=0)),
                    ("mask NULL", dict(step=(-1, size), src={"mask": None}))):
        _tail_refuses(e, lib, device, lambda: batch(o, sx=x, **kw), G, f"{what}: {why}")
    _tail_drain(lib, device)
    return True


# ---- Adam (csrc/adam.hip) ------------------------------------------------------------------------------------------------------------
ADAM_BETAS, ADAM_EPS, ADAM_LR = (0.9, 0.999), 1e-8, 1e-3


def adam_contract_ref(p, g, m, v, step, wd, grad_scale, dt=torch.float64, drop=None):
    """One torch.optim.Adam step (coupled weight decay) in `dt`, the scalars of the update in float64 as the launcher forms them.
    drop: that element's gradient is left out (the detection check).  -> (p, m, v)"""
    b1, b2 = ADAM_BETAS
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    f = lambda x: torch.tensor(x, dtype=torch.float32).to(dt)                 # the entry takes its scalars as fp32
    gr = g * f(grad_scale) + f(wd) * p
    if drop is not None:
        gr[drop] = 0
    m = f(b1) * m + (1 - f(b1)) * gr
    v = f(b2) * v + (1 - f(b2)) * gr * gr
    b1d, b2d, lrd = (float(torch.tensor(x, dtype=torch.float32)) for x in (b1, b2, ADAM_LR))
    step_size, inv = lrd / (1 - b1d ** step), 1 / (1 - b2d ** step) ** 0.5
    if dt == torch.float32:
        step_size, inv = float(torch.tensor(step_size, dtype=dt)), float(torch.tensor(inv, dtype=dt))
    p = p - step_size * (m / (v.sqrt() * inv + f(ADAM_EPS)))
    return p, m, v


def adam_passes(kind, got, ref):
    """The comparator: layer_bound, and for the parameters never above adam_case's 2e-6 + 1e-5 |p| per element."""
    d = (got.detach().cpu().double() - ref).abs()
    if bool(torch.isnan(d).any()):
        return False, float("nan"), 0.0
    bound = torch.full_like(ref, layer_bound(kind, ref, 1))
    if kind == "adam_p":
        bound = torch.minimum(bound, 2e-6 + 1e-5 * ref.abs())
    worst = int((d / bound.clamp_min(1e-300)).argmax()) if d.numel() else 0
    return bool((d <= bound).all()), float(d.reshape(-1)[worst]) if d.numel() else 0.0, float(bound.reshape(-1)[worst]) if d.numel() else 0.0


def _adam_close(entry, kind, got, ref, what):
    ok, err, bound = adam_passes(kind, got, ref)
    _tail_ratio(entry, err, bound)
    assert ok, f"{what}: {kind} err {err:.3e} vs bound {bound:.3e}"


def adam_contract_inputs(n, seed, steps=3):
    gen = torch.Generator().manual_seed(seed)
    return {"p": torch.randn(n, generator=gen), "g": [torch.randn(n, generator=gen) for _ in range(steps)],
            "m": torch.randn(n, generator=gen) * 0.1, "v": torch.rand(n, generator=gen) * 0.01}


def adam_contract_case(lib, device, n, wd, grad_scale, seed=0):
    """hifihr_adam_step, _dyn and _counted on one trajectory: steps 1 - 3 from zero moments, a step at t = 1000 from given moments, an all-zero
    gradient on zero moments; every step against the float64 update continued from the entry's own previous fp32 state."""
    import struct
    from hifihr_amd._lib import _fp
    what = f"adam {(n, wd, grad_scale)}"
    b1, b2 = ADAM_BETAS
    inp = adam_contract_inputs(n, seed)
    G = Guards(device)
    zero = torch.zeros(n)

    def buffers(p, m, v, off=0):
        out = []
        for t in (p, m, v):
            b = G.out(n, offset_floats=off)
            b.copy_(t)
            out.append(b)
        return out

    def state_at(done_steps, off=0):
        st = G.out(48, dtype=torch.uint8, offset_floats=off)
        st.copy_(lib.adam_state_image(ADAM_LR, b1, b2, done_steps))
        return st

    def dyn_at(step):
        b1d, b2d, lrd = (float(torch.tensor(x, dtype=torch.float32)) for x in (b1, b2, ADAM_LR))
        return G.inp(torch.tensor([lrd / (1 - b1d ** step), 1.0 / (1 - b2d ** step) ** 0.5], dtype=torch.float32))

    def run(entry, bufs, g, step, st=None, count=n):
        p, m, v = bufs
        if entry == "adam_step":
            _raw(lib, "hifihr_adam_step", _fp(p), _fp(g), _fp(m), _fp(v), count, grad_scale, ADAM_LR, b1, b2, ADAM_EPS, wd, step, None)
        elif entry == "adam_step_dyn":
            dyn = dyn_at(step)                                           # (kept alive across the call)
            _raw(lib, "hifihr_adam_step_dyn", _fp(p), _fp(g), _fp(m), _fp(v), count, grad_scale, b1, b2, ADAM_EPS, wd, _fp(dyn), None)
        else:
            _raw(lib, "hifihr_adam_step_counted", _fp(p), _fp(g), _fp(m), _fp(v), count, grad_scale, ADAM_EPS, wd, _vp(st), None)

    def read_state(st):
        return struct.unpack("<dddddii", bytes(st.cpu().numpy().tobytes()))

    for entry in ("adam_step", "adam_step_dyn", "adam_step_counted"):
        # steps 1 - 3 from zero moments
        bufs, st = buffers(inp["p"], zero, zero), state_at(0)
        for s in (1, 2, 3):
            before = [b.cpu().clone() for b in bufs]
            gd = G.inp(inp["g"][s - 1])
            ref = adam_contract_ref(before[0], inp["g"][s - 1], before[1], before[2], s, wd, grad_scale)
            run(entry, bufs, gd, s, st)
            for kind, got, r in zip(("adam_p", "adam_m", "adam_v"), bufs, ref):
                _adam_close(entry, kind, got, r, f"{what}: {entry} step {s}")
            if s == 2:                                                  # deterministic: the same step from the same state, the same bits
                again, st2 = buffers(*before), state_at(1)
                run(entry, again, gd, s, st2)
                for a, b_ in zip(again, bufs):
                    _layer_equal(entry, a, b_, f"{what}: {entry} step 2 repeated")
        if entry == "adam_step_counted":
            lr_d, b1_d, b2_d, p1, p2, step_d, done_d = read_state(st)
            assert (lr_d, b1_d, b2_d, step_d, done_d) == (ADAM_LR, b1, b2, 3, 0), f"{what}: state {(lr_d, b1_d, b2_d, step_d, done_d)}"
            assert abs(p1 - b1 ** 3) <= 1e-14 and abs(p2 - b2 ** 3) <= 1e-14, f"{what}: running products"
        # a step at t = 1000 from given moments
        bufs, st = buffers(inp["p"], inp["m"], inp["v"]), state_at(999)
        ref = adam_contract_ref(inp["p"], inp["g"][0], inp["m"], inp["v"], 1000, wd, grad_scale)
        run(entry, bufs, G.inp(inp["g"][0]), 1000, st)
        for kind, got, r in zip(("adam_p", "adam_m", "adam_v"), bufs, ref):
            _adam_close(entry, kind, got, r, f"{what}: {entry} step 1000")
        if entry == "adam_step_counted":
            _, _, _, p1, p2, step_d, done_d = read_state(st)
            assert (step_d, done_d) == (1000, 0) and abs(p1 - b1 ** 1000) <= 1e-14 and abs(p2 - b2 ** 1000) <= 1e-14, f"{what}: state after step 1000"
        # an all-zero gradient on zero moments: 0 / (0 + eps) = 0
        bufs, st = buffers(inp["p"], zero, zero), state_at(0)
        run(entry, bufs, G.inp(zero), 1, st)
        if wd == 0:
            _layer_equal(entry, bufs[0], inp["p"], f"{what}: {entry} zero gradient, parameters")
            assert float(bufs[1].abs().max()) == 0.0 and float(bufs[2].abs().max()) == 0.0, f"{what}: {entry} zero gradient, moments"
        else:
            ref = adam_contract_ref(inp["p"], zero, zero, zero, 1, wd, grad_scale)
            for kind, got, r in zip(("adam_p", "adam_m", "adam_v"), bufs, ref):
                _adam_close(entry, kind, got, r, f"{what}: {entry} zero gradient")
        G.intact(what)
        # n = 0: accepted, not a step -- nothing launched, nothing written, the counter stays
        bufs, st, gd = buffers(inp["p"], inp["m"], inp["v"]), state_at(5), G.inp(inp["g"][0])
        before, st_before = [b.clone() for b in bufs], st.clone()
        _tail_drain(lib, device)
        run(entry, bufs, gd, 6, st, count=0)
        left = _tail_drain(lib, device)
        assert not left, f"{what}: {entry} with n = 0 launched {left}"
        assert all(torch.equal(a, b_) for a, b_ in zip(bufs, before)) and torch.equal(st, st_before), f"{what}: {entry} with n = 0 wrote"
        _layer_log(entry, True, 0.0)
        # refused: a NULL, a buffer one float off 16-byte alignment, the state off 8-byte alignment, step < 1
        for k in range(4):
            args = bufs[:1] + [gd] + bufs[1:]
            args[k] = None
            _tail_refuses(entry, lib, device, lambda: run(entry, (args[0], args[2], args[3]), args[1], 6, st), G, f"{what}: NULL buffer {k}")
            off = buffers(inp["p"], inp["m"], inp["v"], off=1)
            args = bufs[:1] + [gd] + bufs[1:]
            args[k] = off[0] if k != 1 else G.inp(inp["g"][0], offset_floats=1)
            _tail_refuses(entry, lib, device, lambda: run(entry, (args[0], args[2], args[3]), args[1], 6, st), G, f"{what}: buffer {k} off alignment")
        if entry == "adam_step":
            for bad in (0, -1):
                _tail_refuses(entry, lib, device, lambda: run(entry, bufs, gd, bad), G, f"{what}: step {bad}")
        elif entry == "adam_step_counted":
            _tail_refuses(entry, lib, device, lambda: run(entry, bufs, gd, 6, None), G, f"{what}: state NULL")
            st_off = state_at(5, off=4)
            _tail_refuses(entry, lib, device, lambda: run(entry, bufs, gd, 6, st_off), G, f"{what}: state off 8-byte alignment")
        else:
            _tail_refuses(entry, lib, device, lambda: _raw(lib, "hifihr_adam_step_dyn", _fp(bufs[0]), _fp(gd), _fp(bufs[1]), _fp(bufs[2]), n, grad_scale,
                                                           b1, b2, ADAM_EPS, wd, None, None), G, f"{what}: dyn NULL")
    _tail_drain(lib, device)
    return True


# ---- bounds of the float families ------------------------------------------------------------------------------------------------------
# kind -> the absolute tolerance the family's older case in this file gives a quantity `ref` of reduction length L (never exceeded)
TAIL_LEGACY = {
    "tex_fwd": lambda ref, L: 1e-5 * max(1.0, float(ref.abs().max())),                               # texture_pca_case
    "tex_bwd": lambda ref, L: 2e-5 * float(ref.abs().max()) * max(1.0, (L / 4096) ** 0.5),           # texture_pca_case (L = n)
    "geom_out": lambda ref, L: 2e-5 * float(ref.abs().max()) + 1e-7,                                 # geom_loss_case, per term
    "geom_grad": lambda ref, L: 2e-5 * float(ref.abs().max()) + 1e-9,
    "photo_out": lambda ref, L: 3e-5 * float(ref.abs().max()) + 1e-9,                                # photo_loss_case, per term
    "photo_img": lambda ref, L: 1e-6,
    "photo_grad": lambda ref, L: 2e-5 * float(ref.abs().max()) + 1e-12,
    "joint_out": lambda ref, L: 2e-5 * max(1.0, float(ref.abs().max())),                             # joint_terms_case, per term
    "joint_grad": lambda ref, L: 1e-5 * float(ref.abs().max()) + 1e-9,
    "total": lambda ref, L: 1e-6 * max(1.0, float(ref.abs().max())),                                 # loss_total_case
}


def tail_bound(kind, ref, L, cond=0.0):
    """layer_bound, never above the older case's tolerance for the same quantity; c cond on top (what a prefilled accumulator or a
    cancellation inside the operation costs: layer_bound's docstring)."""
    b = layer_bound(kind, ref, L)
    if kind in TAIL_LEGACY and ref.numel():
        b = min(b, TAIL_LEGACY[kind](ref, L))
    return b + LAYER_CONTRACT_C[kind][0] * float(cond)


def tail_passes(kind, got, ref, L, cond=0.0):
    return layer_err(got, ref) <= tail_bound(kind, ref, L, cond)


def _tail_close(entry, kind, got, ref, L, what, cond=0.0):
    err, bound = layer_err(got, ref), tail_bound(kind, ref, L, cond)
    _tail_ratio(entry, err, bound)
    assert err <= bound, f"{what}: err {err:.3e} vs bound {bound:.3e} (kind {kind}, max|ref| {float(ref.abs().max()) if ref.numel() else 0:.3e}, L {L})"


# ---- texture PCA (csrc/texpca.hip) -----------------------------------------------------------------------------------------------------
def texpca_contract_expect(B, K, n):
    return B > 0 and 1 <= K <= 32 and n >= 4 and n % 4 == 0


def texpca_contract_inputs(B, K, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return {"coef": torch.randn(B, K, generator=gen), "basis": torch.randn(K, n, generator=gen) * 0.1, "mean": torch.rand(n, generator=gen),
            "g": torch.randn(B, n, generator=gen), "prefill": torch.randn(B, K, generator=gen)}


def texpca_contract_ref(inp, with_mean, dt=torch.float64, drop_row=None):
    """tex = mean + coef basis (L = K + 1), dcoef = g basis^T (L = n); drop_row: tex without that basis row."""
    coef, basis, g = inp["coef"].to(dt), inp["basis"].to(dt), inp["g"].to(dt)
    if drop_row is not None:
        basis = basis.clone()
        basis[drop_row] = 0
    tex = coef @ basis + (inp["mean"].to(dt) if with_mean else 0.0)
    return {"tex": ("tex_fwd", coef.shape[1] + 1, tex), "dcoef": ("tex_bwd", basis.shape[1], g @ inp["basis"].to(dt).t())}


def texpca_contract_case(lib, device, B, K, n, with_mean=True, seed=0):
    from hifihr_amd._lib import _fp
    import ctypes
    what = f"texpca {(B, K, n, with_mean)}"
    Bs, Ks, ns = max(B, 1), min(max(K, 1), 33), max(n, 4)
    inp = texpca_contract_inputs(Bs, Ks, ns, seed)
    G = Guards(device)
    coef, basis, mean, g = G.inp(inp["coef"]), G.inp(inp["basis"]), G.inp(inp["mean"]), G.inp(inp["g"])
    tex, dcoef = G.out(Bs, ns), G.out(Bs, Ks)
    fwd = lambda c=coef, bs=basis, m=mean, o=tex: _raw(lib, "hifihr_texture_pca_fwd", _fp(c), _fp(bs), _fp(m), B, K, ctypes.c_long(n), _fp(o), None)
    bwd = lambda gg=g, bs=basis, o=dcoef: _raw(lib, "hifihr_texture_pca_bwd", _fp(gg), _fp(bs), B, K, ctypes.c_long(n), _fp(o), None)
    if not texpca_contract_expect(B, K, n):
        _tail_refuses("texture_pca_fwd", lib, device, fwd, G, what)
        _tail_refuses("texture_pca_bwd", lib, device, bwd, G, what)
        return False
    ref = texpca_contract_ref(inp, with_mean)
    fwd(m=mean if with_mean else None)
    _close_tail = lambda e, name, got, tag, cond=0.0: _tail_close(e, ref[name][0], got, ref[name][2], ref[name][1], f"{what}: {e} {name} {tag}", cond)
    _close_tail("texture_pca_fwd", "tex", tex, "")
    first = tex.clone()
    fwd(m=mean if with_mean else None)
    _layer_equal("texture_pca_fwd", tex, first, f"{what}: tex, second call")                  # (no atomics in the forward)
    dcoef.copy_(inp["prefill"])                                                               # "+=": onto what the buffer holds
    bwd()
    pre = float(inp["prefill"].abs().max())
    _tail_close("texture_pca_bwd", "tex_bwd", dcoef.cpu().double() - inp["prefill"].double(), ref["dcoef"][2], n, f"{what}: dcoef onto a prefill", pre)
    bwd()                                                                                     # float atomics: the second sum inside the bound
    _tail_close("texture_pca_bwd", "tex_bwd", (dcoef.cpu().double() - inp["prefill"].double()) / 2, ref["dcoef"][2], n, f"{what}: dcoef, second call", pre)
    dcoef.zero_()
    bwd()
    _close_tail("texture_pca_bwd", "dcoef", dcoef, "from zero")
    G.intact(what)
    for k, call in enumerate((lambda: fwd(c=None), lambda: fwd(bs=None), lambda: fwd(o=None))):
        _tail_refuses("texture_pca_fwd", lib, device, call, G, f"{what}: NULL argument {k}")
    for k, call in enumerate((lambda: bwd(gg=None), lambda: bwd(bs=None), lambda: bwd(o=None))):
        _tail_refuses("texture_pca_bwd", lib, device, call, G, f"{what}: NULL argument {k}")
    _tail_drain(lib, device)
    return True


# ---- the small entries: loss total, light split (csrc/losses.hip) --------------------------------------------------------------------
def loss_total_contract_case(lib, device, counts, lengths=None, mode="ok", seed=0):
    """counts: leading entries summed per part (len = nparts); lengths: the vectors' full lengths (default 64)."""
    from hifihr_amd._lib import _fp, _c_float_p
    import ctypes
    nparts = len(counts)
    lengths = list(lengths) if lengths is not None else [64] * nparts
    what = f"loss_total {(tuple(counts), tuple(lengths), mode)}"
    gen = torch.Generator().manual_seed(seed)
    G = Guards(device)
    alloc = [max(l, c, 1) for l, c in zip(lengths, counts)] or [1]
    parts = [G.inp(torch.randn(a, generator=gen)) for a in alloc]
    grads = [G.out(a, fill=9.0) for a in alloc]
    total, gt = G.out(1), G.inp(torch.tensor([1.75]))
    arr = lambda ts: (_c_float_p * max(len(ts), 1))(*[_fp(t) for t in ts])
    ints = lambda v: (ctypes.c_int * max(len(v), 1))(*[int(x) for x in v])
    fwd = lambda ps=parts, tot=total, np_=nparts: _raw(lib, "hifihr_loss_total_fwd", arr(ps), ints(counts), np_, _fp(tot), None)
    bwd = lambda gs=grads, g=gt, np_=nparts: _raw(lib, "hifihr_loss_total_bwd", _fp(g), arr(gs), ints(counts), ints(lengths), np_, None)
    ok_f = 1 <= nparts <= 4 and all(0 <= c <= 64 for c in counts)
    ok_b = ok_f and all(c <= l <= 64 for c, l in zip(counts, lengths))
    if mode != "ok" or not ok_f:
        _tail_refuses("loss_total_fwd", lib, device, (lambda: fwd(ps=[None] + parts[1:])) if mode == "null" else (lambda: fwd(tot=None)) if mode == "null_total" else fwd, G, what)
    else:
        fwd()
        want = torch.tensor([sum(float(p[:c].double().sum()) for p, c in zip(parts, counts))], dtype=torch.float64)
        _tail_close("loss_total_fwd", "total", total, want, sum(counts), f"{what}: total",
                    sum(float(p[:c].abs().sum()) for p, c in zip(parts, counts)))                      # (a sum of signed terms)
        if sum(counts) == 1:
            _layer_equal("loss_total_fwd", total, [p for p, c in zip(parts, counts) if c][0][:1], f"{what}: a single term")
        first = total.clone()
        fwd()
        _layer_equal("loss_total_fwd", total, first, f"{what}: second call")
    if mode != "ok" or not ok_b:
        _tail_refuses("loss_total_bwd", lib, device, (lambda: bwd(gs=[None] + grads[1:])) if mode == "null" else (lambda: bwd(g=None)) if mode == "null_total" else bwd, G, what)
    else:
        bwd()
        for gr, c, l in zip(grads, counts, lengths):
            want = torch.cat([torch.full((c,), 1.75), torch.zeros(l - c), torch.full((gr.numel() - l,), 9.0)])
            _layer_equal("loss_total_bwd", gr, want, f"{what}: gradient")
    G.intact(what)
    _tail_drain(lib, device)
    return mode == "ok" and ok_b


def light_split_contract_case(lib, device, B, seed=0):
    """hifihr_light_split_fwd / _bwd inside guards: light_split_case's bit-exact rules (clamp ends, a NaN colour, each gradient NULL)."""
    from hifihr_amd._lib import _fp
    what = f"light_split {B}"
    Bs = max(B, 1)
    gen = torch.Generator().manual_seed(seed)
    l = torch.randn(Bs, 6, generator=gen) * 1.5
    l[0, 0] = 1.0; l[min(1, Bs - 1), 1] = -1.0
    l[Bs - 1, 2] = float("nan")
    gc, gd = torch.randn(Bs, 3, generator=gen), torch.randn(Bs, 3, generator=gen)
    lr = l.clone().requires_grad_(True)
    c, dd = torch.nn.functional.hardtanh(lr[:, :3]), lr[:, 3:]
    ((c * gc).sum() + (dd * gd).sum()).backward()
    G = Guards(device)
    ld, gcd, gdd = G.inp(l), G.inp(gc), G.inp(gd)
    oc, od, gl = G.out(Bs, 3), G.out(Bs, 3), G.out(Bs, 6)
    fwd = lambda a=ld, b=oc, c_=od: _raw(lib, "hifihr_light_split_fwd", _fp(a), B, _fp(b), _fp(c_), None)
    bwd = lambda a=ld, b=gcd, c_=gdd, o=gl: _raw(lib, "hifihr_light_split_bwd", _fp(a), _fp(b), _fp(c_), B, _fp(o), None)
    if B <= 0:
        _tail_refuses("light_split_fwd", lib, device, fwd, G, what)
        _tail_refuses("light_split_bwd", lib, device, bwd, G, what)
        return False
    # (the refused calls first: the forward's NaN colour would make every later bit comparison of its buffer fail)
    for k, call in enumerate((lambda: fwd(a=None), lambda: fwd(b=None), lambda: fwd(c_=None))):
        _tail_refuses("light_split_fwd", lib, device, call, G, f"{what}: NULL argument {k}")
    for k, call in enumerate((lambda: bwd(a=None), lambda: bwd(o=None))):
        _tail_refuses("light_split_bwd", lib, device, call, G, f"{what}: NULL argument {k}")
    same = lambda a, b: bool(((a.cpu() == b) | (a.cpu().isnan() & b.isnan())).all())
    fwd()
    _layer_log("light_split_fwd", True)
    assert same(oc, c.detach()) and bool(oc.cpu()[B - 1, 2].isnan()) and torch.equal(od.cpu(), dd.detach().contiguous()), f"{what}: forward"
    bwd()
    _layer_log("light_split_bwd", True)
    assert same(gl, lr.grad) and float(gl.cpu()[B - 1, 2]) == float(gc[B - 1, 2]), f"{what}: backward"
    bwd(b=None)
    assert float(gl.cpu()[:, :3].abs().max()) == 0.0 and torch.equal(gl.cpu()[:, 3:], gd), f"{what}: gcolors NULL"
    bwd(c_=None)
    assert float(gl.cpu()[:, 3:].abs().max()) == 0.0 and same(gl[:, :3], lr.grad[:, :3]), f"{what}: gdirections NULL"
    G.intact(what)
    _tail_drain(lib, device)
    return True


# ---- photometric terms (csrc/losses.hip) -----------------------------------------------------------------------------------------------
PHOTO_LAMBDAS = (0.005, 0.005, 0.1)               # l_tex, l_mrgb, l_sil


def photo_contract_expect(B, H, W):
    return B > 0 and H > 0 and W > 0 and (H * W) % 4 == 0


def photo_contract_inputs(B, H, W, seg_kind, seed, nan_alpha=False):
    """alpha > 0, = 0 and < 0 inside every image; seg in {0, 1} or, seg_kind "ints", in 0 .. 3."""
    gen = torch.Generator().manual_seed(seed)
    rgba = torch.rand(B, 4, H, W, generator=gen)
    cls = torch.arange(B * H * W).reshape(B, H, W) % 3
    cls = cls.reshape(B, -1)[:, torch.randperm(H * W, generator=gen)].reshape(B, H, W) if H * W > 3 else cls
    rgba[:, 3] = torch.where(cls == 0, rgba[:, 3], torch.where(cls == 1, torch.zeros(B, H, W), -rgba[:, 3] - 0.1))
    if nan_alpha:
        rgba[B - 1, 3, H - 1, W - 1] = float("nan")
    imgs = torch.rand(B, 3, H, W, generator=gen)
    seg = torch.randint(0, 4 if seg_kind == "ints" else 2, (B, H, W), generator=gen)
    return {"rgba": rgba, "imgs": imgs, "seg": seg, "g_re": torch.randn(B, 3, H, W, generator=gen) * 1e-6, "gout": torch.tensor([0.8, 1.7, 0.0, 0.0])}


def photo_contract_ref(inp, dt=torch.float64, drop_quad=False):
    """losses.py:355-378 + the `sil` term.  drop_quad: the sums without the last four pixels of the last image."""
    rgba, imgs, seg = inp["rgba"].to(dt), inp["imgs"].to(dt), inp["seg"].to(dt)
    B, _, H, W = rgba.shape
    al = rgba[:, 3:4]
    re_sil = torch.where(al > 0, torch.full_like(al, 255.0), al)
    re_m = rgba[:, :3] * (re_sil / 255.0)
    mk = seg.unsqueeze(1) * imgs
    keep = torch.ones(B, 1, H * W, dtype=dt)
    if drop_quad:
        keep[B - 1, 0, -4:] = 0
    keep = keep.reshape(B, 1, H, W)
    n3, n1 = B * 3 * H * W, B * H * W
    l_tex, l_mrgb, l_sil = (float(torch.tensor(v, dtype=torch.float32)) for v in PHOTO_LAMBDAS)
    sr, sm = (re_m * keep).sum(), (mk * keep).sum()
    dm = sr / n3 - sm / n3
    cancel = float(sr.abs() + sm.abs()) / n3
    return {"re_m": ("photo_img", 1, re_m), "mk": mk,
            "tex": ("photo_out", n3, (l_tex * ((re_m - mk).abs() * keep).sum() / n3).reshape(1)),
            "mrgb": ("photo_out", n3, (l_mrgb * dm * dm).reshape(1), l_mrgb * 2 * abs(float(dm)) * cancel),
            "sil": ("photo_out", n1, (l_sil * ((re_sil - seg.unsqueeze(1)).abs() * keep).sum() / n1).reshape(1)),
            "dm": ("photo_out", n3, dm.reshape(1), cancel), "re_sil": re_sil}


def photo_contract_bwd_ref(inp, re_m, mk, fwd_out, with_g, with_gout, dt=torch.float64, drop_quad=False):
    """grad_rgba from the entry's own forward tensors (re_m, mask_rgbs, out[3]), as the entry reads them."""
    rgba = inp["rgba"].to(dt)
    B, _, H, W = rgba.shape
    n3 = B * 3 * H * W
    l_tex, l_mrgb, _ = (float(torch.tensor(v, dtype=torch.float32)) for v in PHOTO_LAMBDAS)
    al = rgba[:, 3:4]
    sc = torch.where(al > 0, torch.ones_like(al), al / 255.0)
    gout = inp["gout"].to(dt) if with_gout else torch.zeros(4, dtype=dt)
    kt, km = gout[0] * l_tex / n3, gout[1] * l_mrgb * 2 * fwd_out.to(dt)[3] / n3
    g = (inp["g_re"].to(dt) if with_g else 0.0) + kt * torch.sign(re_m.to(dt) - mk.to(dt)) + km
    if drop_quad:
        g = g.clone()
        g.reshape(B, 3, -1)[B - 1, :, -4:] = 0
    return ("photo_grad", 1, torch.cat([g * sc, torch.zeros_like(al)], 1))


def photo_contract_case(lib, device, B, H, W, seg_kind="binary", seed=0):
    from hifihr_amd._lib import _fp
    what = f"photo {(B, H, W, seg_kind)}"
    Bs, Hs, Ws = max(B, 1), max(H, 1), max(W, 1)
    if (Hs * Ws) % 4:
        Hs, Ws = Hs, Ws + (4 - Ws % 4) if Hs % 2 else Ws + Ws % 2
    nan_case = seg_kind == "nan"
    inp = photo_contract_inputs(Bs, Hs, Ws, seg_kind, seed, nan_alpha=nan_case)
    G = Guards(device)
    rd, idd, sd, gre, gout = G.inp(inp["rgba"]), G.inp(inp["imgs"]), G.inp(inp["seg"]), G.inp(inp["g_re"]), G.inp(inp["gout"])
    npart = lib.photo_loss_partial_floats()
    assert npart > 0
    re_m, mk, out, grad = G.out(Bs, 3, Hs, Ws), G.out(Bs, 3, Hs, Ws), G.out(4), G.out(Bs, 4, Hs, Ws)
    partial = G.out(npart)
    scratch = G.outs.pop()                                                # scratch: only its surroundings are watched
    rs, mrgbs = G.out(Bs, 1, Hs, Ws), G.out(Bs, 3, Hs, Ws)
    l = PHOTO_LAMBDAS
    fwd = lambda a=rd, b=idd, c=sd, o1=re_m, o2=mk, p=partial, o=out: _raw(lib, "hifihr_photo_loss_fwd", _fp(a), _fp(b), _vp(c), B, H, W, l[0], l[1], l[2],
                                                                            _fp(o1), _fp(o2), _fp(p), _fp(o), None)
    bwd = lambda a=rd, r=re_m, m=mk, g=gre, go=gout, fo=out, o=grad: _raw(lib, "hifihr_photo_loss_bwd", _fp(a), _fp(r), _fp(m), _fp(g), _fp(go), _fp(fo),
                                                                           B, H, W, l[0], l[1], _fp(o), None)
    post = lambda a=rd, b=idd, o1=rs, o2=mrgbs: _raw(lib, "hifihr_sil_post", _fp(a), _fp(b), B, H, W, _fp(o1), _fp(o2), None)
    if not photo_contract_expect(B, H, W):
        G.outs.append(scratch)
        _tail_refuses("photo_loss_fwd", lib, device, fwd, G, what)
        _tail_refuses("photo_loss_bwd", lib, device, bwd, G, what)
        _tail_refuses("sil_post", lib, device, post, G, what)
        return False
    # refused calls first (NaN outputs of the NaN case would defeat the bit comparison of the buffers afterwards)
    G.outs.append(scratch)
    for k, call in enumerate((lambda: fwd(a=None), lambda: fwd(b=None), lambda: fwd(c=None), lambda: fwd(o1=None), lambda: fwd(o2=None),
                              lambda: fwd(p=None), lambda: fwd(o=None))):
        _tail_refuses("photo_loss_fwd", lib, device, call, G, f"{what}: NULL argument {k}")
    for k, call in enumerate((lambda: bwd(a=None), lambda: bwd(r=None), lambda: bwd(m=None), lambda: bwd(fo=None), lambda: bwd(o=None))):
        _tail_refuses("photo_loss_bwd", lib, device, call, G, f"{what}: NULL argument {k}")
    for k, call in enumerate((lambda: post(a=None), lambda: post(o1=None), lambda: post(b=None))):
        _tail_refuses("sil_post", lib, device, call, G, f"{what}: NULL argument {k}")
    G.outs.pop()
    ref = photo_contract_ref(inp)
    fwd()
    e = "photo_loss_fwd"
    nanpix = torch.zeros(Bs, 1, Hs, Ws, dtype=torch.bool)
    if nan_case:                                                          # pinned: NaN alpha -> NaN re_img_m at that pixel, NaN in all four terms
        nanpix[B - 1, 0, H - 1, W - 1] = True
        assert bool(re_m.cpu().isnan().eq(nanpix.expand(-1, 3, -1, -1)).all()), f"{what}: NaN alpha must reach re_img_m at its pixel only"
        assert bool(out.cpu().isnan().all()), f"{what}: NaN alpha must reach every term, got {out.cpu()}"
        _layer_log(e, True)
    else:
        _tail_close(e, "photo_img", re_m, ref["re_m"][2], 1, f"{what}: re_img_m")
        for k, name in enumerate(("tex", "mrgb", "sil", "dm")):
            q = ref[name]
            _tail_close(e, q[0], out[k:k + 1], q[2], q[1], f"{what}: out[{k}] ({name})", q[3] if len(q) > 3 else 0.0)
    _layer_equal(e, mk, ref["mk"].float(), f"{what}: mask_rgbs")
    first = (re_m.clone(), mk.clone(), out.clone())
    fwd()                                                                 # deterministic (fixed summation order)
    same = lambda a, b: bool(((a == b) | (a.isnan() & b.isnan())).all())
    assert same(re_m, first[0]) and same(mk, first[1]) and same(out, first[2]), f"{what}: forward, second call"
    e = "photo_loss_bwd"
    for with_g, with_gout in ((True, True), (False, True), (True, False)):
        grad.fill_(7.0)                                                   # overwritten, not accumulated
        bwd(g=gre if with_g else None, go=gout if with_gout else None)
        gc = grad.cpu()
        assert float(gc[:, 3].abs().max()) == 0.0, f"{what}: the alpha channel of the gradient must be exact zeros"
        if nan_case:                                                      # pinned: out[3] is NaN, so is every rgb gradient (0 x NaN with gout NULL)
            assert bool(gc[:, :3].isnan().all()), f"{what}: NaN alpha, rgb gradient"
            _layer_log(e, True)
            continue
        q = photo_contract_bwd_ref(inp, first[0].cpu(), first[1].cpu(), first[2].cpu(), with_g, with_gout)
        _tail_close(e, q[0], grad, q[2], q[1], f"{what}: grad_rgba (g_re_img {with_g}, gout {with_gout})")
        if with_g and with_gout:
            g1 = grad.clone()
            bwd()
            _layer_equal(e, grad, g1, f"{what}: backward, second call")
    e = "sil_post"
    post()
    want_sil = ref["re_sil"].float()
    assert same(rs.cpu(), want_sil) and bool(rs.cpu().isnan().eq(nanpix).all()), f"{what}: re_sil"
    _layer_equal(e, mrgbs, (inp["imgs"] * (inp["rgba"][:, 3:4] > 0).float()), f"{what}: maskRGBs")
    rs2 = G.out(Bs, 1, Hs, Ws)
    post(b=None, o1=rs2, o2=None)                                         # mask_rgbs NULL (imgs not needed then)
    assert same(rs2.cpu(), want_sil), f"{what}: re_sil with mask_rgbs NULL"
    _layer_log(e, True)
    G.intact(what)
    whole, lo, hi, canary = scratch
    assert bool((whole[:lo] == canary).all()) and bool((whole[hi:] == canary).all()), f"{what}: wrote outside the partial sums"
    _tail_drain(lib, device)
    return True


# ---- joint terms (csrc/losses.hip) -----------------------------------------------------------------------------------------------------
JOINT_LAMBDAS = (0.7, 1.3, 2.1)
_BONE_PARENT = [0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
_BONE_CHILD = list(range(1, 21))


def joint_contract_expect(B, J, use2, use3):
    return B > 0 and J == 21 and (use2 or use3)


def joint_contract_inputs(B, special, seed, J=21):
    gen = torch.Generator().manual_seed(seed)
    j2d, j2d_gt = torch.rand(B, J, 2, generator=gen) * 224, torch.rand(B, J, 2, generator=gen) * 224
    j3d, j3d_gt = torch.randn(B, J, 3, generator=gen) * 0.05, torch.randn(B, J, 3, generator=gen) * 0.05
    if special == "identical":
        j2d, j3d = j2d_gt.clone(), j3d_gt.clone()
    elif special == "zero_bones" and J == 21:                             # sample 0: bone 3 (3 -> 4) of zero length in pred, bone 7 (7 -> 8) in gt
        j2d[0, 4], j3d[0, 4] = j2d[0, 3], j3d[0, 3]
        j2d_gt[0, 8], j3d_gt[0, 8] = j2d_gt[0, 7], j3d_gt[0, 7]
    return {"j2d": j2d, "j2d_gt": j2d_gt, "j3d": j3d, "j3d_gt": j3d_gt, "gout": torch.tensor([0.9, -1.1, 0.6])}


def joint_contract_ref(inp, mse, use2, use3, dt=torch.float64, drop_bone=None):
    """joint_2d, bone_direc, bone_direc_3d (losses.py:267-282, utils/losses_util.py:217-283 with confidence 1) and the gradient of
    sum_k gout[k] out[k] in closed form: d |vn - vgn|^2 / dv = 2 / (|v| + eps) (dn - vn (dn . v) / |v|), the second term taken as zero at
    |v| = 0 (autograd: NaN).  drop_bone: without that bone of the last sample."""
    lam = [float(torch.tensor(v, dtype=torch.float32)) for v in JOINT_LAMBDAS]
    gout = inp["gout"].to(dt)
    par, chi = torch.tensor(_BONE_PARENT), torch.tensor(_BONE_CHILD)
    B = inp["j2d"].shape[0]
    out, grads = [torch.zeros(1, dtype=dt)] * 3, {}

    def bones(j, jg, k):
        v, vg = j[:, chi] - j[:, par], jg[:, chi] - jg[:, par]
        n = v.pow(2).sum(2, keepdim=True).sqrt()
        il = 1 / (n + 1e-4)
        vn = v * il
        dn = vn - vg * (1 / (vg.pow(2).sum(2, keepdim=True).sqrt() + 1e-4))        # (the same form on both sides: an identical pair gives exactly 0)
        keep = torch.ones(B, 20, 1, dtype=dt)
        if drop_bone is not None:
            keep[B - 1, drop_bone] = 0
        term = lam[k] * (dn.pow(2).sum(2, keepdim=True) * keep).sum() / (B * 20)
        radial = torch.where(n > 0, (dn * vn).sum(2, keepdim=True) * v / n.clamp_min(1e-300), torch.zeros_like(v))
        gv = 2 * gout[k] * lam[k] / (B * 20) * il * (dn - radial) * keep
        g = torch.zeros_like(j)
        g.index_add_(1, chi, gv)
        g.index_add_(1, par, -gv)
        return term.reshape(1), g
    if use2:
        j, jg = inp["j2d"].to(dt), inp["j2d_gt"].to(dt)
        d = jg - j
        out[0] = (lam[0] * ((d * d) if mse else d.abs()).mean()).reshape(1)
        out[1], g = bones(j, jg, 1)
        grads["g2"] = g - gout[0] * lam[0] / d.numel() * ((2 * d) if mse else torch.sign(d))
    if use3:
        out[2], grads["g3"] = bones(inp["j3d"].to(dt), inp["j3d_gt"].to(dt), 2)
    return out, grads


def joint_contract_case(lib, device, B, mse, use2=True, use3=True, special="random", J=21, seed=0):
    from hifihr_amd._lib import _fp
    import ctypes
    what = f"joint_terms {(B, mse, use2, use3, special, J)}"
    Bs = max(B, 1)
    inp = joint_contract_inputs(Bs, special, seed, J)
    G = Guards(device)
    a2 = (G.inp(inp["j2d"]), G.inp(inp["j2d_gt"]))
    a3 = (G.inp(inp["j3d"]), G.inp(inp["j3d_gt"]))
    gout, out, g2, g3 = G.inp(inp["gout"]), G.out(3), G.out(Bs, J, 2), G.out(Bs, J, 3)
    lam = (ctypes.c_float * 3)(*JOINT_LAMBDAS)
    N = lambda t, use: t if use else None
    fwd = lambda p2=N(a2[0], use2), q2=N(a2[1], use2), p3=N(a3[0], use3), q3=N(a3[1], use3), o=out, lm=lam: _raw(
        lib, "hifihr_joint_terms_fwd", _fp(p2), _fp(q2), _fp(p3), _fp(q3), B, J, int(mse), lm, _fp(o), None)
    bwd = lambda p2=N(a2[0], use2), q2=N(a2[1], use2), p3=N(a3[0], use3), q3=N(a3[1], use3), go=gout, o2=N(g2, use2), o3=N(g3, use3), lm=lam: _raw(
        lib, "hifihr_joint_terms_bwd", _fp(p2), _fp(q2), _fp(p3), _fp(q3), B, J, int(mse), lm, _fp(go), _fp(o2), _fp(o3), None)
    if not joint_contract_expect(B, J, use2, use3):
        _tail_refuses("joint_terms_fwd", lib, device, fwd, G, what)
        _tail_refuses("joint_terms_bwd", lib, device, (lambda: bwd(o2=g2, o3=g3)) if not (use2 or use3) and B > 0 and J == 21 else bwd, G, what)
        return False
    ref, gref = joint_contract_ref(inp, mse, use2, use3)
    fwd()
    Ls = (B * 21 * 2, B * 20 * 2, B * 20 * 3)
    for k in range(3):
        _tail_close("joint_terms_fwd", "joint_out", out[k:k + 1], ref[k], Ls[k], f"{what}: out[{k}]")
        if not (use2, use2, use3)[k]:
            assert float(out[k]) == 0.0, f"{what}: a term without inputs must be exactly 0"
    first = out.clone()
    fwd()
    _layer_equal("joint_terms_fwd", out, first, f"{what}: second call")
    bwd()
    for use, got, name in ((use2, g2, "g2"), (use3, g3, "g3")):           # per sample: a zero-length bone's 1 / eps must not hide the others
        for b in range(B if use else 0):
            _tail_close("joint_terms_bwd", "joint_grad", got[b], gref[name][b], 6, f"{what}: {name}, sample {b}")
    firsts = (g2.clone(), g3.clone())
    bwd()
    _layer_equal("joint_terms_bwd", g2, firsts[0], f"{what}: g_j2d, second call")
    _layer_equal("joint_terms_bwd", g3, firsts[1], f"{what}: g_joints, second call")
    if use2 and use3:                                                     # each gradient NULL: the other is the same bits
        h2, h3 = G.out(Bs, J, 2), G.out(Bs, J, 3)
        bwd(o2=h2, o3=None)
        bwd(o2=None, o3=h3)
        _layer_equal("joint_terms_bwd", h2, firsts[0], f"{what}: g_j2d alone")
        _layer_equal("joint_terms_bwd", h3, firsts[1], f"{what}: g_joints alone")
    G.intact(what)
    if use2:
        _tail_refuses("joint_terms_fwd", lib, device, lambda: fwd(q2=None), G, f"{what}: j2d without its gt")
        _tail_refuses("joint_terms_bwd", lib, device, lambda: bwd(q2=None), G, f"{what}: j2d without its gt")
    else:
        _tail_refuses("joint_terms_bwd", lib, device, lambda: bwd(o2=g2), G, f"{what}: g_j2d without j2d")
    if use3:
        _tail_refuses("joint_terms_fwd", lib, device, lambda: fwd(q3=None), G, f"{what}: joints without their gt")
        _tail_refuses("joint_terms_bwd", lib, device, lambda: bwd(q3=None), G, f"{what}: joints without their gt")
    else:
        _tail_refuses("joint_terms_bwd", lib, device, lambda: bwd(o3=g3), G, f"{what}: g_joints without joints")
    _tail_refuses("joint_terms_fwd", lib, device, lambda: fwd(o=None), G, f"{what}: out NULL")
    _tail_refuses("joint_terms_fwd", lib, device, lambda: fwd(lm=None), G, f"{what}: lambda NULL")
    _tail_refuses("joint_terms_bwd", lib, device, lambda: bwd(go=None), G, f"{what}: gout NULL")
    _tail_refuses("joint_terms_bwd", lib, device, lambda: bwd(lm=None), G, f"{what}: lambda NULL")
    _tail_drain(lib, device)
    return True


# ---- geometry terms (csrc/losses.hip) ----------------------------------------------------------------------------------------------------
GEOM_LAMBDAS = (1e4, 1e4, 1e2, 0.25, 0.5)


def geom_contract_expect(B, J, V, F, NS, NP):
    return B > 0 and J > 0 and V > 0 and F >= 0 and NS >= 0 and NP >= 0


def geom_contract_inputs(B, J, V, F, NS, NP, special, seed):
    """special: "random"; "identical" (pred = gt: sign(0) = 0 everywhere); "zero_edges" (face 0 has a zero-length PREDICTED edge, face 1 a
    zero-length GT edge).  The last vertex is in no face whenever V > 3."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    inp = {"joints": rnd(B, J, 3) * 0.05, "joints_gt": rnd(B, J, 3) * 0.05, "verts": rnd(B, V, 3) * 0.05, "verts_gt": rnd(B, V, 3) * 0.05,
           "shape": rnd(B, NS), "pose": rnd(B, NP), "gout": torch.tensor([0.7, 1.3, 0.9, 1.1, 0.6])}
    Vf = V - 1 if V > 3 else V
    inp["faces"] = torch.stack([torch.randperm(Vf, generator=gen)[:3] for _ in range(F)]).int() if F > 0 and V >= 3 else None
    if special == "identical":
        inp["joints"], inp["verts"] = inp["joints_gt"].clone(), inp["verts_gt"].clone()
    elif special == "zero_edges" and inp["faces"] is not None and F >= 2 and V >= 7:
        inp["faces"][0] = torch.tensor([0, 1, 2], dtype=torch.int32)
        inp["faces"][1] = torch.tensor([3, 4, 5], dtype=torch.int32)
        inp["verts"][:, 1] = inp["verts"][:, 0]
        inp["verts_gt"][:, 4] = inp["verts_gt"][:, 3]
    return inp


def geom_contract_ref(inp, mse, dt=torch.float64, drop_vertex=None, drop_face=None):
    """The five terms and their gradients in closed form (autograd gives NaN at a zero-length predicted edge; the kernel -- and this
    reference -- give that edge no gradient).  -> out: five (kind, L, value); grads: gj, gv, gs, gp as (kind, L, tensor)."""
    lam = [float(torch.tensor(v, dtype=torch.float32)) for v in GEOM_LAMBDAS]
    gout = inp["gout"].to(dt)
    j, jg, v, vg, sh, po = (inp[k].to(dt) for k in ("joints", "joints_gt", "verts", "verts_gt", "shape", "pose"))
    B, J, V, NS, NP = j.shape[0], j.shape[1], v.shape[1], sh.shape[1], po.shape[1]
    faces = inp["faces"].long() if inp["faces"] is not None else None
    F = 0 if faces is None else faces.shape[0]
    base = (lambda d: d * d) if mse else (lambda d: d.abs())
    bgrad = (lambda d: 2 * d) if mse else torch.sign
    vkeep = torch.ones(1, V, 1, dtype=dt)
    if drop_vertex is not None:
        vkeep[0, drop_vertex] = 0
    out = [("geom_out", B * J * 3, (lam[0] * base(j - jg).sum() / (B * J * 3)).reshape(1)),
           ("geom_out", B * V * 3, (lam[1] * (base(v - vg) * vkeep).sum() / (B * V * 3)).reshape(1))]
    gv = gout[1] * lam[1] / (B * V * 3) * bgrad(v - vg) * vkeep
    valence = torch.zeros(V)
    if F:
        fkeep = torch.ones(F, dtype=dt)
        if drop_face is not None:
            fkeep[drop_face] = 0
        e = torch.zeros((), dtype=dt)
        ce = gout[2] * lam[2] / (B * F * 3)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ia, ib = faces[:, a], faces[:, b]
            dp, dg = v[:, ia] - v[:, ib], vg[:, ia] - vg[:, ib]
            lp, lg = dp.pow(2).sum(2).sqrt(), dg.pow(2).sum(2).sqrt()
            e = e + ((lp - lg).abs() * fkeep).sum()
            k = torch.where(lp > 0, ce * torch.sign(lp - lg) / lp.clamp_min(1e-300), torch.zeros_like(lp)) * fkeep
            gv = gv.index_add(1, ia, k.unsqueeze(2) * dp).index_add(1, ib, -k.unsqueeze(2) * dp)
            valence.index_add_(0, ia, torch.ones(F)).index_add_(0, ib, torch.ones(F))
        out.append(("geom_out", B * F * 3, (lam[2] * e / (B * F * 3)).reshape(1)))
    else:
        out.append(("geom_out", 1, torch.zeros(1, dtype=dt)))
    out.append(("geom_out", B * NS, (lam[3] * sh.pow(2).sum() / (B * NS)).reshape(1) if NS else torch.zeros(1, dtype=dt)))
    out.append(("geom_out", B * NP, (lam[4] * po.pow(2).sum() / (B * NP)).reshape(1) if NP else torch.zeros(1, dtype=dt)))
    grads = {"gj": ("geom_grad", 1, gout[0] * lam[0] / (B * J * 3) * bgrad(j - jg)), "gv": ("geom_grad", 1 + int(valence.max()), gv),
             "gs": ("geom_grad", 1, gout[3] * lam[3] * 2 / (B * max(NS, 1)) * sh), "gp": ("geom_grad", 1, gout[4] * lam[4] * 2 / (B * max(NP, 1)) * po)}
    return out, grads


def geom_contract_case(lib, device, B, J, V, F, NS, NP, mse, special="random", seed=0):
    from hifihr_amd._lib import _fp, _ip
    import ctypes
    what = f"geom_loss {(B, J, V, F, NS, NP, mse, special)}"
    Bs, Js, Vs = max(B, 1), max(J, 1), max(V, 1)
    inp = geom_contract_inputs(Bs, Js, Vs, F, NS, NP, special, seed)
    Fe = 0 if inp["faces"] is None else F
    G = Guards(device)
    d = {k: G.inp(inp[k]) for k in ("joints", "joints_gt", "verts", "verts_gt", "shape", "pose", "faces", "gout")}
    off = idx = None
    if Fe:
        o_, i_ = vertex_face_csr(inp["faces"].numpy(), Vs)
        off, idx = G.inp(torch.from_numpy(o_)), G.inp(torch.from_numpy(i_))
    partial, out = G.out(Bs * 5), G.out(5)
    scratch = G.outs.pop(-2)                                               # partial: scratch, only its surroundings are watched
    gj, gv, gs, gp = G.out(Bs, Js, 3), G.out(Bs, Vs, 3), G.out(Bs, NS), G.out(Bs, NP)
    lam = (ctypes.c_float * 5)(*GEOM_LAMBDAS)
    nn = lambda t, n: t if n > 0 else None                                # (an empty tensor's pointer is no use: NULL where the count is 0)

    def fwd(B_=B, J_=J, V_=V, F_=Fe, NS_=NS, NP_=NP, lm=lam, **kw):
        a = dict(d, partial=partial, out=out)
        a.update(kw)
        _raw(lib, "hifihr_geom_loss_fwd", _fp(a["joints"]), _fp(a["joints_gt"]), _fp(a["verts"]), _fp(a["verts_gt"]), _fp(nn(a["shape"], NS_)),
             _fp(nn(a["pose"], NP_)), _ip(a["faces"]), B_, J_, V_, F_, NS_, NP_, int(mse), lm, _fp(a["partial"]), _fp(a["out"]), None)

    def bwd(B_=B, J_=J, V_=V, F_=Fe, NS_=NS, NP_=NP, lm=lam, **kw):
        a = dict(d, off=off, idx=idx, gj=gj, gv=gv, gs=nn(gs, NS), gp=nn(gp, NP))
        a.update(kw)
        _raw(lib, "hifihr_geom_loss_bwd", _fp(a["joints"]), _fp(a["joints_gt"]), _fp(a["verts"]), _fp(a["verts_gt"]), _fp(nn(a["shape"], NS_)),
             _fp(nn(a["pose"], NP_)), _ip(a["faces"]), _ip(a["off"]), _ip(a["idx"]), B_, J_, V_, F_, NS_, NP_, int(mse), lm, _fp(a["gout"]),
             _fp(a["gj"]), _fp(a["gv"]), _fp(a["gs"]), _fp(a["gp"]), None)
    if not geom_contract_expect(B, J, V, F, NS, NP):
        G.outs.append(scratch)
        _tail_refuses("geom_loss_fwd", lib, device, fwd, G, what)
        _tail_refuses("geom_loss_bwd", lib, device, bwd, G, what)
        return False
    ref, gref = geom_contract_ref(inp, mse)
    fwd()
    for k in range(5):
        _tail_close("geom_loss_fwd", ref[k][0], out[k:k + 1], ref[k][2], ref[k][1], f"{what}: out[{k}]")
    for k, cnt in ((2, Fe), (3, NS), (4, NP)):
        assert cnt > 0 or float(out[k]) == 0.0, f"{what}: a term with count 0 must be exactly 0, out[{k}] = {float(out[k])}"
    first = out.clone()
    fwd()
    _layer_equal("geom_loss_fwd", out, first, f"{what}: second call")
    bwd()
    got = {"gj": gj, "gv": gv, "gs": gs, "gp": gp}
    for name in ("gj", "gv", "gs", "gp"):
        q = gref[name]
        _tail_close("geom_loss_bwd", q[0], got[name], q[2], q[1], f"{what}: {name}")
    firsts = {k: v.clone() for k, v in got.items()}
    bwd()
    for name in got:
        _layer_equal("geom_loss_bwd", got[name], firsts[name], f"{what}: {name}, second call")
    for name in ("gj", "gv", "gs", "gp"):                                   # each gradient NULL: the others are the same bits
        fresh = {"gj": G.out(Bs, Js, 3), "gv": G.out(Bs, Vs, 3), "gs": nn(G.out(Bs, NS), NS), "gp": nn(G.out(Bs, NP), NP)}
        fresh[name] = None
        bwd(**fresh)
        for other in got:
            if other != name and fresh[other] is not None:
                _layer_equal("geom_loss_bwd", fresh[other], firsts[other], f"{what}: {other} with {name} NULL")
    G.intact(what)
    whole, lo, hi, canary = scratch
    assert bool((whole[:lo] == canary).all()) and bool((whole[hi:] == canary).all()), f"{what}: wrote outside the partial sums"
    G.outs.append(scratch)
    bad = [("joints NULL", dict(joints=None)), ("joints_gt NULL", dict(joints_gt=None)), ("verts NULL", dict(verts=None)), ("verts_gt NULL", dict(verts_gt=None)),
           ("lambda NULL", dict(lm=None)), ("F < 0", dict(F_=-1)), ("NS < 0", dict(NS_=-1)), ("NP < 0", dict(NP_=-1))]
    bad += [("faces NULL", dict(faces=None))] if Fe else [("F > 0 without faces", dict(F_=3, faces=None))]
    bad += [("shape NULL", dict(shape=None))] if NS else [("NS > 0 without shape", dict(NS_=4, shape=None))]
    bad += [("pose NULL", dict(pose=None))] if NP else [("NP > 0 without pose", dict(NP_=4, pose=None))]
    for why, kw in bad:
        _tail_refuses("geom_loss_fwd", lib, device, lambda: fwd(**kw), G, f"{what}: {why}")
        _tail_refuses("geom_loss_bwd", lib, device, lambda: bwd(**kw), G, f"{what}: {why}")
    _tail_refuses("geom_loss_fwd", lib, device, lambda: fwd(partial=None), G, f"{what}: partial NULL")
    _tail_refuses("geom_loss_fwd", lib, device, lambda: fwd(out=None), G, f"{what}: out NULL")
    _tail_refuses("geom_loss_bwd", lib, device, lambda: bwd(gout=None), G, f"{what}: gout NULL")
    if Fe:
        _tail_refuses("geom_loss_bwd", lib, device, lambda: bwd(off=None), G, f"{what}: no vertex -> face offsets")
        _tail_refuses("geom_loss_bwd", lib, device, lambda: bwd(idx=None), G, f"{what}: no vertex -> face table")
    _tail_drain(lib, device)
    return True


# ---- MANO layer, joint regression, the fused form (csrc/mano_lbs.hip) -------------------------------------------------------------------
TAIL_LEGACY.update({
    "mano_v": lambda ref, L: 5e-6,                                        # mano_fwd_bwd_case / mano_full_case: absolute, metres
    "mano_j": lambda ref, L: 2e-6,                                        # mano_joints_case
    "mano_g": lambda ref, L: 3e-4 * float(ref.abs().max()),               # mano_fwd_bwd_case / mano_full_case: of the largest gradient
    "mano_gv": lambda ref, L: 2e-4,                                       # mano_joints_case
    "lbs_v": lambda ref, L: 2e-6 * max(1.0, float(ref.abs().max()) / 0.1),           # lbs_case
    "lbs_g": lambda ref, L: 2e-4 * float(ref.abs().max()),
})
MANO_POSE_FAMILIES = ("zero", "1e-7", "1e-4", "0.6", "3.0", "root0", "rootpi")


def mano_contract_inputs(B, family, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    scale = {"zero": 0.0, "root0": 0.6, "rootpi": 0.6}.get(family)
    pose = rnd(B, 48) * (float(family) if scale is None else scale)
    if family == "root0":
        pose[:, :3] = 0.0                                                 # the root rotation exactly 0
    elif family == "rootpi":
        pose[:, :3] = 0.0
        pose[torch.arange(B), torch.arange(B) % 3] = float(np.float32(np.pi))          # exactly pi about an axis
    return {"pose": pose, "beta": rnd(B, 10) * 0.7, "root_xyz": rnd(B, 3) * 0.3, "wv": rnd(B, 778, 3), "wj": rnd(B, 21, 3), "wc": rnd(B, 778, 3),
            "wr": rnd(B, 3), "wv2": rnd(B, 778, 3), "wj2": rnd(B, 21, 3), "ap": rnd(B, 48), "ab": rnd(B, 10)}


def mano_layer_ref(tables, inp, dt=torch.float64, drop_vertex=None):
    """ManoLayer.forward and, per incoming gradient, d/d(pose, beta): {"v": of sum(verts wv), "j": of sum(jtr wj)} (linear: a NULL
    gradient leaves its part out).  drop_vertex: that vertex's gverts left out."""
    pose, beta = inp["pose"].to(dt).requires_grad_(True), inp["beta"].to(dt).requires_grad_(True)
    verts, jtr, _ = mo.mano_forward(tables, pose, beta, dtype=dt)
    wv = inp["wv"].to(dt).clone()
    if drop_vertex is not None:
        wv[:, drop_vertex] = 0
    g = {k: torch.autograd.grad(t, (pose, beta), retain_graph=True) for k, t in (("v", (verts * wv).sum()), ("j", (jtr * inp["wj"].to(dt)).sum()))}
    return verts.detach(), jtr.detach(), g


def mano_joints_ref(tables, verts, inp, root_id, dt=torch.float64, drop_vertex=None):
    """xyz_from_vertice + the root-relative step on `verts`, and per incoming gradient d/dverts: "j", "v", "r"."""
    v = verts.to(dt).clone().requires_grad_(True)
    vin = v
    if drop_vertex is not None:
        m = torch.ones(1, 778, 1, dtype=dt)
        m[0, drop_vertex] = 0
        vin = v * m
    j = mo.xyz_from_vertice(tables, vin, dtype=dt)
    if root_id >= 0:
        jr, vr, root = mo.root_relative(j, v, root_id)
    else:
        jr, vr, root = j, v, torch.zeros(v.shape[0], 1, 3, dtype=dt)
    terms = {"j": (jr * inp["wj2"].to(dt)).sum(), "v": (vr * inp["wv2"].to(dt)).sum(), "r": (root.reshape(-1, 3) * inp["wr"].to(dt)).sum()}
    g = {k: (torch.autograd.grad(t, v, retain_graph=True)[0] if t.requires_grad else torch.zeros_like(v)) for k, t in terms.items()}
    return jr.detach(), vr.detach(), root.detach().reshape(-1, 3), g


def mano_full_ref(tables, inp, root_id, dt=torch.float64):
    """The chain layer -> regression -> root-relative -> + root_xyz and, per incoming gradient, d/d(pose, beta): "j", "v", "c", "r"."""
    pose, beta = inp["pose"].to(dt).requires_grad_(True), inp["beta"].to(dt).requires_grad_(True)
    verts, _, _ = mo.mano_forward(tables, pose, beta, dtype=dt)
    j = mo.xyz_from_vertice(tables, verts, dtype=dt)
    if root_id >= 0:
        jr, vr, root = mo.root_relative(j, verts, root_id)
    else:
        jr, vr, root = j, verts, torch.zeros(verts.shape[0], 1, 3, dtype=dt)
    vc = vr + inp["root_xyz"].to(dt).unsqueeze(1)
    terms = {"j": (jr * inp["wj2"].to(dt)).sum(), "v": (vr * inp["wv2"].to(dt)).sum(), "c": (vc * inp["wc"].to(dt)).sum(),
             "r": (root.reshape(-1, 3) * inp["wr"].to(dt)).sum()}
    zero = (torch.zeros_like(pose), torch.zeros_like(beta))
    g = {k: (torch.autograd.grad(t, (pose, beta), retain_graph=True) if t.requires_grad else zero) for k, t in terms.items()}
    return {"verts": verts.detach(), "jr": jr.detach(), "vr": vr.detach(), "vc": vc.detach(), "root": root.detach().reshape(-1, 3)}, g


def mano_contract_case(lib, device, tables, B, family, root_id, seed=0):
    """All six hifihr_mano_* compute entries on one (batch, pose family, root) -- see the section header for the contract."""
    from hifihr_amd._lib import _fp
    what = f"mano {(B, family, root_id)}"
    Bs = max(B, 1)
    inp = mano_contract_inputs(Bs, family, seed)
    G = Guards(device)
    d = {k: G.inp(v) for k, v in inp.items()}
    h = lib.mano_create(tables)
    NV = 778
    try:
        lfwd = lambda pose=d["pose"], beta=d["beta"], verts=None, jtr=None, saved=None, hh=h, B_=B: _raw(
            lib, "hifihr_mano_lbs_fwd", hh, _fp(pose), _fp(beta), B_, _fp(verts), _fp(jtr), _fp(saved), None)
        lbwd = lambda pose=d["pose"], beta=d["beta"], saved=None, gv=d["wv"], gj=d["wj"], gp=None, gb=None, hh=h, B_=B: _raw(
            lib, "hifihr_mano_lbs_bwd", hh, _fp(pose), _fp(beta), _fp(saved), _fp(gv), _fp(gj), B_, _fp(gp), _fp(gb), None)
        jfwd = lambda verts=None, jr=None, vr=None, root=None, rid=root_id, hh=h, B_=B: _raw(
            lib, "hifihr_mano_joints_fwd", hh, _fp(verts), B_, rid, _fp(jr), _fp(vr), _fp(root), None)
        jbwd = lambda gj=d["wj2"], gv=d["wv2"], gr=d["wr"], out=None, rid=root_id, hh=h, B_=B: _raw(
            lib, "hifihr_mano_joints_bwd", hh, _fp(gj), _fp(gv), _fp(gr), B_, rid, _fp(out), None)
        ffwd = lambda pose=d["pose"], beta=d["beta"], rxyz=d["root_xyz"], verts=None, jr=None, vr=None, vc=None, root=None, saved=None, rid=root_id, hh=h, B_=B: _raw(
            lib, "hifihr_mano_full_fwd", hh, _fp(pose), _fp(beta), B_, rid, _fp(rxyz), _fp(verts), _fp(jr), _fp(vr), _fp(vc), _fp(root), _fp(saved), None)
        fbwd = lambda pose=d["pose"], beta=d["beta"], saved=None, gj=d["wj2"], gv=d["wv2"], gc=d["wc"], gr=d["wr"], ap=None, ab=None, gp=None, gb=None, rid=root_id, hh=h, B_=B: _raw(
            lib, "hifihr_mano_full_bwd", hh, _fp(pose), _fp(beta), _fp(saved), _fp(gj), _fp(gv), _fp(gc), _fp(gr), _fp(ap), _fp(ab), B_, rid, _fp(gp), _fp(gb), None)
        V3 = lambda: G.out(Bs, NV, 3)
        verts, jtr, saved, gp, gb = V3(), G.out(Bs, 21, 3), V3(), G.out(Bs, 48), G.out(Bs, 10)
        jr, vr, root, gverts = G.out(Bs, 21, 3), V3(), G.out(Bs, 3), V3()
        if B < 0 or root_id >= 21:
            _tail_refuses("mano_full_fwd", lib, device, lambda: ffwd(verts=verts, jr=jr, vr=vr, saved=saved), G, what)
            _tail_refuses("mano_full_bwd", lib, device, lambda: fbwd(saved=saved, gp=gp, gb=gb), G, what)
            _tail_refuses("mano_joints_fwd", lib, device, lambda: jfwd(verts=d["wv"], jr=jr, vr=vr, root=root), G, what)
            _tail_refuses("mano_joints_bwd", lib, device, lambda: jbwd(out=gverts), G, what)
            if B < 0:
                _tail_refuses("mano_lbs_fwd", lib, device, lambda: lfwd(verts=verts, jtr=jtr, saved=saved), G, what)
                _tail_refuses("mano_lbs_bwd", lib, device, lambda: lbwd(saved=saved, gp=gp, gb=gb), G, what)
            return False
        if B == 0:                                                        # accepted; writes nothing, launches nothing
            _tail_drain(lib, device)
            before = [w.clone() for w in G.wholes()]
            for e, call in (("mano_lbs_fwd", lambda: lfwd(verts=verts, jtr=jtr, saved=saved)), ("mano_lbs_bwd", lambda: lbwd(saved=saved, gp=gp, gb=gb)),
                            ("mano_joints_fwd", lambda: jfwd(verts=d["wv"], jr=jr, vr=vr, root=root)), ("mano_joints_bwd", lambda: jbwd(out=gverts)),
                            ("mano_full_fwd", lambda: ffwd(verts=verts, jr=jr, vr=vr, saved=saved)), ("mano_full_bwd", lambda: fbwd(saved=saved, gp=gp, gb=gb))):
                call()
                _layer_log(e, True)
            assert not _tail_drain(lib, device), f"{what}: B = 0 launched a kernel"
            assert all(torch.equal(a, b) for a, b in zip(G.wholes(), before)), f"{what}: B = 0 wrote"
            return True
        # ---- the layer ----
        rv, rj, rg = mano_layer_ref(tables, inp)
        lfwd(verts=verts, jtr=jtr, saved=saved)
        _tail_close("mano_lbs_fwd", "mano_v", verts, rv, 16, f"{what}: verts")
        _tail_close("mano_lbs_fwd", "mano_v", jtr, rj, 16, f"{what}: jtr")
        first = (verts.clone(), jtr.clone(), saved.clone())
        lfwd(verts=verts, jtr=jtr, saved=saved)
        for a, b, n in zip((verts, jtr, saved), first, ("verts", "jtr", "saved")):
            _layer_equal("mano_lbs_fwd", a, b, f"{what}: {n}, second call")
        v2, j2 = V3(), G.out(Bs, 21, 3)
        lfwd(verts=v2, jtr=None, saved=None)                              # jtr / saved NULL
        _layer_equal("mano_lbs_fwd", v2, first[0], f"{what}: verts with jtr and saved NULL")
        lbwd(saved=saved, gp=gp, gb=gb)
        _tail_close("mano_lbs_bwd", "mano_g", gp, rg["v"][0] + rg["j"][0], NV, f"{what}: gpose")
        _tail_close("mano_lbs_bwd", "mano_g", gb, rg["v"][1] + rg["j"][1], NV, f"{what}: gbeta")
        g1 = (gp.clone(), gb.clone())
        lbwd(saved=saved, gp=gp, gb=gb)                                   # overwritten, deterministic
        _layer_equal("mano_lbs_bwd", gp, g1[0], f"{what}: gpose, second call")
        _layer_equal("mano_lbs_bwd", gb, g1[1], f"{what}: gbeta, second call")
        for null, keep in (("gv", "j"), ("gj", "v")):
            gp2, gb2 = G.out(Bs, 48), G.out(Bs, 10)
            lbwd(saved=saved, gp=gp2, gb=gb2, **{null: None})
            _tail_close("mano_lbs_bwd", "mano_g", gp2, rg[keep][0], NV, f"{what}: gpose with {null} NULL")
            _tail_close("mano_lbs_bwd", "mano_g", gb2, rg[keep][1], NV, f"{what}: gbeta with {null} NULL")
        # ---- regression + root-relative step, on the layer's own vertices ----
        qjr, qvr, qroot, qg = mano_joints_ref(tables, first[0].cpu(), inp, root_id)
        jfwd(verts=verts, jr=jr, vr=vr, root=root)
        for got, ref_, n in ((jr, qjr, "joints_rel"), (vr, qvr, "verts_rel"), (root, qroot, "root")):
            _tail_close("mano_joints_fwd", "mano_j", got, ref_, NV, f"{what}: {n}")
        two = (jr.clone(), vr.clone(), root.clone())
        alias, jr2 = V3(), G.out(Bs, 21, 3)
        alias.copy_(verts)
        jfwd(verts=alias, jr=jr2, vr=alias, root=None)                    # verts_rel aliasing verts; root NULL
        _layer_equal("mano_joints_fwd", alias, two[1], f"{what}: verts_rel written over verts")
        _layer_equal("mano_joints_fwd", jr2, two[0], f"{what}: joints_rel, aliased call")
        jr3 = G.out(Bs, 21, 3)
        jfwd(verts=verts, jr=jr3, vr=None, root=None)                     # verts_rel NULL
        _layer_equal("mano_joints_fwd", jr3, two[0], f"{what}: joints_rel with verts_rel NULL")
        jbwd(out=gverts)
        _tail_close("mano_joints_bwd", "mano_gv", gverts, qg["j"] + qg["v"] + qg["r"], 22, f"{what}: gverts")
        gv1 = gverts.clone()
        jbwd(out=gverts)
        _layer_equal("mano_joints_bwd", gverts, gv1, f"{what}: gverts, second call")
        for null, keep in (("gj", "vr"), ("gv", "jr"), ("gr", "jv")):
            gv2 = V3()
            jbwd(out=gv2, **{null: None})
            _tail_close("mano_joints_bwd", "mano_gv", gv2, sum(qg[k] for k in keep), 22, f"{what}: gverts with {null} NULL")
        # ---- the fused form: bit for bit the two-call form ----
        fr, fg = mano_full_ref(tables, inp, root_id)
        o = {"verts": V3(), "jr": G.out(Bs, 21, 3), "vr": V3(), "vc": V3(), "root": G.out(Bs, 3), "saved": V3()}
        ffwd(**o)
        for k, want in (("verts", first[0]), ("saved", first[2]), ("jr", two[0]), ("vr", two[1]), ("root", two[2])):
            _layer_equal("mano_full_fwd", o[k], want, f"{what}: fused {k} against the two-call form")
        _tail_close("mano_full_fwd", "mano_v", o["vc"], fr["vc"], 16, f"{what}: verts_cam")
        _tail_close("mano_full_fwd", "mano_v", o["vr"], fr["vr"], 16, f"{what}: verts_rel against the chain")
        o2 = {"verts": V3(), "jr": G.out(Bs, 21, 3), "vr": V3(), "vc": V3()}
        ffwd(rxyz=None, **o2)                                             # root_xyz / root / saved NULL: verts_cam = verts_rel
        _layer_equal("mano_full_fwd", o2["vc"], two[1], f"{what}: verts_cam with root_xyz NULL")
        _layer_equal("mano_full_fwd", o2["jr"], two[0], f"{what}: joints_rel with root and saved NULL")
        o3 = {"verts": V3(), "jr": G.out(Bs, 21, 3), "vr": V3()}
        ffwd(**o3)                                                        # verts_cam NULL
        _layer_equal("mano_full_fwd", o3["vr"], two[1], f"{what}: verts_rel with verts_cam NULL")
        fbwd(saved=saved, gp=gp, gb=gb)
        tot = lambda keys, i: sum(fg[k][i] for k in keys)
        _tail_close("mano_full_bwd", "mano_g", gp, tot("jvcr", 0), NV, f"{what}: fused gpose")
        _tail_close("mano_full_bwd", "mano_g", gb, tot("jvcr", 1), NV, f"{what}: fused gbeta")
        f1 = (gp.clone(), gb.clone())
        fbwd(saved=saved, gp=gp, gb=gb)
        _layer_equal("mano_full_bwd", gp, f1[0], f"{what}: fused gpose, second call")
        _layer_equal("mano_full_bwd", gb, f1[1], f"{what}: fused gbeta, second call")
        for null, keep in (("gj", "vcr"), ("gv", "jcr"), ("gc", "jvr"), ("gr", "jvc")):
            gp2, gb2 = G.out(Bs, 48), G.out(Bs, 10)
            fbwd(saved=saved, gp=gp2, gb=gb2, **{null: None})
            _tail_close("mano_full_bwd", "mano_g", gp2, tot(keep, 0), NV, f"{what}: fused gpose with {null} NULL")
            _tail_close("mano_full_bwd", "mano_g", gb2, tot(keep, 1), NV, f"{what}: fused gbeta with {null} NULL")
        gp3, gb3 = G.out(Bs, 48), G.out(Bs, 10)
        fbwd(saved=saved, gp=gp3, gb=gb3, ap=d["ap"], ab=d["ab"])          # gpose_add / gbeta_add: one fp32 addition on top
        _layer_equal("mano_full_bwd", gp3, f1[0].cpu() + inp["ap"], f"{what}: gpose_add")
        _layer_equal("mano_full_bwd", gb3, f1[1].cpu() + inp["ab"], f"{what}: gbeta_add")
        G.intact(what)
        # ---- refused: NULLs ----
        for e, calls in (("mano_lbs_fwd", (lambda: lfwd(verts=verts, jtr=jtr, hh=None), lambda: lfwd(pose=None, verts=verts), lambda: lfwd(beta=None, verts=verts), lambda: lfwd())),
                         ("mano_lbs_bwd", (lambda: lbwd(saved=saved, gp=gp, gb=gb, hh=None), lambda: lbwd(pose=None, saved=saved, gp=gp, gb=gb), lambda: lbwd(beta=None, saved=saved, gp=gp, gb=gb),
                                           lambda: lbwd(gp=gp, gb=gb), lambda: lbwd(saved=saved, gb=gb), lambda: lbwd(saved=saved, gp=gp))),
                         ("mano_joints_fwd", (lambda: jfwd(verts=verts, jr=jr, hh=None), lambda: jfwd(jr=jr), lambda: jfwd(verts=verts))),
                         ("mano_joints_bwd", (lambda: jbwd(out=gverts, hh=None), lambda: jbwd())),
                         ("mano_full_fwd", (lambda: ffwd(verts=verts, jr=jr, vr=vr, hh=None), lambda: ffwd(pose=None, verts=verts, jr=jr, vr=vr), lambda: ffwd(beta=None, verts=verts, jr=jr, vr=vr),
                                            lambda: ffwd(jr=jr, vr=vr), lambda: ffwd(verts=verts, vr=vr), lambda: ffwd(verts=verts, jr=jr))),
                         ("mano_full_bwd", (lambda: fbwd(saved=saved, gp=gp, gb=gb, hh=None), lambda: fbwd(pose=None, saved=saved, gp=gp, gb=gb), lambda: fbwd(beta=None, saved=saved, gp=gp, gb=gb),
                                            lambda: fbwd(gp=gp, gb=gb), lambda: fbwd(saved=saved, gb=gb), lambda: fbwd(saved=saved, gp=gp)))):
            for k, call in enumerate(calls):
                _tail_refuses(e, lib, device, call, G, f"{what}: NULL argument {k}")
        _tail_drain(lib, device)
        return True
    finally:
        lib.mano_destroy(h)


# ---- generic linear-blend skinning (csrc/lbs.hip) ---------------------------------------------------------------------------------------
def lbs_contract_inputs(tabs, B, seed):
    vt, sd, jr, w, parents = tabs
    V, J, S = vt.shape[0], w.shape[1], sd.shape[2]
    gen = torch.Generator().manual_seed(seed)
    theta = torch.randn(B, J, 3, generator=gen) * 0.6
    theta[0, min(1, J - 1)] = 0.0                                         # one joint's rotation exactly 0
    theta[B - 1, min(2, J - 1) if B == 1 else 0] = torch.randn(3, generator=gen) * 1e-7          # and one at 1e-7
    return {"theta": theta, "beta": torch.randn(B, S, generator=gen), "wv": torch.randn(B, V, 3, generator=gen), "wj": torch.randn(B, J, 3, generator=gen),
            "prefill": torch.randn(B, S, generator=gen)}


def lbs_contract_ref(tabs, inp, dt=torch.float64, drop_vertex=None):
    """oracle/lbs_oracle.py in `dt`: verts, posed joints, per incoming gradient d/d(theta, beta) ("v", "j"), and what the backward leaves in
    its scratch: gA[b][j] = sum_v w_vj gverts_v [v_shaped_v; 1]^T (3 x 4, row-major)."""
    from oracle import lbs_oracle as lo
    vt, sd, jr, w, parents = tabs
    th, be = inp["theta"].to(dt).requires_grad_(True), inp["beta"].to(dt).requires_grad_(True)
    rv, rj = lo.lbs_forward(vt, sd, jr, w, parents, th, be)
    wv = inp["wv"].to(dt).clone()
    if drop_vertex is not None:
        wv[:, drop_vertex] = 0
    zero = lambda t: torch.zeros_like(t)
    g = {}
    for k, term in (("v", (rv * wv).sum()), ("j", (rj * inp["wj"].to(dt)).sum())):
        gt = torch.autograd.grad(term, (th, be), retain_graph=True, allow_unused=True)
        g[k] = (gt[0] if gt[0] is not None else zero(th), gt[1] if gt[1] is not None else zero(be))
    vs = torch.as_tensor(vt, dtype=dt).unsqueeze(0) + torch.einsum("vck,bk->bvc", torch.as_tensor(sd, dtype=dt), be.detach())
    vs1 = torch.cat([vs, torch.ones_like(vs[..., :1])], 2)
    gA = torch.einsum("vj,bvr,bvc->bjrc", torch.as_tensor(w, dtype=dt), wv, vs1).reshape(wv.shape[0], -1, 12)
    return rv.detach(), rj.detach(), g, gA


def lbs_contract_case(lib, device, V, J, S, B, seed=0):
    from hifihr_amd._lib import _fp
    what = f"lbs {(V, J, S, B)}"
    tabs = random_lbs_tables(V, J, S, seed)
    Bs = max(B, 1)
    inp = lbs_contract_inputs(tabs, Bs, seed)
    G = Guards(device)
    d = {k: G.inp(v) for k, v in inp.items()}
    nn = lambda t: t if S > 0 else None
    h = lib.lbs_create(*tabs)
    try:
        verts, joints, scratch, gth, gbe = G.out(Bs, V, 3), G.out(Bs, J, 3), G.out(Bs, J, 12, fill=0.0), G.out(Bs, J, 3), G.out(Bs, S)
        fwd = lambda theta=d["theta"], beta=nn(d["beta"]), v=verts, j=joints, hh=h, B_=B: _raw(lib, "hifihr_lbs_fwd", hh, _fp(theta), _fp(beta), B_, _fp(v), _fp(j), None)
        bwd = lambda theta=d["theta"], beta=nn(d["beta"]), gv=d["wv"], gj=d["wj"], sc=scratch, gt=gth, gb=nn(gbe), hh=h, B_=B: _raw(
            lib, "hifihr_lbs_bwd", hh, _fp(theta), _fp(beta), _fp(gv), _fp(gj), B_, _fp(sc), _fp(gt), _fp(gb), None)
        if B < 0:
            _tail_refuses("lbs_fwd", lib, device, fwd, G, what)
            _tail_refuses("lbs_bwd", lib, device, bwd, G, what)
            return False
        if B == 0:
            _tail_drain(lib, device)
            before = [w_.clone() for w_ in G.wholes()]
            fwd()
            bwd()
            _layer_log("lbs_fwd", True)
            _layer_log("lbs_bwd", True)
            assert not _tail_drain(lib, device) and all(torch.equal(a, b) for a, b in zip(G.wholes(), before)), f"{what}: B = 0 launched or wrote"
            return True
        rv, rj, rg, rA = lbs_contract_ref(tabs, inp)
        depth = J                                                         # a chain of up to J transforms in front of a vertex
        fwd()
        _tail_close("lbs_fwd", "lbs_v", verts, rv, depth, f"{what}: verts")
        _tail_close("lbs_fwd", "lbs_v", joints, rj, depth, f"{what}: joints")
        v1 = verts.clone()
        v2 = G.out(Bs, V, 3)
        fwd(v=v2, j=None)                                                 # joints NULL
        _layer_equal("lbs_fwd", v2, v1, f"{what}: verts with joints NULL")
        for rep in range(2):                                              # float atomics: each run inside the bound
            scratch.zero_()
            if S:
                gbe.copy_(inp["prefill"])                                 # gbeta is ACCUMULATED: onto what the buffer holds
            bwd()
            _tail_close("lbs_bwd", "lbs_g", gth, rg["v"][0] + rg["j"][0], V, f"{what}: gtheta (run {rep})")
            if S:
                _tail_close("lbs_bwd", "lbs_g", gbe.cpu().double() - inp["prefill"].double(), rg["v"][1] + rg["j"][1], V, f"{what}: gbeta (run {rep})",
                            float(inp["prefill"].abs().max()))
            _tail_close("lbs_bwd", "lbs_g", scratch, rA, V, f"{what}: scratch = d(sum gverts verts) / dA (run {rep})")
        scratch.zero_()
        gth2, gbe2 = G.out(Bs, J, 3), G.out(Bs, S, fill=0.0)
        bwd(gj=None, gt=gth2, gb=nn(gbe2))                                # gjoints NULL
        _tail_close("lbs_bwd", "lbs_g", gth2, rg["v"][0], V, f"{what}: gtheta with gjoints NULL")
        if S:
            _tail_close("lbs_bwd", "lbs_g", gbe2, rg["v"][1], V, f"{what}: gbeta with gjoints NULL")
        G.intact(what)
        bad_f = [lambda: fwd(hh=None), lambda: fwd(theta=None), lambda: fwd(v=None)] + ([lambda: fwd(beta=None)] if S else [])
        bad_b = [lambda: bwd(hh=None), lambda: bwd(theta=None), lambda: bwd(gv=None), lambda: bwd(sc=None), lambda: bwd(gt=None)]
        bad_b += [lambda: bwd(beta=None), lambda: bwd(gb=None)] if S else []
        for k, call in enumerate(bad_f):
            _tail_refuses("lbs_fwd", lib, device, call, G, f"{what}: NULL argument {k}")
        for k, call in enumerate(bad_b):
            _tail_refuses("lbs_bwd", lib, device, call, G, f"{what}: NULL argument {k}")
        _tail_drain(lib, device)
        return True
    finally:
        lib.lbs_destroy(h)


# ------------------------------------------------------------------------------------------------
# The renderer contract: the ten hifihr_render* entries (csrc/render.hip, csrc/render_bwd.hip) on the lists of
# tests/test_hostsim_render_contract.py (the GPU half: tests/test_gpu_render.py), in the tail contract's form.  A case is
# (scene, V/F source[/options], B, image_size, aa, mode); mode: "vc" batched vertex colours, "shared" [V][3] colours, "uv" TexturesUV,
# "point" point lights.  Options after "/" in the source: "mat" non-default materials and background, "tex384" a 384 x 384 texture (more
# texels per backward tile than TexAcc holds), "dim" the second image lit at 1 / 100 of the first with no ambient or specular term and the upstream gradient of sum(rgb^2) / 2, "small" a mesh of a few
# pixels, "poseN" the N-th pose after the one the case's shape gives (render_contract_admits decides when a case needs another).
#   * face ids: bit for bit those of oracle/raster_oracle.c on the float32 projection (the discontinuity stays a float32 target);
#   * everything behind them -- pixels and all gradients -- against render_oracle.render in FLOAT64 with those ids imposed (p2f=), per
#     image and per quantity:  err <= min(c (sqrt(L) + K), cap) max|ref of that image|,  L the number of summed terms (aa^2 for a pixel,
#     the largest number of samples feeding one vertex / one texel / the light for a gradient), K the conditioning of the image's worst
#     winning face taken from the float64 reference (render_contract_cond); cap = what render_case / render_uv_case accept;
#   * alpha = hits / aa^2 exactly; a pixel without a hit = the sum of aa^2 background samples over aa^2, exactly; a second forward gives
#     the same bits, a second backward on the same workspace the first one's values to rounding (float atomics);
#   * outputs prefilled with NaN, canaries around every output and behind the render_workspace_bytes(h, B) bytes of workspace.
# No NaN / Inf / Z == 0 vertex goes in (include/hifihr.h: outside the contract).
# ------------------------------------------------------------------------------------------------
RENDER_CONTRACT_ENTRIES = ("renderer_create", "renderer_set_light_mode", "renderer_set_uv", "renderer_destroy", "render_workspace_bytes",
                           "render_uv_scratch_bytes", "render_fwd", "render_bwd", "render_fwd_uv", "render_bwd_uv")
RENDER_MAX_IMAGE = 720                # include/hifihr.h: the largest image_size hifihr_renderer_create accepts
# kind: (c, cap) as in LAYER_CONTRACT_C: c = 4 x the worst err / ((sqrt(L) + K) max|ref|) of render_contract_ref run in float32 (plain fp32
# torch on the CPU) against its float64 run over RENDER_CASES of tests/test_hostsim_render_contract.py (tools/render_contract_c.py prints
# them); cap = the tolerance render_case / render_uv_case use for the same quantity, relative to max|ref| (pixels: 2e-5 absolute on
# values of the order of 1).
RENDER_CONTRACT_C = {
    "render_rgb": (5.1e-7, 2e-5),     # 1.27e-07 x 4      rgb, L = aa^2                                    (render_case atol 2e-5)
    #                                                     (+ render_device_allowance on the GPU: the approximate reciprocals of its forward)
    "render_gv": (1.7e-6, 2e-3),      # 4.20e-07 x 4      gverts, L = samples on the faces of one vertex     (render_case 2e-3)
    "render_gc": (3.4e-7, 2e-3),      # 8.47e-08 x 4      gvcolors, same L                                   (render_case 2e-3)
    "render_gmap": (1.7e-6, 3e-3),    # 4.14e-07 x 4      gmaps, L = samples with a tap on one texel         (render_uv_case 3e-3)
    "render_glc": (2.7e-6, 2e-3),     # 6.85e-07 x 4      glight_color, L = covered samples of the image     (render_case 2e-3)
    "render_gld": (2.0e-6, 2e-3),     # 4.89e-07 x 4      glight_dir, same L                                 (render_case 2e-3)
}
RENDER_CONTRACT_KINDS = tuple(RENDER_CONTRACT_C)
LAYER_CONTRACT_C.update(RENDER_CONTRACT_C)
RENDER_LAUNCHED = set()               # kernels the emulator launched under the renderer cases (the reach test reads it)
RENDER_COUNTS = {"merges": 0, "resolves": 0, "strips": 0, "slotless": 0, "vertex_overflow": 0, "texel_overflow": 0}
RENDER_NONDEFAULT = dict(ambient=(0.3, 0.5, 0.25), mat_diffuse=(0.9, 0.6, 0.7), specular=(0.1, 0.04, 0.2), shininess=12.0,
                         background=(0.3, 0.75, 0.1))
RENDER_DIM = dict(ambient=(0.0, 0.0, 0.0), mat_diffuse=(0.8, 0.8, 0.8), specular=(0.0, 0.0, 0.0), shininess=30.0, background=(0.0, 0.0, 0.0))
_RENDER_MEMO = {}


def _render_drain(lib, device):
    """Launch log and path counters of the emulator since the last look, added to RENDER_LAUNCHED / RENDER_COUNTS (nothing on a GPU)."""
    if device != "cpu":
        return None
    import ctypes
    names = [k.replace(" ", "") for k in launch_log(lib)]
    RENDER_LAUNCHED.update(names)
    f4, b2 = (ctypes.c_int * 4)(), (ctypes.c_int * 2)()
    lib.c.hifihr_hostsim_render_fwd3_counts(f4, 1)
    lib.c.hifihr_hostsim_render_bwd_counts(b2, 1)
    for k, v in zip(RENDER_COUNTS, list(f4) + list(b2)):
        RENDER_COUNTS[k] += v
    return names


def _render_refuses(entry, lib, device, call, guards, what):
    """HIFIHR_EINVAL, every output and guard untouched, nothing launched."""
    _render_drain(lib, device)
    _refuses(entry, call, guards, f"{entry}: {what}")
    left = _render_drain(lib, device)
    assert not left, f"{entry}: {what}: refused but launched {left}"


def icosahedron():
    """12 vertices on the unit sphere, 20 faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
                  (-t, 0, -1), (-t, 0, 1)], dtype=np.float32)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int32)
    return v / np.linalg.norm(v[0]), f


def _render_tables():
    if "tables" not in _RENDER_MEMO:
        from hifihr_amd.mano_tables import synthetic_mano_tables
        _RENDER_MEMO["tables"] = synthetic_mano_tables(0)
    return _RENDER_MEMO["tables"]


def render_contract_inputs(case):
    """The inputs of one case, float32, and the float32 oracle's face ids for them ("p2f"); memoised: the runner, the detection test and
    the measurement share them."""
    if case in _RENDER_MEMO:
        return _RENDER_MEMO[case]
    from oracle import render_oracle as ro
    scene, src, B, H, aa, mode = case
    src, *opts = src.split("/")
    seed = 1000 + 7 * H + 3 * aa + B + len(scene) + sum(int(o[4:]) for o in opts if o.startswith("pose"))
    gen = torch.Generator().manual_seed(seed)
    hv, _, cam, lc, ld = make_render_inputs(_render_tables(), B, seed, H)
    centre = hv.mean(1, keepdim=True)                                     # [B,1,3]: in front of the camera, z in 0.6 .. 0.8
    fx = cam[:, 0].view(B, 1)
    if src == "mano":
        verts, faces = hv, np.asarray(_render_tables().faces, dtype=np.int32)
    elif src == "ico":
        iv, faces = icosahedron()
        verts = torch.from_numpy(iv)[None] * (0.006 if "small" in opts else 0.07) + centre
    elif src == "skin":
        mv, faces = nimble_sized_mesh(B, seed)
        verts = mv + centre
    elif src == "one":
        faces = np.array([[0, 1, 2]], dtype=np.int32)
        verts = torch.tensor([[-0.08, -0.05, 0.0], [0.09, -0.04, 0.05], [0.0, 0.1, -0.03]])[None] * (0.1 if "small" in opts else 1.0) + centre
    elif src == "quads96":
        # 96 quads, each larger than the image, at distinct depths and with their own small tilt (the planes cross: the winner changes
        # from sample to sample); quads 11 and 51 are copies of 10 and 50: coplanar at identical z, the lower face index wins
        Q = 96
        corners = torch.tensor([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])
        order = torch.randperm(Q, generator=gen).float()
        order[[10, 50]] = 0.0                                             # (the copied quads in front: their ties decide samples)
        z = 0.5 + 0.004 * order
        tilt = 0.05 * (torch.rand(Q, 4, generator=gen) - 0.5)
        tilt[50] = -tilt[10]
        zq = z.view(Q, 1) + tilt
        xy = corners.view(1, 4, 2) * (0.4 + 0.04 * torch.rand(Q, 4, 2, generator=gen)) * zq.view(Q, 4, 1)      # (no two diagonals coincide)
        quad = torch.cat([xy, zq.view(Q, 4, 1)], -1)
        quad[11], quad[51] = quad[10], quad[50]
        verts = quad.reshape(1, 4 * Q, 3).repeat(B, 1, 1)
        base = 4 * np.arange(Q, dtype=np.int32)[:, None]
        faces = np.concatenate([base + np.array([[0, 1, 2]]), base + np.array([[0, 2, 3]])], 1).reshape(-1, 3).astype(np.int32)
        cam = cam.clone(); cam[:, 2:] = 0.0
    elif src == "tris":
        # large triangles with one or two vertices BEHIND the camera plane (Z negative and finite, never 0: NDC coordinates huge but
        # finite; per sample pz >= 0 decides), next to one wholly in front
        # (without clipping, the interpolated depth is z0 z1 z2 / denom: ONE vertex behind the camera makes it negative wherever the
        # corrected barycentrics are positive -- faces 0 and 3 cover nothing, after the full arithmetic on every sample of their boxes --
        # and with TWO behind the covered samples are those of the NDC bounding box in the cone beyond the front vertex: face 1 is laid
        # out in NDC with that vertex inside the image; face 3's vertex at Z = -1e-3 projects hundreds of image widths away)
        ndcz = torch.tensor([[[-0.8, -0.7, 0.8], [0.8, 0.9, 0.8], [0.1, -0.1, -0.5]],
                             [[0.1, -0.1, 0.6], [-0.9, -0.8, -0.3], [0.9, 0.9, -0.5]]])
        cam = cam.clone(); cam[:, 2:] = 0.0
        laid = torch.stack([ndcz[..., 0].view(1, 2, 3) * ndcz[..., 2] / cam[:, 0].view(B, 1, 1), ndcz[..., 1].view(1, 2, 3) * ndcz[..., 2] / cam[:, 1].view(B, 1, 1),
                            ndcz[..., 2].view(1, 2, 3).expand(B, -1, -1)], -1)
        tri = torch.tensor([[[-0.25, -0.1, 1.0], [0.2, -0.15, 1.1], [0.05, 0.2, 0.9]],
                            [[0.1, 0.1, 0.7], [-0.15, 0.12, 0.75], [0.0, -0.1, -1e-3]]])
        verts = torch.cat([laid.reshape(B, 6, 3), tri.reshape(1, 6, 3).repeat(B, 1, 1)], 1)
        verts = verts * (1.0 + 0.1 * torch.arange(B, dtype=torch.float32).view(B, 1, 1))
        faces = np.arange(12, dtype=np.int32).reshape(4, 3)
    elif src == "odd":
        # f1 shares all three vertices with f0 (a tie at every sample: f0 wins); f3 repeats a vertex and f4 is collinear (zero area);
        # vertex 9 belongs to no face (zero normal sum: normalize's epsilon path, zero gradient)
        verts = torch.tensor([[-0.1, -0.08, 0.0], [0.1, -0.07, 0.02], [0.0, 0.1, -0.02], [-0.05, -0.1, 0.05], [0.12, 0.0, 0.06],
                              [-0.08, 0.09, 0.04], [-0.1, 0.0, -0.05], [0.0, 0.0, -0.05], [0.1, 0.0, -0.05], [0.02, 0.03, -0.1]])[None] + centre
        faces = np.array([[0, 1, 2], [0, 1, 2], [3, 4, 5], [3, 3, 4], [6, 7, 8]], dtype=np.int32)
    elif src == "confetti196":
        # 14 x 14 disjoint small triangles (V = 3 F = 588 > the 512 slots of BwdAcc) inside ONE 16 x 16-pixel backward tile; inradius
        # 0.034 NDC > half the diagonal of a sample cell at S = 48 (0.0295): every triangle covers at least one sample
        n = 14
        c = (torch.arange(n, dtype=torch.float32) + 0.5) / n * 2 - 1
        cy, cx = torch.meshgrid(c, c, indexing="ij")
        ang = torch.rand(n * n, 1, generator=gen) * 6.2832 + torch.tensor([[0.0, 2.0944, 4.1888]])
        ndc = torch.stack([cx.reshape(-1, 1) + 0.068 * torch.cos(ang), cy.reshape(-1, 1) + 0.068 * torch.sin(ang)], -1)     # [F,3,2]
        zz = 0.6 + 0.2 * torch.rand(n * n, 3, generator=gen)
        cam = cam.clone(); cam[:, 2:] = 0.0
        v1 = torch.cat([ndc * zz.unsqueeze(-1), zz.unsqueeze(-1)], -1).reshape(1, 3 * n * n, 3).repeat(B, 1, 1)
        verts = torch.cat([v1[..., :1] / cam[:, 0].view(B, 1, 1), v1[..., 1:2] / cam[:, 1].view(B, 1, 1), v1[..., 2:]], -1)
        faces = np.arange(3 * n * n, dtype=np.int32).reshape(-1, 3)
    else:
        raise ValueError(src)
    verts = verts.expand(B, -1, -1).clone() if verts.shape[0] != B else verts.clone()
    if scene == "offscreen":
        # image k: across the left / right / top / bottom border, wholly outside, the principal point far off-centre (the mesh moved with it,
        # half an image off); an NDC shift of s is a move of s Z / fx in view space
        shifts = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (4.0, 0.3), (0.5, -0.4)]
        cam = cam.clone()
        for b in range(B):
            sx, sy = shifts[b % 6]
            if b % 6 == 5:
                cam[b, 2], cam[b, 3] = 1.7, -1.3
            zc = float(centre[b, 0, 2])
            verts[b, :, 0] += (sx - float(cam[b, 2]) * (b % 6 == 5)) * zc / float(cam[b, 0])
            verts[b, :, 1] += (sy - float(cam[b, 3]) * (b % 6 == 5)) * zc / float(cam[b, 1])
    V = verts.shape[1]
    if scene == "degenerate":
        ld = ld.clone(); ld[0] = 0.0                                      # a zero light direction
        lc = lc.clone(); lc[0] = torch.tensor([-1.0, 1.0, 1.0])          # the ends of the hardtanh range
        if B > 1:
            lc[1] = torch.tensor([1.0, -1.0, -1.0])
    consts = dict(ambient=(0.5, 0.5, 0.5), mat_diffuse=(0.8, 0.8, 0.8), specular=(0.04, 0.04, 0.04), shininess=30.0, background=(1.0, 1.0, 1.0))
    if "mat" in opts:
        consts = dict(RENDER_NONDEFAULT)
    if "dim" in opts:
        consts = dict(RENDER_DIM)
        lc = lc.abs() + 0.2
        lc[1] = lc[0] * 0.01
        ld = ld.clone(); ld[1] = ld[0]
        verts[1] = verts[0]
        cam = cam.clone(); cam[1] = cam[0]
    if mode == "point":
        lc = torch.full((B, 3), 0.3)
        ld = torch.tensor([[0.0, 1.0, 0.0]]).repeat(B, 1)
        if B > 1:
            ld[1] = torch.tensor([0.1, -0.2, 0.3])
    inp = {"case": case, "verts": verts.contiguous(), "faces": faces, "V": V, "F": len(faces), "cam": cam.contiguous(), "lc": lc.contiguous(),
           "ld": ld.contiguous(), "consts": consts, "point": mode == "point", "uv": None, "vcol": None, "B": B, "H": H, "aa": aa}
    if mode == "uv":
        TH, TW = (384, 384) if "tex384" in opts else (24, 40)
        fu, vu = synthetic_uv_tables(faces, V, seed)
        # a smooth image (a skin texture is one): under a coarse raster a random texture is noise -- one sliver's barycentrics, off by
        # 1e-5, move its sample across texels that differ by 1 -- and no float32 evaluation is within 2e-5 of the float64 pixel there
        yy, xx = torch.meshgrid(torch.arange(TH) / TH, torch.arange(TW) / TW, indexing="ij")
        ph = torch.rand(B, 1, 1, 3, generator=gen) * 6.2832
        fr = torch.tensor([5.0, 3.0, 4.0]).view(1, 1, 1, 3)
        maps = 0.5 + 0.4 * torch.sin(fr * xx[None, :, :, None] + (8.0 - fr) * yy[None, :, :, None] + ph)
        inp["uv"] = (fu, vu, maps.contiguous())
    else:
        inp["vcol"] = 0.3 + 0.6 * torch.rand(*((V, 3) if mode == "shared" else (B, V, 3)), generator=gen)
    w = torch.randn(B, 4, H, H, generator=gen)
    if "dim" in opts:
        w[1] = w[0]
    inp["w"] = w
    vndc = ro.project_ndc(inp["verts"], inp["cam"])
    assert bool(torch.isfinite(vndc).all()) and bool(torch.isfinite(inp["verts"]).all())
    inp["p2f"] = ro.rasterize(vndc, torch.as_tensor(faces).long(), H * aa)[0]
    if "dim" in opts:                                                     # the gradient of sum(rgb^2) / 2: 1e-4 of the first image's in the second
        r32, _ = ro.render(inp["verts"], inp["vcol"], inp["cam"], inp["lc"], inp["ld"], torch.as_tensor(faces).long(), image_size=H, aa=aa,
                           consts=ro.ShadeConsts(**consts), p2f=inp["p2f"])
        w = r32.clone()
        w[:, 3] = 0
        inp["w"] = w
    inp["w"] = (w * render_kink_free(inp).view(B, 1, H, H)).contiguous()
    _RENDER_MEMO[case] = inp
    return inp


RENDER_KINK_MARGIN = (1e-4, 1e-2)      # |cosang|, |d| of the unit vectors; distance of a texel coordinate from an integer


def render_kink_free(inp):
    """[B,H,H] 0 / 1: pixels that take an upstream gradient.  The shading has kinks -- relu(cosang), the specular lobe's relu(d) under its
    cosang > 0 mask, the bilinear quad floor(ix), floor(iy) and the border clamp of the texture -- where the VALUE is continuous and the
    GRADIENT jumps: a sample within rounding of one takes either side in float32, and no float32 evaluation, torch's included, can be held
    to the float64 gradient there (as for visibility, which the imposed face ids take out).  A pixel with a covered sample inside
    RENDER_KINK_MARGIN of a kink, judged on the float64 reference, gets no upstream gradient; its pixel VALUE is compared like every other."""
    from oracle import render_oracle as ro
    B, H, aa, dt = inp["B"], inp["H"], inp["aa"], torch.float64
    aux = {}
    tuv = None if inp["uv"] is None else (inp["uv"][2].to(dt), torch.from_numpy(inp["uv"][0]).long(), torch.from_numpy(inp["uv"][1]).to(dt))
    vc = None if inp["vcol"] is None else inp["vcol"].to(dt)
    ro.render(inp["verts"].to(dt), vc, inp["cam"].to(dt), inp["lc"].to(dt), inp["ld"].to(dt), torch.as_tensor(inp["faces"]).long(), image_size=H,
              aa=aa, consts=ro.ShadeConsts(**inp["consts"]), point_lights=inp["point"], textures_uv=tuv, p2f=inp["p2f"], aux=aux)
    m_cos, m_tex = RENDER_KINK_MARGIN
    near = (aux["cosang"].abs() < m_cos) | ((aux["cosang"] > 0) & (aux["d"].abs() < m_cos))
    if tuv is not None:
        TH, TW = tuv[0].shape[1], tuv[0].shape[2]
        for k, T in ((0, TW), (1, TH)):
            t = aux["uv"][..., k] * (T - 1)
            near = near | ((t - t.round()).abs() < m_tex) | (t < m_tex) | (t > T - 1 - m_tex)
    near = near & aux["hit"]
    return 1.0 - near.view(B, H, aa, H, aa).any(4).any(2).float()


def render_drop_choice(inp, ref):
    """The contributions the detection test removes: the covered sample of the LAST image that has one whose pixel carries the largest
    upstream gradient, and the first corner of the face it shows."""
    hit = inp["p2f"] >= 0
    if not hit.any():
        return None
    b = max(k for k in range(inp["B"]) if hit[k].any())
    aa = inp["aa"]
    wpix = inp["w"][b, :3].abs().sum(0).numpy().repeat(aa, 0).repeat(aa, 1)
    y, x = np.unravel_index(int(np.argmax(np.where(hit[b], wpix, -1.0))), hit[b].shape)
    return b, int(y), int(x), int(inp["p2f"][b, y, x])


def render_contract_ref(inp, dt=torch.float64, drop=None):
    """The checked quantities, per image, of render_oracle.render run in `dt` on the float32 run's face ids: "rgb" [B,3,H,H], "alpha",
    "gverts", "gvcolors" (vertex colours) or "gmaps" (UV), "glight_color", "glight_dir" for the loss sum(rgba * w).
    drop removes ONE contribution (render_drop_choice gives b, y, x, f):
      ("sample", b, y, x)   that sample from its pixel's aa x aa block -- and with it from every gradient sum it feeds;
      ("normal", f, k)      face f from the normal sum of its corner k's vertex;
      ("tap", b, y, x)      the largest of that sample's bilinear taps from the texture gradient."""
    from oracle import render_oracle as ro
    B, H, aa = inp["B"], inp["H"], inp["aa"]
    leaf = lambda t: t.to(dt).clone().requires_grad_(True)
    v, lc, ld = leaf(inp["verts"]), leaf(inp["lc"]), leaf(inp["ld"])
    faces = torch.as_tensor(inp["faces"]).long()
    consts = ro.ShadeConsts(**inp["consts"])
    sw = skip = None
    if drop is not None and drop[0] == "sample":
        sw = torch.ones(B, H * aa, H * aa, dtype=dt)
        sw[drop[1], drop[2], drop[3]] = 0
    if drop is not None and drop[0] == "normal":
        skip = (drop[1], drop[2])
    if inp["uv"] is not None:
        tex = leaf(inp["uv"][2])
        tuv = (tex, torch.from_numpy(inp["uv"][0]).long(), torch.from_numpy(inp["uv"][1]).to(dt))
        rgba, _ = ro.render(v, None, inp["cam"].to(dt), lc, ld, faces, image_size=H, aa=aa, consts=consts, textures_uv=tuv, p2f=inp["p2f"],
                            sample_weight=sw, normal_skip=skip)
    else:
        vc = inp["vcol"] if inp["vcol"].dim() == 3 else inp["vcol"].unsqueeze(0).expand(B, -1, -1)
        tex = leaf(vc)
        rgba, _ = ro.render(v, tex, inp["cam"].to(dt), lc, ld, faces, image_size=H, aa=aa, consts=consts, point_lights=inp["point"],
                            p2f=inp["p2f"], sample_weight=sw, normal_skip=skip)
    (rgba * inp["w"].to(dt)).sum().backward()
    z = lambda t: t.grad.detach() if t.grad is not None else torch.zeros_like(t)
    out = {"rgb": rgba.detach()[:, :3], "alpha": rgba.detach()[:, 3], "gverts": z(v), "glight_color": z(lc),
           "glight_dir": torch.zeros_like(ld) if inp["point"] else z(ld)}
    out["gmaps" if inp["uv"] is not None else "gvcolors"] = z(tex)
    if drop is not None and drop[0] == "tap":
        one = torch.zeros(B, H * aa, H * aa, dtype=dt)
        one[drop[1], drop[2], drop[3]] = 1
        t2 = leaf(inp["uv"][2])
        r2, _ = ro.render(inp["verts"].to(dt), None, inp["cam"].to(dt), inp["lc"].to(dt), inp["ld"].to(dt), faces, image_size=H, aa=aa, consts=consts,
                          textures_uv=(t2, tuv[1], tuv[2]), p2f=inp["p2f"], sample_weight=one)
        (r2 * inp["w"].to(dt)).sum().backward()
        g1 = t2.grad[drop[1]]                                             # the sample's (up to) four taps
        ty, tx = np.unravel_index(int(g1.abs().sum(-1).argmax()), g1.shape[:2])
        out["gmaps"] = out["gmaps"].clone()
        out["gmaps"][drop[1], ty, tx] -= g1[ty, tx]
    return out


def render_contract_cond(inp):
    """Per image: (L of a vertex gradient, L of a light gradient, L of a texel gradient, K).  L: the largest number of samples on the faces
    of one vertex / covered samples of the image / samples with a bilinear tap on one texel.  K: the conditioning of the barycentrics of the
    image's worst WINNING face, from the float64 reference: max(1, |x|, |y|) (dx + dy) / |area| of its NDC coordinates, bounding box and
    edge-function area (float32 holds a projected vertex to 2^-24 of its coordinate; the barycentrics move by that over the triangle's
    height, area / extent: about 2 / extent for a well-shaped face, large for a sliver) times the largest sum |bary_k| of a covered sample (1 in front of the camera; the perspective correction cancels when a
    vertex lies behind it), times -- TexturesUV -- 1 + (T - 1) max |step between neighbouring texels|, what an error of uv is worth in
    the texel.  0 where nothing is covered."""
    from oracle import render_oracle as ro
    faces = torch.as_tensor(inp["faces"]).long()
    vndc = ro.project_ndc(inp["verts"].double(), inp["cam"].double())
    p2f = torch.from_numpy(inp["p2f"])
    bary, hit, idx = ro.differentiable_bary(vndc, faces, p2f)
    out = []
    for b in range(inp["B"]):
        ids = inp["p2f"][b][inp["p2f"][b] >= 0]
        if ids.size == 0:
            out.append((1, 1, 1, 0.0))
            continue
        cnt_f = np.bincount(ids, minlength=inp["F"])
        cnt_v = np.zeros(inp["V"], dtype=np.int64)
        for k in range(3):
            np.add.at(cnt_v, inp["faces"][:, k], cnt_f)
        win = torch.from_numpy(np.unique(ids)).long()
        fv = vndc[b][faces[win]]                                           # [n,3,3]
        ext = (fv[..., 0].amax(1) - fv[..., 0].amin(1)) + (fv[..., 1].amax(1) - fv[..., 1].amin(1))
        area = ro._edge(fv[:, 2, 0], fv[:, 2, 1], fv[:, 0, 0], fv[:, 0, 1], fv[:, 1, 0], fv[:, 1, 1]).abs()
        cmax = fv[..., :2].abs().amax((1, 2)).clamp(min=1.0)
        K = float((cmax * ext / area).max()) * float(bary[b][hit[b]].abs().sum(-1).max())
        Lt = 1
        if inp["uv"] is not None:
            fu, vu, maps = inp["uv"]
            TH, TW = maps.shape[1], maps.shape[2]
            uv = (bary[b][hit[b]].unsqueeze(-1) * torch.from_numpy(vu).double()[torch.from_numpy(fu).long()][idx[b][hit[b]]]).sum(-2)
            ix = (uv[:, 0] * (TW - 1)).clamp(0, TW - 1); iy = (uv[:, 1] * (TH - 1)).clamp(0, TH - 1)
            x0, y0 = ix.floor().long(), iy.floor().long()
            x1, y1 = (x0 + 1).clamp(max=TW - 1), (y0 + 1).clamp(max=TH - 1)
            taps = torch.stack([y0 * TW + x0, y0 * TW + x1, y1 * TW + x0, y1 * TW + x1], 1)
            Lt = int(torch.bincount(taps.reshape(-1), minlength=TH * TW).max())
            # the texel moves with uv at (T - 1) x the step between neighbouring texels: an error of the barycentrics is worth that much more
            m = maps[b].double()
            K *= 1.0 + max(float((m[:, 1:] - m[:, :-1]).abs().max()) * (TW - 1), float((m[1:] - m[:-1]).abs().max()) * (TH - 1))
        out.append((max(1, int(cnt_v.max())), int(ids.size), Lt, K))
    return out


def render_contract_ref_once(case):
    """(float64 reference, conditioning) of a case: computed once, shared by the runner and the detection tests, left unchanged."""
    key = ("ref", case)
    if key not in _RENDER_MEMO:
        inp = render_contract_inputs(case)
        _RENDER_MEMO[key] = (render_contract_ref(inp), render_contract_cond(inp))
    return _RENDER_MEMO[key]


def render_bound(kind, ref, L, K, approx=0.0):
    """min(c (sqrt(L) + K) + approx, cap) max|ref|: layer_bound with cond = K max|ref|, and never above the older case's tolerance.
    approx: render_device_allowance (the device's forward only)."""
    c, cap = LAYER_CONTRACT_C[kind]
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return min(layer_bound(kind, ref, L, K * scale) + approx * scale, cap * scale)


def render_device_allowance(inp, device):
    """What the DEVICE build's forward may add to the emulator's error, relative to max|rgb| -- not measured on the kernel: from the
    documented accuracy of the instructions shade_fwd_fast and resolve_shade2 use where the emulator divides and takes square roots
    exactly.  V_RCP_F32 and V_RSQ_F32 are accurate to 1 ulp (2^-23 relative; CDNA ISA guide).  Along one sample: rcp(area) and rcp(denom)
    put 2 ulp on the barycentrics and so on P, N and the texel; rsq on the normal, the view vector and -- point lights -- the light
    vector put 1 ulp on each unit vector.  Diffuse term: texel (2) x cosang (2 + 1 + 1) = 6 ulp of (ambient + diffuse) texel <= max|rgb|.
    Specular term: d = view . reflection carries the same 6 ulp, the power multiplies a relative error by the shininess: 6 s ulp of
    specular d^s <= max(specular)."""
    if device == "cpu":
        return 0.0
    return 2.0 ** -23 * (6.0 + 6.0 * inp["consts"]["shininess"] * max(inp["consts"]["specular"]))


def render_passes(kind, got, ref, L, K):
    return layer_err(got, ref) <= render_bound(kind, ref, L, K)


def _render_close(entry, kind, got, ref, L, K, what, approx=0.0):
    err, bound = layer_err(got, ref), render_bound(kind, ref, L, K, approx)
    _tail_ratio(entry, err, bound)
    assert err <= bound, f"{what}: err {err:.3e} vs bound {bound:.3e} (kind {kind}, max|ref| {float(ref.abs().max()):.3e}, L {L}, K {K:.3g})"


def render_quantities(inp):
    """(name of the reference's quantity, kind, which L of render_contract_cond) of the backward."""
    tex = ("gmaps", "render_gmap", 2) if inp["uv"] is not None else ("gvcolors", "render_gc", 0)
    return [("gverts", "render_gv", 0), tex, ("glight_color", "render_glc", 1), ("glight_dir", "render_gld", 1)]


def render_legacy_passes(got, ref, tol=2e-3):
    """render_case's criterion: ONE maximum over the batch and all elements."""
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-12) < tol


def render_contract_float32_errors(case):
    """[(image, kind, L, K, err, max|ref|)] of the reference run in float32 (plain torch on the CPU) against its float64 run; once per
    case: the measurement of RENDER_CONTRACT_C and the admission of a case share it."""
    key = ("f32", case)
    if key not in _RENDER_MEMO:
        inp = render_contract_inputs(case)
        (r64, cond), r32 = render_contract_ref_once(case), render_contract_ref(inp, torch.float32)
        rows = []
        for b in range(inp["B"]):
            for name, kind, L in [("rgb", "render_rgb", inp["aa"] ** 2)] + [(n, k, cond[b][i]) for n, k, i in render_quantities(inp)]:
                scale = float(r64[name][b].abs().max())
                if scale > 0:
                    rows.append((b, kind, L, cond[b][3], layer_err(r32[name][b], r64[name][b]), scale))
        _RENDER_MEMO[key] = rows
    return _RENDER_MEMO[key]


def render_contract_measure(cases):
    """The float32 run of the reference against its float64 run: kind -> worst err / ((sqrt(L) + K) max|ref|) (x 4 = RENDER_CONTRACT_C)."""
    worst = {k: 0.0 for k in RENDER_CONTRACT_KINDS}
    for case in cases:
        for b, kind, L, K, err, scale in render_contract_float32_errors(case):
            worst[kind] = max(worst[kind], err / ((L ** 0.5 + K) * scale))
    return worst


RENDER_ADMIT = 0.5                     # the share of a cap the float32 run of the reference may use up on a case of the lists


def render_contract_admits(case):
    """What keeps a case OUT of the lists: [(image, kind, err / max|ref|, cap)] where the reference's own float32 run is further than
    RENDER_ADMIT x cap from its float64 run.  The caps are the older cases' tolerances and do not grow with the conditioning: on a pose
    whose winning sliver costs plain float32 arithmetic most of a cap, a correct float32 kernel that merely rounds elsewhere -- another
    summation order, a reciprocal for a division -- cannot be held to it, and a failure there says nothing about the kernel.  Two float32
    evaluations with independent rounding are up to twice one's error apart, hence the half.  Decided on the reference alone, never on a
    kernel's output; such a case takes its next pose ("poseN")."""
    return [(b, kind, err / scale, LAYER_CONTRACT_C[kind][1]) for b, kind, L, K, err, scale in render_contract_float32_errors(case)
            if err > RENDER_ADMIT * LAYER_CONTRACT_C[kind][1] * scale]


def render_contract_case(lib, device, case):
    """One accepted case through create / set_light_mode / set_uv / workspace_bytes / fwd / bwd / destroy (module comment above)."""
    inp = render_contract_inputs(case)
    ref, cond = render_contract_ref_once(case)
    B, H, aa, V, F_ = inp["B"], inp["H"], inp["aa"], inp["V"], inp["F"]
    S, uv, what = H * aa, inp["uv"] is not None, str(case)
    fwd_e, bwd_e = ("render_fwd_uv", "render_bwd_uv") if uv else ("render_fwd", "render_bwd")
    _render_drain(lib, device)
    h = lib.renderer_create(inp["faces"], V, image_size=H, aa=aa, **inp["consts"])
    _layer_log("renderer_create", True)
    try:
        lib.renderer_set_light_mode(h, inp["point"])
        _layer_log("renderer_set_light_mode", True)
        assert lib.render_uv_scratch_bytes(h, B) == 0
        _layer_log("render_uv_scratch_bytes", True)
        if uv:
            lib.renderer_set_uv(h, inp["uv"][0], inp["uv"][1])
            _layer_log("renderer_set_uv", True)
        nws = lib.render_workspace_bytes(h, B)
        assert nws > 0 and lib.render_workspace_bytes(h, B + 1) >= nws >= lib.render_workspace_bytes(h, max(B - 1, 0))
        _layer_log("render_workspace_bytes", True)
        G = Guards(device)
        ws = G.out(nws, dtype=torch.uint8, fill=0xFF)
        dv, dcam, dlc, dld, dw = (G.inp(inp[k]) for k in ("verts", "cam", "lc", "ld", "w"))
        dtex = G.inp(inp["uv"][2] if uv else inp["vcol"])
        rgba = [G.out(B, 4, H, H, fill=float("nan")) for _ in range(2)]
        fid = [G.out(B, S, S, dtype=torch.int32, fill=_POISON[torch.int32]) for _ in range(2)]

        def fwd(k):
            if uv:
                lib.render_fwd_uv(h, dv, dtex, dcam, dlc, dld, rgba[k], fid[k], None, ws)
            else:
                lib.render_fwd(h, dv, dtex, dcam, dlc, dld, rgba[k], fid[k], ws)
            G.intact(f"{what}: forward {k}")

        fwd(0)
        got_fid = fid[0].cpu().numpy()
        assert np.array_equal(got_fid, inp["p2f"]), f"{what}: {int((got_fid != inp['p2f']).sum())} face ids differ from the float32 oracle's"
        _layer_log(fwd_e, True, 0.0)
        got = rgba[0].cpu()
        hits = torch.from_numpy((inp["p2f"] >= 0).reshape(B, H, aa, H, aa).sum((2, 4)).astype(np.float32))
        assert torch.equal(got[:, 3], hits / np.float32(aa * aa)), f"{what}: alpha is not the hit fraction"
        bgsum = np.zeros(3, dtype=np.float32)
        for _ in range(aa * aa):
            bgsum = bgsum + np.asarray(inp["consts"]["background"], dtype=np.float32)
        bgpix = torch.from_numpy(bgsum / np.float32(aa * aa))
        empty = hits == 0
        assert bool((got[:, :3].permute(0, 2, 3, 1)[empty] == bgpix).all()), f"{what}: a pixel without a hit is not the background"
        for b in range(B):
            _render_close(fwd_e, "render_rgb", got[b, :3], ref["rgb"][b], aa * aa, cond[b][3], f"{what}: rgb of image {b}",
                          render_device_allowance(inp, device))
        fwd(1)
        assert torch.equal(fid[1], fid[0]) and torch.equal(rgba[1].view(torch.int32), rgba[0].view(torch.int32)), f"{what}: a second forward differs"
        _layer_log(fwd_e, True, 0.0)

        tshape = tuple(inp["uv"][2].shape) if uv else (B, V, 3)
        first = None
        for rep in range(2):                                              # the second run finds the accumulators dirty (render_ws_mark_clean)
            gv, glc, gld = G.out(B, V, 3, fill=float("nan")), G.out(B, 3, fill=float("nan")), G.out(B, 3, fill=float("nan"))
            gt = G.out(*tshape, fill=0.0 if uv else float("nan"))         # gmaps is ACCUMULATED onto the caller's zeros
            if uv:
                lib.render_bwd_uv(h, dv, dtex, dcam, dlc, dld, fid[0], dw, None, None, gv, gt, glc, gld, ws)
            else:
                lib.render_bwd(h, dv, dcam, dlc, dld, fid[0], dw, gv, gt, glc, gld, ws)
            G.intact(f"{what}: backward {rep}")
            outs = {"gverts": gv, "gmaps" if uv else "gvcolors": gt, "glight_color": glc, "glight_dir": gld}
            for b in range(B):
                for name, kind, li in render_quantities(inp):
                    _render_close(bwd_e, kind, outs[name][b], ref[name][b], cond[b][li], cond[b][3], f"{what}: {name} of image {b} (run {rep})")
            if inp["point"]:
                assert float(gld.abs().max()) == 0.0, f"{what}: point lights: glight_dir is not zero"
            if first is None:
                first = {k: t.cpu().clone() for k, t in outs.items()}
            else:
                for k, t in outs.items():
                    for b in range(B):
                        scale = float(first[k][b].abs().max())
                        assert float((t[b].cpu() - first[k][b]).abs().max()) <= 1e-5 * scale, f"{what}: second backward on one workspace: {k} of image {b} differs"
        if not uv:                                                        # gvcolors NULL: the other gradients as before
            gv2, glc2, gld2 = G.out(B, V, 3, fill=float("nan")), G.out(B, 3, fill=float("nan")), G.out(B, 3, fill=float("nan"))
            lib.render_bwd(h, dv, dcam, dlc, dld, fid[0], dw, gv2, None, glc2, gld2, ws)
            G.intact(f"{what}: backward without gvcolors")
            for b in range(B):
                _render_close(bwd_e, "render_gv", gv2[b], ref["gverts"][b], cond[b][0], cond[b][3], f"{what}: gverts of image {b} with gvcolors NULL")
        _render_drain(lib, device)
        return True
    finally:
        lib.renderer_destroy(h)
        _layer_log("renderer_destroy", True)


def render_refusal_case(lib, device, entry):
    """Every refused call of one entry -- HIFIHR_EINVAL, outputs and guards untouched, nothing launched -- and its accepted edge calls
    (B == 0: a no-op; the byte queries).  True when the entry has refused calls at all."""
    import ctypes
    case = ("refusals", "ico", 2, 8, 2, "uv")
    inp = render_contract_inputs(case)
    B, H, aa, V, F_ = inp["B"], inp["H"], inp["aa"], inp["V"], inp["F"]
    S = H * aa
    fu, vu, maps = inp["uv"]
    TH, TW = maps.shape[1], maps.shape[2]
    c_int, c_float, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    np_p = lambda a: vp(a.ctypes.data) if a is not None else vp(0)
    faces = np.ascontiguousarray(inp["faces"], dtype=np.int32)
    mats = {k: np.asarray(inp["consts"][k], dtype=np.float32) for k in ("ambient", "mat_diffuse", "specular", "background")}
    G = Guards(device)
    _render_drain(lib, device)

    def _raw(lib_, name, *a):                                             # (the argument types include/hifihr.h declares: cast the pointers to them)
        fn = getattr(lib_.c, name)
        a = [ctypes.cast(x, t) if isinstance(x, vp) and t is not vp and hasattr(t, "contents") else x
             for x, t in zip(a, fn.argtypes)]
        lib_.check(fn(*a), name)

    def create(out="ok", faces_=faces, V_=V, F2=F_, H_=H, aa_=aa, null=None):
        hh = vp(0)
        m = {k: (None if k == null else v) for k, v in mats.items()}
        try:
            _raw(lib, "hifihr_renderer_create", ctypes.byref(hh) if out is not None else vp(0), np_p(faces_), c_int(V_), c_int(F2), c_int(H_), c_int(aa_),
                 np_p(m["ambient"]), np_p(m["mat_diffuse"]), np_p(m["specular"]), c_float(30.0), np_p(m["background"]))
        finally:
            assert hh.value is None or out == "made", "a refused hifihr_renderer_create left a handle"
        return hh

    if entry == "renderer_create":
        bad_lo, bad_hi = faces.copy(), faces.copy()
        bad_lo[3, 1], bad_hi[F_ - 1, 2] = -1, V
        calls = [("out NULL", lambda: create(out=None)), ("faces NULL", lambda: create(faces_=None)), ("V = 0", lambda: create(V_=0)),
                 ("V = -1", lambda: create(V_=-1)), ("F = 0", lambda: create(F2=0)), ("F = -1", lambda: create(F2=-1)),
                 ("image_size = 0", lambda: create(H_=0)), ("image_size = -1", lambda: create(H_=-1)),
                 (f"image_size = {RENDER_MAX_IMAGE + 1}", lambda: create(H_=RENDER_MAX_IMAGE + 1)), ("aa = 0", lambda: create(aa_=0)),
                 ("aa = 4", lambda: create(aa_=4)), ("a face index of -1", lambda: create(faces_=bad_lo)), ("a face index of V", lambda: create(faces_=bad_hi))]
        calls += [(f"{k} NULL", lambda k=k: create(null=k)) for k in mats]
        for name, call in calls:
            _render_refuses(entry, lib, device, call, G, name)
        hh = create(out="made", H_=RENDER_MAX_IMAGE)                      # the limit itself is accepted (no launch here)
        assert hh.value is not None and lib.render_workspace_bytes(hh, 1) > 0
        lib.renderer_destroy(hh)
        _layer_log(entry, True)
        return True
    h = lib.renderer_create(faces, V, image_size=H, aa=aa, **inp["consts"])
    try:
        if entry == "renderer_set_light_mode":
            for name, call in [("h NULL", lambda: _raw(lib, "hifihr_renderer_set_light_mode", vp(0), c_int(1))),
                               ("mode 2", lambda: _raw(lib, "hifihr_renderer_set_light_mode", h, c_int(2))),
                               ("mode -1", lambda: _raw(lib, "hifihr_renderer_set_light_mode", h, c_int(-1)))]:
                _render_refuses(entry, lib, device, call, G, name)
            return True
        if entry == "renderer_set_uv":
            lo, hi = fu.copy(), fu.copy()
            lo[0, 0], hi[F_ - 1, 2] = -1, len(vu)
            set_uv = lambda hh=h, f=fu, v=vu, n=len(vu): _raw(lib, "hifihr_renderer_set_uv", hh, np_p(f), np_p(v), c_int(n))
            for name, call in [("h NULL", lambda: set_uv(hh=vp(0))), ("faces_uvs NULL", lambda: set_uv(f=None)), ("verts_uvs NULL", lambda: set_uv(v=None)),
                               ("n_uv = 0", lambda: set_uv(n=0)), ("n_uv = -1", lambda: set_uv(n=-1)), ("an index of -1", lambda: set_uv(f=lo)),
                               ("an index of n_uv", lambda: set_uv(f=hi))]:
                _render_refuses(entry, lib, device, call, G, name)
            # a refused set_uv leaves the renderer without tables: the UV forward is still refused
            return True
        if entry in ("renderer_destroy", "render_workspace_bytes", "render_uv_scratch_bytes"):
            assert lib.c.hifihr_render_workspace_bytes(vp(0), c_int(2)) == 0 and lib.render_workspace_bytes(h, -1) == 0
            sizes = [lib.render_workspace_bytes(h, b) for b in range(6)]
            assert sizes == sorted(sizes) and sizes[1] > 0, sizes
            assert lib.render_uv_scratch_bytes(h, B) == 0 and lib.render_uv_scratch_bytes(h, 0) == 0
            assert lib.c.hifihr_renderer_destroy(vp(0)) == 0              # nothing to destroy: accepted
            assert not _render_drain(lib, device)
            _layer_log(entry, True)
            return False
        uvm = entry.endswith("_uv")
        bwd = "bwd" in entry
        ws = G.out(lib.render_workspace_bytes(h, B), dtype=torch.uint8)
        dv, dcam, dlc, dld, dw, dmaps = (G.inp(t) for t in (inp["verts"], inp["cam"], inp["lc"], inp["ld"], inp["w"], maps))
        dcol = G.inp(0.5 * torch.ones(B, V, 3))
        rgba, fid = G.out(B, 4, H, H), G.out(B, S, S, dtype=torch.int32)
        gv, gt, glc, gld = G.out(B, V, 3), G.out(*(maps.shape if uvm else (B, V, 3))), G.out(B, 3), G.out(B, 3)
        fid_in = G.inp(torch.from_numpy(inp["p2f"]))
        if entry == "render_fwd":
            names = ["h", "verts", "vcolors", "cam", "light_color", "light_dir", "rgba", "face_id", "workspace"]
            args = lambda B_=B: [h, _vp(dv), _vp(dcol), c_int(1), _vp(dcam), _vp(dlc), _vp(dld), c_int(B_), _vp(rgba), _vp(fid), _vp(ws), vp(0)]
            ptrs = [0, 1, 2, 4, 5, 6, 8, 9, 10]
        elif entry == "render_bwd":
            names = ["h", "verts", "cam", "light_color", "light_dir", "face_id", "grad_rgba", "gverts", "glight_color", "glight_dir", "workspace"]
            args = lambda B_=B: [h, _vp(dv), _vp(dcam), _vp(dlc), _vp(dld), _vp(fid_in), _vp(dw), c_int(B_), _vp(gv), _vp(gt), _vp(glc), _vp(gld), _vp(ws), vp(0)]
            ptrs = [0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12]
        elif entry == "render_fwd_uv":
            names = ["h", "verts", "maps", "cam", "light_color", "light_dir", "rgba", "face_id", "workspace"]
            args = lambda B_=B, th=TH, tw=TW: [h, _vp(dv), _vp(dmaps), c_int(th), c_int(tw), _vp(dcam), _vp(dlc), _vp(dld), c_int(B_), _vp(rgba), _vp(fid),
                                               vp(0), _vp(ws), vp(0)]
            ptrs = [0, 1, 2, 5, 6, 7, 9, 10, 12]
        else:
            names = ["h", "verts", "maps", "cam", "light_color", "light_dir", "face_id", "grad_rgba", "gverts", "glight_color", "glight_dir", "workspace"]
            args = lambda B_=B, th=TH, tw=TW: [h, _vp(dv), _vp(dmaps), c_int(th), c_int(tw), _vp(dcam), _vp(dlc), _vp(dld), _vp(fid_in), _vp(dw), c_int(B_),
                                               vp(0), vp(0), _vp(gv), _vp(gt), _vp(glc), _vp(gld), _vp(ws), vp(0)]
            ptrs = [0, 1, 2, 5, 6, 7, 8, 9, 13, 15, 16, 17]
        assert len(names) == len(ptrs)

        def call(null=None, **kw):
            a = args(**kw)
            if null is not None:
                a[null] = vp(0)
            _raw(lib, "hifihr_" + entry, *a)

        if uvm:                                                          # no UV tables yet: refused whatever else is right
            _render_refuses(entry, lib, device, call, G, "before hifihr_renderer_set_uv")
            lib.renderer_set_uv(h, fu, vu)
            _render_refuses(entry, lib, device, lambda: call(th=0), G, "TH = 0")
            _render_refuses(entry, lib, device, lambda: call(tw=0), G, "TW = 0")
            _render_refuses(entry, lib, device, lambda: call(th=-1), G, "TH = -1")
        for name, k in zip(names, ptrs):
            _render_refuses(entry, lib, device, lambda k=k: call(null=k), G, f"{name} NULL")
        _render_refuses(entry, lib, device, lambda: call(B_=-1), G, "B = -1")
        before = [t.clone() for t in G.wholes()]
        call(B_=0)                                                        # accepted: a no-op
        assert all(torch.equal(a, b2) for a, b2 in zip(G.wholes(), before)), f"{entry}: B = 0 wrote something"
        assert not _render_drain(lib, device), f"{entry}: B = 0 launched something"
        _layer_log(entry, True)
        return True
    finally:
        lib.renderer_destroy(h)
