"""Shared bodies of the tests of the self-supervised keypoint terms (hifihr_open2d_terms_fwd / _bwd, csrc/losses.hip) and of the launch
that feeds them (hifihr_freihand_keypoints, csrc/augment.hip): tests/test_hostsim_open2d.py runs them on the emulator (device='cpu'),
tests/test_gpu_open2d.py on the MI355X (device='cuda').  The reference is the float64 restatement of tests/open2d_ref.py, which
tests/test_open2d_host.py holds to the reference's own code (tests/golden/open2d.npz).

Sizes: B = 1, 13 (13 x 20 bones exceed the forward's 256 threads) and 65 (a second backward workgroup).
Bounds of the kernel pair: FACTOR = 8 times the worst error, over TERM_CASES, of the SAME restatement evaluated in float32 against float64
(tools/open2d_precision.py computes it on the CPU; profiles/open2d_precision.txt).  The 8 is the factor the `depth` term uses for a
summation order that differs from the yardstick's.  Errors are relative: an output against its own float64 value (every output is a sum of
non-negative addends), a gradient against the largest float64 gradient element of its case.  A float64 value of exactly 0 must come back as
exactly 0.  The yardstick is the float32 restatement, never the kernel."""
import numpy as np
import torch

import kernel_cases as kc
import open2d_ref as ref

EINVAL = -1
FACTOR = 8.0
# worst float32-restatement error over TERM_CASES, per output and for the gradient (tools/open2d_precision.py, CPU; profiles/open2d_precision.txt)
F32_WORST_OUT = (1.800e-07, 2.728e-07, 1.642e-07)
F32_WORST_GRAD = 1.581e-07

SPECIALS = ("random", "identical", "far", "straddle", "zero_con", "one_con", "zero_bones", "lam0", "lam1", "lam2")
# (B, special, confidences as [B,21,1] instead of [B,21])
TERM_CASES = [(1, "random", False), (13, "random", True), (65, "random", False), (13, "identical", False), (65, "identical", True),
              (1, "far", True), (13, "far", False), (1, "straddle", False), (13, "straddle", True), (65, "straddle", False),
              (13, "zero_con", True), (65, "zero_con", False), (13, "one_con", False), (65, "one_con", True), (13, "zero_bones", True),
              (65, "zero_bones", False), (13, "lam0", False), (13, "lam1", True), (13, "lam2", False)]
KERNELS = {"open2d_terms_fwd_kernel", "open2d_terms_bwd_kernel"}


def term_inputs(B, special, con3):
    """-> (j2d, det, con, lam, gout): float32 CPU tensors / tuples, seeded by the case."""
    g = torch.Generator().manual_seed(1000 * B + SPECIALS.index(special))
    det = 112.0 + 40.0 * torch.randn(B, 21, 2, generator=g)
    ang = 2 * np.pi * torch.rand(B, 21, generator=g)
    unit = torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    con = torch.rand(B, 21, generator=g)
    con[torch.rand(B, 21, generator=g) < 0.1] = 0.0                       # a missed joint
    lam, gout = (0.7, 0.2, 1.3), (1.25, -0.5, 0.75)
    if special == "identical":
        j2d = det.clone()
    elif special == "far":                                                # every d > 5
        j2d = det + unit * (6.0 + 20.0 * torch.rand(B, 21, 1, generator=g))
    elif special == "straddle":                                           # d on both sides of 5 within every sample
        mag = torch.stack([torch.linspace(3.0, 7.0, 21)[torch.randperm(21, generator=g)] for _ in range(B)])
        j2d = det + unit * mag.unsqueeze(-1)
    else:
        j2d = det + 3.0 * torch.randn(B, 21, 2, generator=g)
    if special == "zero_con":
        con = torch.zeros(B, 21)
        lam = (0.7, 0.2, 0.0)            # (open_2dj_de does not read the confidences)
    elif special == "one_con":
        con = torch.zeros(B, 21)
        con[B // 2, 7] = 0.6
    elif special == "zero_bones":                                         # coincident joints: predicted (a whole finger on the wrist) and detected
        j2d[:, 1:5] = j2d[:, 0:1]
        det[1::2, 6] = det[1::2, 5]
    elif special.startswith("lam"):
        lam = tuple(0.9 if k == int(special[3]) else 0.0 for k in range(3))
    return j2d.contiguous(), det.contiguous(), (con.unsqueeze(-1) if con3 else con).contiguous(), lam, gout


def f32_errors(B, special, con3):
    """The yardstick: the float32 restatement against the float64 one on this case -> (relative error per output [3], relative gradient
    error); an entry whose float64 value is 0 counts 0 when float32 gives 0 too, inf otherwise."""
    j2d, det, con, lam, gout = term_inputs(B, special, con3)
    o64, g64 = ref.terms_and_grad(j2d, det, con, lam, gout, torch.float64)
    o32, g32 = ref.terms_and_grad(j2d, det, con, lam, gout, torch.float32)
    rel = lambda err, scale: (err / scale) if scale > 0 else (0.0 if err == 0 else float("inf"))
    outs = [rel(abs(float(o32[k].double() - o64[k])), abs(float(o64[k]))) for k in range(3)]
    return outs, rel(float((g32.double() - g64).abs().max()), float(g64.abs().max()))


def run_pair(lib, device, j2d, det, con, lam, gout):
    """-> (out [3], g_j2d [B,21,2]) on the CPU; inputs and outputs sit in guard bands, both directions run twice: the same bits."""
    G = kc.Guards(device)
    j, d, c = G.inp(j2d), G.inp(det), G.inp(con)
    go = G.inp(torch.tensor(gout, dtype=torch.float32))
    outs, grads = [], []
    for _ in range(2):
        out, g = G.out(3, fill=float("nan")), G.out(*j2d.shape, fill=float("nan"))
        lib.open2d_terms_fwd(j, d, c, lam, out)
        lib.open2d_terms_bwd(j, d, c, lam, go, g)
        outs.append(out.cpu()); grads.append(g.cpu())
    G.intact("open2d_terms")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "out: two calls differ in their bits"
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)), "g_j2d: two calls differ in their bits"
    assert bool(torch.isfinite(outs[0]).all()) and bool(torch.isfinite(grads[0]).all()), "an element was not written, or is not finite"
    return outs[0], grads[0]


def terms_case(lib, device, B, special, con3):
    j2d, det, con, lam, gout = term_inputs(B, special, con3)
    out, grad = run_pair(lib, device, j2d, det, con, lam, gout)
    o64, g64 = ref.terms_and_grad(j2d, det, con, lam, gout, torch.float64)
    what = f"open2d_terms {(B, special, con3)}"
    for k in range(3):
        err, want = abs(float(out[k].double() - o64[k])), abs(float(o64[k]))
        print(f"{what}: out[{k}] = {float(out[k]):.9g}, float64 {float(o64[k]):.9g}, error {err:.3e}, bound {FACTOR * F32_WORST_OUT[k] * want:.3e}")
        if want == 0.0:
            assert float(out[k]) == 0.0, f"{what}: out[{k}] must be exactly 0"
        else:
            assert err <= FACTOR * F32_WORST_OUT[k] * want, f"{what}: out[{k}]"
    gerr, gmax = float((grad.double() - g64).abs().max()), float(g64.abs().max())
    print(f"{what}: gradient error {gerr:.3e}, largest element {gmax:.3e}, bound {FACTOR * F32_WORST_GRAD * gmax:.3e}")
    if gmax == 0.0:
        assert float(grad.abs().max()) == 0.0, f"{what}: the gradient must be exactly 0"
    else:
        assert gerr <= FACTOR * F32_WORST_GRAD * gmax, f"{what}: gradient"
    if special == "identical":
        assert float(grad.abs().max()) == 0.0 and float(out.abs().max()) == 0.0, f"{what}: prediction == detections"
    if special == "zero_con":
        assert float(out.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0, f"{what}: all confidences 0"
        # with the unweighted term switched on as well, the two weighted ones stay exactly 0
        out3, _ = run_pair(lib, device, j2d, det, con, (0.7, 0.2, 1.3), gout)
        assert float(out3[0]) == 0.0 and float(out3[1]) == 0.0 and float(out3[2]) > 0.0, f"{what}: with lambda_j2d_de"
    if special.startswith("lam"):
        k = int(special[3])
        assert all(float(out[i]) == 0.0 for i in range(3) if i != k) and float(out[k]) > 0.0, f"{what}: one term alone"


def refusal_case(lib, device):
    """J = 20 and 22, B = 0 and each NULL pointer: HIFIHR_EINVAL, nothing written."""
    from hifihr_amd._lib import _floats
    G = kc.Guards(device)
    B = 3
    j, d = G.inp(torch.randn(B, 22, 2)), G.inp(torch.randn(B, 22, 2))
    c, go = G.inp(torch.rand(B, 22)), G.inp(torch.ones(3))
    out, g = G.out(3), G.out(B, 22, 2)
    lam = _floats((1.0, 1.0, 1.0), 3)
    fwd = lambda j=j, d=d, c=c, B=B, J=21, lam=lam, out=out: lib._call("hifihr_open2d_terms_fwd", j, d, c, B, J, lam, out)
    bwd = lambda j=j, d=d, c=c, B=B, J=21, lam=lam, go=go, g=g: lib._call("hifihr_open2d_terms_bwd", j, d, c, B, J, lam, go, g)
    tries = [("J = 20", dict(J=20)), ("J = 22", dict(J=22)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("j2d NULL", dict(j=None)),
             ("open_2dj NULL", dict(d=None)), ("open_2dj_con NULL", dict(c=None)), ("lambda NULL", dict(lam=None))]
    if device == "cpu":
        kc.launch_log(lib)
    for what, kw in tries + [("out NULL", dict(out=None))]:
        assert fwd(**kw) == EINVAL, f"hifihr_open2d_terms_fwd accepted {what}"
    for what, kw in tries + [("gout NULL", dict(go=None)), ("g_j2d NULL", dict(g=None))]:
        assert bwd(**kw) == EINVAL, f"hifihr_open2d_terms_bwd accepted {what}"
    if device == "cuda":
        torch.cuda.synchronize()
    else:
        assert not [k for k in kc.launch_log(lib) if k.startswith("open2d")], "a refused call launched a kernel"
    G.intact("open2d_terms refusals")
    assert kc._is_canary(out) and kc._is_canary(g), "a refused call wrote an output"
    assert fwd() == 0 and bwd() == 0                         # the same arguments with J = 21 pass


# ---- the data path ---------------------------------------------------------------------------------------------------------------------
# (B, rotation, semi_ratio); the cache has CACHE_N rows so that indices on both sides of 32 560 exist; coordinates stay below 512 in magnitude
CACHE_N = ref.TRAIN_SIZE + 16300
KEYPOINT_CASES = [(B, rot, semi) for B in (1, 3, 65) for rot in ("zero", "quarter", "random") for semi in (None, 0.5)]
# indices around the thresholds: 32 560 (texture_con's factor; the wrap of idx % 32 560) and 16 280 = 32 560 x 0.5 (the semi mix)
EDGE_IDX = [0, 16279, 16280, 32559, 32560, 32561, 32560 + 16279, 32560 + 16280, 5, 40000]
TEX_ROUNDINGS = 21


def keypoint_cache():
    """-> (open_2dj [n,21,2] in 0 .. 224, open_2dj_con [n,21,1]): rows near EDGE_IDX carry every gate situation."""
    g = torch.Generator().manual_seed(7)
    det = 224.0 * torch.rand(CACHE_N, 21, 2, generator=g)
    con = 0.12 + 0.88 * torch.rand(CACHE_N, 21, 1, generator=g)
    low = torch.rand(CACHE_N, generator=g) < 0.4                          # 4 rows in 10: one joint at or below the gate's 0.1
    level = torch.tensor([0.0, 0.05, 0.1, float(np.float32(0.1))])[torch.randint(0, 4, (CACHE_N,), generator=g)]
    joint = torch.randint(0, 21, (CACHE_N,), generator=g)
    rows = torch.nonzero(low).view(-1)
    con[rows, joint[rows], 0] = level[rows]
    return det.contiguous(), con.contiguous()


def keypoint_inputs(B, rot, semi):
    from hifihr_amd.data import batch_affine_terms
    g = torch.Generator().manual_seed(100 * B + len(rot) + (1 if semi else 0))
    idx = torch.randint(0, CACHE_N, (B,), generator=g)
    idx[:min(B, len(EDGE_IDX))] = torch.tensor(EDGE_IDX[:B] if B < len(EDGE_IDX) else EDGE_IDX)
    if B == 3:
        idx = torch.tensor([16279, 16280, 32560])
    rots = {"zero": np.zeros(B), "quarter": np.full(B, np.pi / 2)}.get(rot)
    if rots is None:
        rots = ((2 * torch.rand(B, generator=g, dtype=torch.float64) - 1) * np.pi).numpy()
    total = batch_affine_terms(np.asarray([112, 112]), 224, [224, 224], rots, with_total=True)[3]
    j2d_gt = 224.0 * torch.rand(B, 21, 2, generator=g)
    return idx, torch.from_numpy(total).contiguous(), j2d_gt.contiguous()


def check_keypoints(what, got_det, got_con, got_tex, det, con, idx, total, j2d_gt, semi):
    """The three outputs (CPU tensors) against the restatement: the warp within 1e-4 px of a float64 evaluation of the same float32
    coefficients (three float32 roundings of values below 512: 3 x 2^-24 x 512 = 9.2e-5), confidences bit for bit, the gate and the mix
    exactly the restatement's choices, texture_con within TEX_ROUNDINGS float32 roundings."""
    B = idx.shape[0]
    pick = ref.semi_choice(idx, semi)
    warped = ref.warp(det[idx].double(), total.double())
    assert float(warped.abs().max()) < 512.0
    want_det, want_con = ref.semi_mix(warped, con[idx], j2d_gt.double(), idx, semi)
    for b in range(B):
        if bool(pick[b]):
            assert torch.equal(got_det[b], j2d_gt[b]) and bool((got_con[b] == 1.0).all()), f"{what}: sample {b} must take the ground truth"
        else:
            err = float((got_det[b].double() - want_det[b]).abs().max())
            assert err <= 1e-4, f"{what}: sample {b} warped {err:.3e} px off"
            assert torch.equal(got_con[b].view(torch.int32), want_con[b].view(torch.int32)), f"{what}: sample {b} confidences"
    tex = ref.texture_con(con[idx].double(), idx)
    c = con[idx].reshape(B, 21)
    open_gate = c.min(1)[0] > np.float32(0.1)
    assert torch.equal(got_tex > 0, open_gate), f"{what}: texture_con's gate"
    err = (got_tex.double() - tex).abs()
    assert bool((err <= TEX_ROUNDINGS * 2.0 ** -24 * tex.abs()).all()), f"{what}: texture_con {float(err.max()):.3e}"
    print(f"{what}: {int(pick.sum())} of {B} samples mixed, {int(open_gate.sum())} gates open, worst texture_con error "
          f"{float((err / tex.abs().clamp_min(1e-30)).max()) / 2.0 ** -24:.2f} roundings")


_CACHE = {}


def keypoints_case(lib, device, B, rot, semi, con3=True):
    from hifihr_amd.traineval import semi_below
    if "cache" not in _CACHE:
        _CACHE["cache"] = keypoint_cache()
    det, con = _CACHE["cache"]
    if (device, "det") not in _CACHE:
        _CACHE[device, "det"], _CACHE[device, "con"] = det.to(device), con.to(device)
    idx, total, j2d_gt = keypoint_inputs(B, rot, semi)
    G = kc.Guards(device)
    odet, ocon, otex = G.out(B, 21, 2, fill=float("nan")), G.out(B, 21, 1, fill=float("nan")), G.out(B, fill=float("nan"))
    below = semi_below(semi)
    cc = _CACHE[device, "con"] if con3 else _CACHE[device, "con"].view(CACHE_N, 21)
    lib.freihand_keypoints(_CACHE[device, "det"], cc, G.inp(idx.int()), G.inp(total), G.inp(j2d_gt) if below else None, below, odet, ocon, otex)
    G.intact("freihand_keypoints")
    check_keypoints(f"freihand_keypoints {(B, rot, semi)}", odet.cpu(), ocon.cpu(), otex.cpu(), det, con, idx, total, j2d_gt, semi)


def keypoints_refusal_case(lib, device):
    G = kc.Guards(device)
    B, n = 2, 4
    det, con = G.inp(torch.rand(n, 21, 2)), G.inp(torch.rand(n, 21))
    idx, total, gt = G.inp(torch.tensor([1, 3], dtype=torch.int32)), G.inp(torch.eye(3).repeat(B, 1, 1)), G.inp(torch.rand(B, 21, 2))
    odet, ocon, otex = G.out(B, 21, 2), G.out(B, 21), G.out(B)
    call = lambda det=det, con=con, n=n, idx=idx, total=total, gt=gt, below=0, B=B, odet=odet, ocon=ocon, otex=otex: lib._call(
        "hifihr_freihand_keypoints", det, con, n, idx, total, gt, below, B, odet, ocon, otex)
    for what, kw in [("n = 0", dict(n=0)), ("B = 0", dict(B=0)), ("semi_below < 0", dict(below=-1)), ("a mix without j2d_gt", dict(below=5, gt=None)),
                     ("open_2dj NULL", dict(det=None)), ("open_2dj_con NULL", dict(con=None)), ("idx NULL", dict(idx=None)),
                     ("total NULL", dict(total=None)), ("no output", dict(odet=None, ocon=None, otex=None))]:
        assert call(**kw) == EINVAL, f"hifihr_freihand_keypoints accepted {what}"
    if device == "cuda":
        torch.cuda.synchronize()
    G.intact("freihand_keypoints refusals")
    assert kc._is_canary(odet) and kc._is_canary(ocon) and kc._is_canary(otex), "a refused call wrote an output"
    assert call() == 0 and call(gt=None, otex=None) == 0
    # an index outside the cache cannot be refused (it lives in device memory): that sample is zeros, its neighbour is served
    bad = G.inp(torch.tensor([n, 2], dtype=torch.int32))
    o2, c2, t2 = G.out(B, 21, 2, fill=float("nan")), G.out(B, 21, fill=float("nan")), G.out(B, fill=float("nan"))
    assert call(idx=bad, odet=o2, ocon=c2, otex=t2) == 0
    assert float(o2[0].abs().max()) == 0.0 and float(c2[0].abs().max()) == 0.0 and float(t2[0]) == 0.0 and torch.equal(c2[1].cpu(), con[2].cpu())
    G.intact("freihand_keypoints, index outside the cache")
