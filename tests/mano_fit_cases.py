"""Shared bodies of the tests of the one-launch keypoint fit (hifihr_mano_fit, csrc/mano_fit.hip): tests/test_hostsim_mano_fit.py runs them
on the emulator (device='cpu'), tests/test_gpu_mano_fit.py on the MI355X (device='cuda').  The reference is the float64 restatement of
tests/mano_fit_ref.py.

Inputs: seeded hands on the given tables whose start is the truth perturbed by 0.15 rad (root rotation), 0.4 (PCA coefficients), shape 0 and
1 cm (root position); K = diag(480, 480) with principal point 112, z about 0.6; joint 7 missing (confidence 0, detection 0), joint 12 at
confidence 0.4.

Bounds: every compared quantity (a parameter group, a trace column, a gradient group) is held to FACTOR = 8 times the error of the SAME
restatement evaluated in float32 against float64 ON THAT CASE (largest absolute error over the quantity's elements), with a floor of
FLOOR_ROUNDINGS = 8 float32 roundings (2^-24 each) of the quantity's largest float64 magnitude: a quantity the float32 restatement happens
to hit almost exactly (eshape and epca are plain means) is still a few float32 operations away from its inputs.  The 8 is the factor the neighbouring kernels use for a
summation order that differs from the yardstick's.  A float64 value of exactly 0 (scale 0) must come back as exactly 0.  The yardstick is
the float32 restatement, never the kernel.  No element is excluded from a comparison.

The case builder ASSERTS that on every case the float32 restatement's parameters stay within CLOSE = 1e-4 of the float64 ones: two orders
above the float32 noise quoted for these inputs, two orders below one Adam step (lr >= 0.0025), so an ill-conditioned seed is rejected
loudly instead of widening the bounds."""
import numpy as np
import torch

import kernel_cases as kc
import mano_fit_ref as ref

EINVAL = -1
FACTOR = 8.0
FLOOR_ROUNDINGS = 8
ROUNDING = 2.0 ** -24
CLOSE = 1e-4
KERNEL = "mano_fit_kernel"
WEIGHTS = (1.0, 1.0, 0.0, 0.1, 0.1, 0.01)            # w2d, wbone, w3d, wprior, wshape, wpca
W3D = 1.0e4                                          # the 3-D term in the unit of the vertices (m^2): 1 cm^2 counts as 1 px of rho
LR_MULT = (1.0, 1.0, 1.0, 0.1)
TRACE_NAMES = ("E", "e2d", "ebone", "e3d", "eprior", "eshape", "epca", "pixel error")
GROUP_NAMES = ("root rotation", "pose coefficients", "shape", "root position")

_CASES = {}


def tsa_prior():
    from hifihr_amd import fit
    return tuple(torch.as_tensor(np.asarray(t, dtype=np.float32)).reshape(48) for t in (fit.TSA_LO, fit.TSA_HI, fit.TSA_W))


def build_case(tables, name, B, seed, with3d=False, with_prior=True, root_id=9):
    """-> dict of float32 CPU inputs (cached by name)."""
    if name in _CASES:
        return _CASES[name]
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pose_gt = torch.cat([0.5 * r(B, 3), 0.5 * r(B, 45)], 1)
    beta_gt = 0.5 * r(B, 10)
    root_gt = torch.cat([0.02 * r(B, 2), 0.6 + 0.03 * r(B, 1)], 1)
    K = torch.tensor([[480.0, 0.0, 112.0], [0.0, 480.0, 112.0], [0.0, 0.0, 1.0]], dtype=torch.float64).repeat(B, 1, 1)
    verts, _, _ = ref.mo.mano_forward(tables, pose_gt, beta_gt, dtype=torch.float64, center_idx=None)
    jrel, _, _ = ref.mo.root_relative(ref.mo.xyz_from_vertice(tables, verts, dtype=torch.float64), verts, root_id)
    X = jrel + root_gt.unsqueeze(1)
    p = (X.unsqueeze(2) * K.unsqueeze(1)).sum(3)
    kp2d = p[:, :, :2] / p[:, :, 2:3]
    conf = torch.ones(B, 21, dtype=torch.float64)
    conf[:, 7] = 0.0
    kp2d[:, 7] = 0.0                                                      # a missing joint: no detection at all
    conf[:, 12] = 0.4
    pose = pose_gt + torch.cat([0.15 * r(B, 3), 0.4 * r(B, 45)], 1)
    root = root_gt + 0.01 * r(B, 3)
    conf3 = torch.ones(B, 21, dtype=torch.float64)
    conf3[:, 3] = 0.0
    conf3[:, 15] = 0.5
    f = lambda t: t.float().contiguous()
    case = dict(name=name, tables=tables, B=B, root_id=root_id, pose=f(pose), beta=torch.zeros(B, 10), root=f(root), K=f(K), kp2d=f(kp2d),
                conf=f(conf), kp3d=f(jrel) if with3d else None, conf3=f(conf3) if with3d else None, prior=tsa_prior() if with_prior else None,
                weights=WEIGHTS[:2] + ((W3D,) if with3d else (0.0,)) + WEIGHTS[3:], refs={})
    _CASES[name] = case
    return case


def reference(case, iters, keep=(), lr=None):
    """The float64 and float32 restatements of `iters` iterations on this case (computed once, shared, never changed); asserts the two
    stay close."""
    key = (iters, tuple(keep))
    if key not in case["refs"]:
        lr = ref.DEFAULT_LR if lr is None else lr
        kw = dict(kp3d=case["kp3d"], conf3=case["conf3"], prior=case["prior"], weights=case["weights"], lr=lr, iters=iters, lr_mult=LR_MULT,
                  root_id=case["root_id"], keep=keep)
        args = (case["tables"], case["pose"], case["beta"], case["root"], case["K"], case["kp2d"], case["conf"])
        r64, r32 = ref.fit(*args, dtype=torch.float64, **kw), ref.fit(*args, dtype=torch.float32, **kw)
        for i, p64 in r64["params"].items():
            dev = float((r32["params"][i].double() - p64).abs().max())
            print(f"{case['name']}: after {i} iterations the float32 restatement is within {dev:.3e} of the float64 one")
            assert dev <= CLOSE, f"{case['name']}: ill-conditioned inputs, float32 and float64 restatements part by {dev:.3e} after {i} iterations"
        case["refs"][key] = (r64, r32)
    return case["refs"][key]


def held(what, got, want64, got32):
    """One quantity against its float64 value, bound from the float32 restatement's error on the same quantity."""
    got, want64, got32 = got.double(), want64.double(), got32.double()
    scale = float(want64.abs().max())
    err, err32 = float((got - want64).abs().max()), float((got32 - want64).abs().max())
    bound = max(FACTOR * err32, FLOOR_ROUNDINGS * ROUNDING * scale)
    print(f"{what}: error {err:.3e}, float32 restatement {err32:.3e}, bound {bound:.3e}, scale {scale:.3e}, ratio to the restatement "
          f"{err / err32 if err32 > 0 else float('inf') if err > 0 else 0.0:.2f}")
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, f"{what}: must be exactly 0"
    else:
        assert err <= bound, f"{what}: {err:.3e} above {bound:.3e}"


def held_params(what, got61, want64, got32):
    for (a, b), n in zip(ref.GROUPS, GROUP_NAMES):
        held(f"{what}, {n}", got61[:, a:b], want64[:, a:b], got32[:, a:b])


def held_trace(what, got, want64, got32):
    """One bound per trace column over all its rows: the scale and the float32 error are those of the largest row (the start), so the rows at
    the end of a long trajectory are held more loosely than the parameters, which held_params compares at the result itself."""
    for k, n in enumerate(TRACE_NAMES):
        held(f"{what}, trace column {n}", got[..., k], want64[..., k], got32[..., k])


def bits(t):
    return t.contiguous().view(torch.int32)


def run_fit(lib, device, handle, case, iters, lr=None, lr_mult=LR_MULT, weights=None, want_grad0=False, over=None, sel=None):
    """One call of the entry -> dict(par [B,61], trace, grad0, done) on the CPU.  The outputs sit in guard bands.  `over` replaces inputs by
    name, `sel` picks hands."""
    inp = {k: case[k] for k in ("pose", "beta", "root", "K", "kp2d", "conf", "kp3d", "conf3")}
    inp.update(over or {})
    if sel is not None:
        inp = {k: (None if v is None else v[sel].contiguous()) for k, v in inp.items()}
    B = inp["pose"].shape[0]
    G = kc.Guards(device)
    pose, beta, root = G.out(B, 48, fill=0.0), G.out(B, 10, fill=0.0), G.out(B, 3, fill=0.0)
    pose.copy_(inp["pose"]); beta.copy_(inp["beta"]); root.copy_(inp["root"])
    trace, done = G.out(B, iters + 1, 8, fill=float("nan")), G.out(B, fill=-7, dtype=torch.int32)
    grad0 = G.out(B, 61, fill=float("nan")) if want_grad0 else None
    lr = (ref.DEFAULT_LR if lr is None else lr)[:iters]
    lr_d = G.inp(torch.tensor(lr, dtype=torch.float32)) if iters > 0 else None
    prior = None if case["prior"] is None else tuple(G.inp(t) for t in case["prior"])
    lib.mano_fit(handle, pose, beta, root, G.inp(inp["K"]), G.inp(inp["kp2d"]), G.inp(inp["conf"]), G.inp(inp["kp3d"]), G.inp(inp["conf3"]), prior,
                 lr_d, iters, case["weights"] if weights is None else weights, lr_mult, case["root_id"], trace, grad0, done)
    if device == "cuda":
        torch.cuda.synchronize()
    G.intact(f"mano_fit {case['name']}")
    return dict(par=torch.cat([pose, beta, root], 1).cpu(), trace=trace.cpu(), grad0=None if grad0 is None else grad0.cpu(), done=done.cpu(),
                par_in=torch.cat([inp["pose"], inp["beta"], inp["root"]], 1))


# ---- 1. iters = 0 -----------------------------------------------------------------------------------------------------------------------
# (name, B, seed, 3-D term, prior, root_id, tables)
EVAL_CASES = [("plain-b1", 1, 11, False, False, 9, "synth"), ("plain-b3", 3, 12, False, False, 9, "synth"),
              ("prior-b3", 3, 13, False, True, 9, "synth"), ("kp3d-b3", 3, 14, True, False, 9, "synth"),
              ("all-root0-b3", 3, 15, True, True, 0, "synth"), ("all-dense-b3", 3, 16, True, True, 9, "dense"),
              ("plain-dense-root0-b1", 1, 17, False, False, 0, "dense")]


def eval_case(lib, device, tables, name, B, seed, with3d, with_prior, root_id):
    case = build_case(tables, "eval-" + name, B, seed, with3d, with_prior, root_id)
    r64, r32 = reference(case, 0)
    h = lib.mano_create(tables)
    try:
        out = run_fit(lib, device, h, case, 0, want_grad0=True)
    finally:
        lib.mano_destroy(h)
    assert torch.equal(bits(out["par"]), bits(out["par_in"])), f"{name}: iters = 0 changed a parameter's bits"
    assert out["done"].tolist() == [0] * B, out["done"]
    held_trace(f"{name} iters = 0", out["trace"][:, 0], r64["trace"][:, 0], r32["trace"][:, 0])
    held_params(f"{name} grad0", out["grad0"], r64["grad0"], r32["grad0"])
    assert float(r64["trace"][:, 0, 4].min()) > 0.0 or not with_prior, "the prior is not active on this case"
    assert float(r64["trace"][:, 0, 3].min()) > 0.0 or not with3d, "the 3-D term is not active on this case"


# ---- 2. / 3. trajectory and recovery ----------------------------------------------------------------------------------------------------
def trajectory_case(lib, device, tables, iters, with3d=False, B=3):
    """Parameters and trace after `iters` iterations -> the kernel's outputs and the float64 reference (for the recovery check)."""
    case = build_case(tables, f"traj-{'3d' if with3d else '2d'}-b{B}", B, 21 + with3d, with3d, True, 9)
    r64, r32 = reference(case, iters)
    h = lib.mano_create(tables)
    try:
        out = run_fit(lib, device, h, case, iters)
    finally:
        lib.mano_destroy(h)
    assert out["done"].tolist() == [iters] * B, out["done"]
    held_params(f"{case['name']} after {iters} iterations", out["par"], r64["params"][iters], r32["params"][iters])
    held_trace(f"{case['name']} over {iters} iterations", out["trace"], r64["trace"], r32["trace"])
    return out, r64, case


def recovery_check(out, r64, case):
    """Final E below a tenth of the starting E for every hand; with the 3-D term on, the root-relative joint error falls.  The error used
    is the trace's e3d, the confidence-weighted mean SQUARED distance of the root-relative joints to kp3d (the quantity the kernel reports),
    not a plain mean distance: it falls when the joints approach their targets."""
    E0, E1 = out["trace"][:, 0, 0], out["trace"][:, -1, 0]
    print(f"{case['name']}: E {E0.tolist()} -> {E1.tolist()} (float64: {r64['trace'][:, -1, 0].tolist()}), pixel error "
          f"{out['trace'][:, 0, 7].tolist()} -> {out['trace'][:, -1, 7].tolist()}")
    assert bool((E1 < E0 / 10.0).all()), f"{case['name']}: the fit did not reach a tenth of its starting objective"
    if case["kp3d"] is not None:
        e3 = out["trace"][:, :, 3]
        assert bool((e3[:, -1] < e3[:, 0]).all()), f"{case['name']}: the root-relative joint error did not fall"


# ---- 4. invariances ---------------------------------------------------------------------------------------------------------------------
def _invariance_ab(lib, device, h, case, iters):
    a = run_fit(lib, device, h, case, iters, want_grad0=True)
    b = run_fit(lib, device, h, case, iters, want_grad0=True)
    for k in ("par", "trace", "grad0", "done"):
        assert torch.equal(bits(a[k]), bits(b[k])), f"(a) two calls differ in the bits of {k}"
    assert not torch.equal(a["par"], a["par_in"])
    alone = run_fit(lib, device, h, case, iters, want_grad0=True, sel=[1])
    for k in ("par", "trace", "grad0", "done"):
        assert torch.equal(bits(a[k][1:2]), bits(alone[k])), f"(b) hand 1 of 3 differs from the same hand alone in {k}"


def invariance_case(lib, device, tables, iters=5, parts="abcde"):
    """(a) .. (e) of the invariances; `parts` picks some of them (the emulator runs them in three tests)."""
    case = build_case(tables, "inv-b3", 3, 31, True, True, 9)
    h = lib.mano_create(tables)
    try:
        if "a" in parts or "b" in parts:
            _invariance_ab(lib, device, h, case, iters)
        for grp, (lo, hi) in enumerate(ref.GROUPS if "c" in parts else ()):
            mult = tuple(0.0 if k == grp else m for k, m in enumerate(LR_MULT))
            o = run_fit(lib, device, h, case, iters, lr_mult=mult)
            assert torch.equal(bits(o["par"][:, lo:hi]), bits(o["par_in"][:, lo:hi])), f"(c) frozen group {GROUP_NAMES[grp]} moved"
            for g2, (l2, h2) in enumerate(ref.GROUPS):
                if g2 != grp:
                    assert bool((o["par"][:, l2:h2] != o["par_in"][:, l2:h2]).any(1).all()), f"(c) {GROUP_NAMES[g2]} did not move with {GROUP_NAMES[grp]} frozen"
        if "d" in parts or "e" in parts:
            o = run_fit(lib, device, h, case, iters, weights=(0.0,) * 6)
            assert torch.equal(bits(o["par"]), bits(o["par_in"])) and o["done"].tolist() == [iters] * 3, "(d) all weights 0 moved a parameter"
            assert float(o["trace"][:, :, 0].abs().max()) == 0.0
            off = build_case(tables, "inv-nopriors-b3", 3, 32, False, False, 9)
            o = run_fit(lib, device, h, off, iters, weights=(1.0, 1.0, 0.0, 0.0, 0.0, 0.0), over=dict(conf=torch.zeros(3, 21)))
            assert torch.equal(bits(o["par"]), bits(o["par_in"])) and o["done"].tolist() == [iters] * 3, "(e) sum c^2 = 0 moved a parameter"
            assert float(o["trace"][:, :, :3].abs().max()) == 0.0 and float(o["trace"][:, :, 7].abs().max()) == 0.0
    finally:
        lib.mano_destroy(h)


# ---- 5. non-finite inputs ---------------------------------------------------------------------------------------------------------------
def nonfinite_case(lib, device, tables, iters=3):
    case = build_case(tables, "inv-b3", 3, 31, True, True, 9)
    kp = case["kp2d"].clone()
    kp[1, 5, 0] = float("inf")
    h = lib.mano_create(tables)
    try:
        clean = run_fit(lib, device, h, case, iters)
        o = run_fit(lib, device, h, case, iters, over=dict(kp2d=kp))
    finally:
        lib.mano_destroy(h)
    assert o["done"].tolist() == [iters, 0, iters], o["done"]
    assert torch.equal(bits(o["par"][1]), bits(o["par_in"][1])), "the hand with an inf moved"
    assert not bool(torch.isfinite(o["trace"][1, 0, 0])) and float(o["trace"][1, 1:].abs().max()) == 0.0
    for b in (0, 2):
        assert torch.equal(bits(o["par"][b]), bits(clean["par"][b])) and torch.equal(bits(o["trace"][b]), bits(clean["trace"][b])), f"hand {b} was affected"
    # a non-finite keypoint counts even at confidence 0 (include/hifihr.h): joint 7 is the missing joint of every case
    assert float(case["conf"][2, 7]) == 0.0
    kp0 = case["kp2d"].clone()
    kp0[2, 7, 1] = float("inf")
    h = lib.mano_create(tables)
    try:
        o = run_fit(lib, device, h, case, iters, over=dict(kp2d=kp0))
    finally:
        lib.mano_destroy(h)
    assert o["done"].tolist() == [iters, iters, 0], o["done"]
    assert torch.equal(bits(o["par"][2]), bits(o["par_in"][2])) and not bool(torch.isfinite(o["trace"][2, 0, 0]))
    for b in (0, 1):
        assert torch.equal(bits(o["par"][b]), bits(clean["par"][b])), f"hand {b} was affected"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def refusal_case(lib, device, tables):
    from hifihr_amd._lib import _floats
    case = build_case(tables, "inv-b3", 3, 31, True, True, 9)
    B, iters = 3, 2
    G = kc.Guards(device)
    pose, beta, root = G.out(B, 48), G.out(B, 10), G.out(B, 3)
    trace, grad0, done = G.out(B, iters + 1, 8), G.out(B, 61), G.out(B, dtype=torch.int32)
    K, kp, c, kp3, c3 = (G.inp(case[k]) for k in ("K", "kp2d", "conf", "kp3d", "conf3"))
    lo, hi, w = (G.inp(t) for t in case["prior"])
    lr = G.inp(torch.tensor([0.01, 0.01]))
    wt, mu = _floats(case["weights"], 6), _floats(LR_MULT, 4)
    h = lib.mano_create(tables)
    call = lambda h=h, pose=pose, beta=beta, root=root, K=K, kp=kp, c=c, kp3=kp3, c3=c3, lo=lo, hi=hi, w=w, lr=lr, iters=iters, wt=wt, mu=mu, \
        root_id=9, B=B, trace=trace, grad0=grad0, done=done: lib._call("hifihr_mano_fit", h, pose, beta, root, K, kp, c, kp3, c3, lo, hi, w, lr,
                                                                      iters, wt, mu, root_id, B, trace, grad0, done)
    bad6 = lambda v: _floats(tuple(v if k == 2 else 1.0 for k in range(6)), 6)
    bad4 = lambda v: _floats(tuple(v if k == 3 else 1.0 for k in range(4)), 4)
    tries = [("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("iters < 0", dict(iters=-1)), ("root_id = 21", dict(root_id=21)), ("root_id = -1", dict(root_id=-1)),
             ("handle NULL", dict(h=None)), ("pose NULL", dict(pose=None)), ("beta NULL", dict(beta=None)), ("root NULL", dict(root=None)),
             ("K NULL", dict(K=None)), ("kp2d NULL", dict(kp=None)), ("conf2d NULL", dict(c=None)), ("weights NULL", dict(wt=None)),
             ("lr_mult NULL", dict(mu=None)), ("trace NULL", dict(trace=None)), ("done NULL", dict(done=None)), ("lr NULL with iters > 0", dict(lr=None)),
             ("kp3d without conf3d", dict(c3=None)), ("conf3d without kp3d", dict(kp3=None)), ("prior without lo", dict(lo=None)),
             ("prior without hi", dict(hi=None)), ("prior without w", dict(w=None)), ("a negative weight", dict(wt=bad6(-1.0))),
             ("a NaN weight", dict(wt=bad6(float("nan")))), ("an infinite weight", dict(wt=bad6(float("inf")))),
             ("a negative multiplier", dict(mu=bad4(-0.1))), ("a NaN multiplier", dict(mu=bad4(float("nan"))))]
    try:
        if device == "cpu":
            kc.launch_log(lib)
        for what, kw in tries:
            assert call(**kw) == EINVAL, f"hifihr_mano_fit accepted {what}"
        if device == "cuda":
            torch.cuda.synchronize()
        else:
            assert KERNEL not in kc.launch_log(lib), "a refused call launched the kernel"
        G.intact("mano_fit refusals")
        for t in (pose, beta, root, trace, grad0, done):
            assert kc._is_canary(t), "a refused call wrote an output"
        pose.copy_(case["pose"]); beta.copy_(case["beta"]); root.copy_(case["root"])
        assert call() == 0 and call(kp3=None, c3=None, lo=None, hi=None, w=None, grad0=None) == 0 and call(iters=0, lr=None) == 0
        if device == "cuda":
            torch.cuda.synchronize()
        G.intact("mano_fit after the accepted calls")
    finally:
        lib.mano_destroy(h)
