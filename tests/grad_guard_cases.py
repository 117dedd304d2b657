"""Shared bodies of the gradient-guard tests (hifihr_grad_norm / hifihr_adam_step_guarded, csrc/adam.hip): tests/test_hostsim_grad_guard.py
runs them on the emulator (device='cpu'), tests/test_gpu_grad_guard.py on the MI355X (device='cuda').

References: torch on the CPU (torch.nn.utils.clip_grad_norm_ + torch.optim.Adam) for the clipped trajectory, a float64 restatement of the
Adam update with an explicit step number for the skip cases, the unguarded entries themselves for max_norm = inf (bit identity).
Bounds:
  norm    1e-6 relative to the float64 norm: the squares and every sum are formed in double, what is left is the rounding of the double
          sum itself (n 2^-53 at the very worst) -- the bound is the one the contract states, with room to spare.
  coef    2^-23 relative to min(1, max_norm / (norm_f64 + 1e-6)): one rounding to fp32 on top of the norm's error.
  Adam    2e-6 + 1e-5 |p| per element, the comparator of kernel_cases.adam_case."""
import ctypes
import math
import struct

import numpy as np
import torch

import kernel_cases as kc

NORM_RTOL = 1e-6
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
NORM_SIZES = [1, 3, 1003, 4096, 70001]
# several grid-stride sweeps plus a tail for the launcher's cap of 2048 workgroups x 256 threads x 4 floats = 2 097 152 floats per sweep
NORM_SIZE_LARGE = 12_000_005
ADAM_SIZES = [1003, 4096]
TRAJECTORY_SCALES = (1.0, 100.0, 0.01)
TRAJECTORY_GRAD_SCALE, TRAJECTORY_MAX_NORM = 0.5, 10.0


def read_guard(lib, guard):
    return lib.grad_guard_unpack(guard.cpu().numpy().tobytes())


def _raw_bytes(guard):
    return bytes(guard.cpu().numpy().tobytes())


def expected_coef(norm64, max_norm):
    return min(1.0, max_norm / (norm64 + 1e-6))


# ------------------------------------------------------------------------------------------------
# norm pass
# ------------------------------------------------------------------------------------------------
def norm_case(lib, device, n, grad_scale=0.5, seed=None):
    """A random gradient: the norm against float64, the coefficient on both sides of 1, the same bits from the same call, the counters."""
    gen = torch.Generator().manual_seed(n if seed is None else seed)
    g = torch.randn(n, generator=gen)
    ref = abs(grad_scale) * float(g.double().norm())
    gd = g.to(device)
    guard, ws = lib.grad_guard_alloc(n, device)
    lo, hi = 0.5 * ref, 2.0 * ref                                  # one max_norm that clips, one that does not
    lib.grad_norm(gd, grad_scale, lo, guard, ws)
    first = read_guard(lib, guard)
    first_raw = _raw_bytes(guard)
    print(f"grad_norm n={n}: norm {first['norm']!r} ref {ref!r} rel {abs(first['norm'] - ref) / ref:.3e} coef {first['clip_coef']!r}")
    assert abs(first["norm"] - ref) <= NORM_RTOL * ref, (n, first["norm"], ref)
    assert first["finite"] and (first["steps"], first["clipped"], first["skipped"]) == (1, 1, 0), first
    want = expected_coef(ref, lo)
    assert first["clip_coef"] < 1.0 and abs(first["clip_coef"] - want) <= 2.0 ** -23 * want + NORM_RTOL * want, (first, want)
    lib.grad_norm(gd, grad_scale, lo, guard, ws)                   # the same call: the same bits (counters apart)
    again_raw = _raw_bytes(guard)
    assert again_raw[:16] == first_raw[:16], "the same input gave other bits"
    assert read_guard(lib, guard)["steps"] == 2 and read_guard(lib, guard)["clipped"] == 2
    lib.grad_norm(gd, grad_scale, hi, guard, ws)
    third = read_guard(lib, guard)
    assert third["clip_coef"] == 1.0 and third["finite"] and (third["steps"], third["clipped"], third["skipped"]) == (3, 2, 0), third
    assert _raw_bytes(guard)[:8] == first_raw[:8]                  # (the norm does not depend on max_norm)
    lib.grad_norm(gd, grad_scale, float("inf"), guard, ws)         # guard only
    fourth = read_guard(lib, guard)
    assert fourth["clip_coef"] == 1.0 and fourth["finite"] and (fourth["steps"], fourth["clipped"]) == (4, 2), fourth


def zero_case(lib, device, n):
    guard, ws = lib.grad_guard_alloc(n, device)
    lib.grad_norm(torch.zeros(n, device=device), 0.5, 1.0, guard, ws)
    s = read_guard(lib, guard)
    assert s["norm"] == 0.0 and s["clip_coef"] == 1.0 and s["finite"] and (s["steps"], s["clipped"], s["skipped"]) == (1, 0, 0), s


def huge_case(lib, device, n=1003):
    """Every element 1e30: the fp32 squares would overflow, the double ones do not -- finite, clipped, NOT skipped."""
    g = torch.full((n,), 1e30)
    ref = float(g.double().norm())                                 # 3.167e31 at n = 1003
    assert math.isfinite(ref) and not math.isfinite(float((g * g).sum()))       # (the fp32 sum of squares is inf)
    guard, ws = lib.grad_guard_alloc(n, device)
    lib.grad_norm(g.to(device), 1.0, 1.0, guard, ws)
    s = read_guard(lib, guard)
    assert s["finite"] and abs(s["norm"] - ref) <= NORM_RTOL * ref, (s, ref)
    assert 0.0 < s["clip_coef"] < 1.0 and (s["steps"], s["clipped"], s["skipped"]) == (1, 1, 0), s
    assert abs(s["clip_coef"] - 1.0 / ref) <= 2.0 ** -22 * (1.0 / ref), (s, 1.0 / ref)


def nonfinite_positions(n):
    """index 0, the last element of the last float4, the last element of the scalar tail"""
    assert n % 4 != 0 and n > 8
    return {"first": 0, "last_float4": n // 4 * 4 - 1, "tail": n - 1}


def nonfinite_case(lib, device, value, where, n=1003):
    g = torch.randn(n, generator=torch.Generator().manual_seed(7))
    g[nonfinite_positions(n)[where]] = value
    guard, ws = lib.grad_guard_alloc(n, device)
    lib.grad_norm(g.to(device), 0.5, 10.0, guard, ws)
    s = read_guard(lib, guard)
    assert not s["finite"] and s["clip_coef"] == 0.0 and not math.isfinite(s["norm"]), s
    assert (s["steps"], s["clipped"], s["skipped"]) == (1, 0, 1), s


# ------------------------------------------------------------------------------------------------
# guarded Adam
# ------------------------------------------------------------------------------------------------
class _Run:
    """One trajectory through the guarded entry: host-scalar form (counted=False) or counted form (state in device memory)."""

    def __init__(self, lib, device, p0, counted, wd, grad_scale, max_norm, guarded=True):
        n = p0.numel()
        self.lib, self.device, self.counted, self.wd, self.gs, self.max_norm, self.guarded = lib, device, counted, wd, grad_scale, max_norm, guarded
        self.p = p0.clone().to(device)
        self.m = torch.zeros(n, device=device)
        self.v = torch.zeros(n, device=device)
        self.state = lib.adam_state_image(LR, B1, B2, 0).to(device) if counted else None
        self.guard, self.ws = lib.grad_guard_alloc(n, device)
        self.t = 0

    def step(self, g):
        self.t += 1
        gd = g.to(self.device)
        lib = self.lib
        if self.guarded:
            lib.grad_norm(gd, self.gs, self.max_norm, self.guard, self.ws)
            lib.adam_step_guarded(self.p, gd, self.m, self.v, self.gs, LR, B1, B2, EPS, self.wd, self.t, self.state, self.guard)
        elif self.counted:
            lib.adam_step_counted(self.p, gd, self.m, self.v, self.gs, EPS, self.wd, self.state)
        else:
            lib.adam_step(self.p, gd, self.m, self.v, self.gs, LR, B1, B2, EPS, self.wd, self.t)

    def buffers(self):
        return [t.cpu().clone() for t in (self.p, self.m, self.v)]

    def read_state(self):
        return struct.unpack("<dddddii", bytes(self.state.cpu().numpy().tobytes()))


def trajectory_grads(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    return p0, [torch.randn(n, generator=gen) * s for s in TRAJECTORY_SCALES]


_TORCH_REF = {}


def torch_clipped_reference(n, wd, clip=True):
    """clip_grad_norm_ + torch.optim.Adam on the CPU: (parameters after three steps, the norms clip_grad_norm_ saw).  Computed once per case."""
    key = (n, wd, clip)
    if key not in _TORCH_REF:
        p0, grads = trajectory_grads(n)
        ref = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
        norms = []
        for g in grads:
            ref.grad = (g * TRAJECTORY_GRAD_SCALE).clone()
            if clip:
                norms.append(float(torch.nn.utils.clip_grad_norm_([ref], TRAJECTORY_MAX_NORM, norm_type=2)))
            opt.step()
        _TORCH_REF[key] = (ref.detach().clone(), norms)
    return _TORCH_REF[key]


def adam_close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    err = (got - ref).abs()
    bound = 2e-6 + 1e-5 * ref.abs()
    worst = float((err / bound).max())
    print(f"{what}: worst err / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: err / (2e-6 + 1e-5 |p|) = {worst:.3f}"


def clipped_trajectory_case(lib, device, n, counted, wd=0.0):
    p0, grads = trajectory_grads(n)
    ref, norms = torch_clipped_reference(n, wd)
    clips = sum(1 for x in norms if TRAJECTORY_MAX_NORM / (x + 1e-6) < 1.0)
    assert clips == 2, norms                                        # two steps clip and one does not
    unclipped, _ = torch_clipped_reference(n, wd, clip=False)       # a guard that does nothing cannot pass
    assert float((unclipped - ref).abs().max()) > 1e-3
    run = _Run(lib, device, p0, counted, wd, TRAJECTORY_GRAD_SCALE, TRAJECTORY_MAX_NORM)
    for g in grads:
        run.step(g)
    adam_close(run.p, ref, f"clipped trajectory n={n} counted={counted} wd={wd}")
    s = read_guard(lib, run.guard)
    assert (s["steps"], s["clipped"], s["skipped"]) == (3, 2, 0), s
    assert abs(s["norm"] - norms[-1]) <= 1e-5 * norms[-1], (s, norms)      # (torch's norm is an fp32 one)
    if counted:
        st = run.read_state()
        assert (st[5], st[6]) == (3, 0), st


def inf_is_bit_identical_case(lib, device, n, counted, wd=0.01):
    """max_norm = inf: coef is exactly 1.0f and parameters and both moments carry the bits of the unguarded entry."""
    p0, grads = trajectory_grads(n, seed=1)
    a = _Run(lib, device, p0, counted, wd, 0.5, float("inf"))
    b = _Run(lib, device, p0, counted, wd, 0.5, None, guarded=False)
    for g in grads:
        a.step(g); b.step(g)
        for x, y, name in zip(a.buffers(), b.buffers(), ("params", "exp_avg", "exp_avg_sq")):
            assert torch.equal(x, y), f"n={n} counted={counted}: {name} differ from the unguarded entry at step {a.t}"
    assert read_guard(lib, a.guard)["clip_coef"] == 1.0
    if counted:
        assert a.read_state() == b.read_state()


def adam_f64(p, g, m, v, t, wd, grad_scale):
    """The update in float64 from fp32 inputs, with an explicit step number."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gr = g * float(np.float32(grad_scale)) + float(np.float32(wd)) * p
    b1, b2 = float(np.float32(B1)), float(np.float32(B2))
    m = b1 * m + (1 - b1) * gr
    v = b2 * v + (1 - b2) * gr * gr
    denom = v.sqrt() / math.sqrt(1 - B2 ** t) + float(np.float32(EPS))
    return p - (LR / (1 - B1 ** t)) * (m / denom), m, v


def skip_case(lib, device, n, counted, value, wd=0.01):
    """A non-finite gradient at step 2 of 3: the three buffers keep their bits across it, the step still counts, step 3 is the t = 3 update."""
    p0, grads = trajectory_grads(n, seed=2)
    grads[1] = grads[1].clone()
    grads[1][n // 2] = value
    run = _Run(lib, device, p0, counted, wd, 0.5, float("inf"))
    run.step(grads[0])
    before = run.buffers()
    ref1 = adam_f64(p0, grads[0], torch.zeros(n), torch.zeros(n), 1, wd, 0.5)
    adam_close(before[0], ref1[0], f"skip n={n} counted={counted}: step 1")
    run.step(grads[1])
    after = run.buffers()
    for x, y, name in zip(before, after, ("params", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), f"n={n} counted={counted}: the skipped step changed {name}"
    s = read_guard(lib, run.guard)
    assert not s["finite"] and (s["steps"], s["clipped"], s["skipped"]) == (2, 0, 1), s
    if counted:                                                     # the skipped step counts: counter and running products advance
        st = run.read_state()
        assert (st[5], st[6]) == (2, 0) and abs(st[3] - B1 ** 2) <= 1e-14 and abs(st[4] - B2 ** 2) <= 1e-14, st
    run.step(grads[2])
    ref3 = adam_f64(after[0], grads[2], after[1], after[2], 3, wd, 0.5)
    ref_t2 = adam_f64(after[0], grads[2], after[1], after[2], 2, wd, 0.5)
    assert float((ref3[0] - ref_t2[0]).abs().max()) > 1e-4          # (t = 2 and t = 3 are told apart at this tolerance)
    adam_close(run.p, ref3[0], f"skip n={n} counted={counted}: step 3 with t = 3")
    s = read_guard(lib, run.guard)
    assert s["finite"] and (s["steps"], s["clipped"], s["skipped"]) == (3, 0, 1), s
    if counted:
        assert run.read_state()[5] == 3


# ------------------------------------------------------------------------------------------------
# refusals: HIFIHR_EINVAL, nothing launched or written (guard bands around every buffer the entries could write)
# ------------------------------------------------------------------------------------------------
def refusal_case(lib, device, n=1003):
    from hifihr_amd._lib import _fp
    G = kc.Guards(device)
    gen = torch.Generator().manual_seed(3)
    g = G.inp(torch.randn(n, generator=gen))
    g_off = G.inp(torch.randn(n, generator=gen), offset_floats=1)          # 4 bytes past a 16-byte boundary
    p, m, v = (G.out(n, fill=0.25) for _ in range(3))
    p_off = G.out(n, fill=0.25, offset_floats=1)
    guard_b, ws_b = (int(lib.c.hifihr_grad_guard_bytes()), int(lib.c.hifihr_grad_norm_workspace_bytes(ctypes.c_size_t(n))))
    assert guard_b == 32 and guard_b % 8 == 0 and ws_b >= 8 and ws_b % 8 == 0
    guard = G.out(guard_b, dtype=torch.uint8, fill=0)
    guard_off = G.out(guard_b, dtype=torch.uint8, fill=0, offset_floats=4)     # (bytes: 4 past an 8-byte boundary)
    ws = G.out(ws_b, dtype=torch.uint8, fill=0)
    ws_off = G.out(ws_b, dtype=torch.uint8, fill=0, offset_floats=4)
    state = G.out(48, dtype=torch.uint8)
    state.copy_(lib.adam_state_image(LR, B1, B2, 0))
    state_off = G.out(48, dtype=torch.uint8, offset_floats=4)
    state_off.copy_(lib.adam_state_image(LR, B1, B2, 0))
    for t in (guard, ws, state):
        assert t.data_ptr() % 8 == 0
    for t in (guard_off, ws_off, state_off):
        assert t.data_ptr() % 8 == 4
    assert g.data_ptr() % 16 == 0 and g_off.data_ptr() % 16 == 4 and p_off.data_ptr() % 16 == 4
    vp, nz = kc._vp, ctypes.c_size_t(n)
    nan, inf = float("nan"), float("inf")

    def norm(gp=None, count=nz, gs=0.5, mx=1.0, gd=guard, w=ws):
        return lambda: kc._raw(lib, "hifihr_grad_norm", _fp(g) if gp is None else gp, count, gs, mx, vp(gd), vp(w), None)

    def step(pp=p, gp=g, mm=m, vv=v, count=nz, gs=0.5, t=1, st=None, gd=guard):
        return lambda: kc._raw(lib, "hifihr_adam_step_guarded", _fp(pp), _fp(gp), _fp(mm), _fp(vv), count, gs, LR, B1, B2, EPS, 0.0, t,
                               vp(st), vp(gd), None)
    null_f = ctypes.cast(None, ctypes.POINTER(ctypes.c_float))
    refused = {
        "norm: NULL grads": norm(gp=null_f), "norm: NULL guard": norm(gd=None), "norm: NULL workspace": norm(w=None),
        "norm: misaligned grads": norm(gp=_fp(g_off)), "norm: misaligned guard": norm(gd=guard_off), "norm: misaligned workspace": norm(w=ws_off),
        "norm: max_norm NaN": norm(mx=nan), "norm: max_norm 0": norm(mx=0.0), "norm: max_norm < 0": norm(mx=-1.0),
        "norm: max_norm -inf": norm(mx=-inf), "norm: grad_scale NaN": norm(gs=nan), "norm: grad_scale inf": norm(gs=inf),
        "step: NULL params": step(pp=None), "step: NULL grads": step(gp=None), "step: NULL exp_avg": step(mm=None),
        "step: NULL exp_avg_sq": step(vv=None), "step: NULL guard": step(gd=None),
        "step: misaligned params": step(pp=p_off), "step: misaligned grads": step(gp=g_off), "step: misaligned exp_avg": step(mm=p_off),
        "step: misaligned exp_avg_sq": step(vv=p_off), "step: misaligned guard": step(gd=guard_off),
        "step: misaligned state": step(st=state_off), "step: grad_scale NaN": step(gs=nan), "step: grad_scale inf": step(gs=-inf),
        "step: step 0 without a state": step(t=0), "step: step -1 without a state": step(t=-1),
    }
    for what, call in refused.items():
        kc._contract_rejects(call, G.wholes(), what)
    # n = 0 is accepted and is not a step: nothing written, no counter moves
    before = [w.clone() for w in G.wholes()]
    norm(count=ctypes.c_size_t(0))()
    step(count=ctypes.c_size_t(0))()
    step(count=ctypes.c_size_t(0), st=state, t=0)()
    for a, b in zip(G.wholes(), before):
        assert torch.equal(a, b), "n = 0 wrote something"
    # and the accepted call writes only inside its outputs (step 0 is fine WITH a state: the counted form ignores it)
    norm()()
    step(st=state, t=0)()
    step()()
    G.intact("grad guard")
    s = read_guard(lib, guard)
    assert (s["steps"], s["skipped"]) == (1, 0) and s["finite"], s
    assert struct.unpack("<dddddii", bytes(state.cpu().numpy().tobytes()))[5:] == (1, 0)
    assert not torch.equal(p.cpu(), torch.full((n,), 0.25))
