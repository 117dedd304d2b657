"""Cases of the LPIPS backward entries (csrc/lpips.hip: hifihr_lpips_tap_bwd, hifihr_lpips_maxpool_fwd / _bwd,
hifihr_image_scale_to_nhwc4_bwd) and of LPIPS(differentiable=True), shared by tests/test_hostsim_lpips_loss.py (emulator,
device='cpu') and tests/test_gpu_lpips_loss.py (device='cuda'); the style of tests/lpips_cases.py.  Every figure is printed before it is
asserted.

The tolerance is the rule of tests/lpips_cases.py: the error of the HIP result against float64 is at most E2E_FACTOR (64) times the error
of the float32 CPU restatement (tests/lpips_grad_ref.py) against float64 on the same inputs, both as max |error| / max |float64 result|.
PRECISION collects the measured ratios (tools/lpips_precision.py-style record: profiles/lpips_loss_precision.txt)."""
import torch
import torch.nn.functional as F

import kernel_cases as kc
import lpips_cases as lc
import lpips_grad_ref as lg
import lpips_ref as lr

FACTOR = lc.E2E_FACTOR
PRECISION = []                     # (what, HIP error, float32 CPU error, both relative to max |ref|)
KINK_MARGIN = 1e-4                 # of a layer's max |pre-activation|: how near a ReLU kink or a pool tie the float64 reference may come


def rel_errors(got, ref64, ref32):
    """-> (HIP error, float32 restatement's error), max |. - ref64| / max |ref64|."""
    den = max(float(ref64.abs().max()), 1e-300)
    return float((got.detach().cpu().double() - ref64).abs().max()) / den, float((ref32.double() - ref64).abs().max()) / den


def assert_within_factor(what, got, ref64, ref32):
    e, r32 = rel_errors(got, ref64, ref32)
    PRECISION.append((what, e, r32))
    print(f"[{what}] HIP rel err {e:.3e}, r32 {r32:.3e}, ratio {e / r32 if r32 > 0 else (0.0 if e == 0 else float('inf')):.2f} (bound {FACTOR:.0f})")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert e <= FACTOR * r32, f"{what}: HIP relative error {e:.3e} > {FACTOR:.0f} x r32 = {FACTOR * r32:.3e}"
    return e, r32


# ------------------------------------------------------------------------------------------------
# hifihr_lpips_tap_bwd
# ------------------------------------------------------------------------------------------------
def tap_gval(B, seed):
    """A different incoming gradient per sample; with B > 1 the first is exactly 0."""
    g = 0.5 + torch.rand(B, generator=torch.Generator().manual_seed(seed + 17))
    if B > 1:
        g[0] = 0.0
    return g


def tap_bwd_case(lib, device, B, HW, C, seed=0):
    """hifihr_lpips_tap_bwd against float64 autograd of the restatement (zero-norm convention of tests/lpips_grad_ref.py) on the inputs of the
    forward's cases -- all-zero pixels in f0 only, in both maps and in f1 only; with B > 1 the last sample's maps are identical.
    accumulate off over a NaN-filled output (overwritten), two calls bit-identical, a sample whose gval is 0 and the identical sample
    exactly 0, accumulate on over a non-zero gf0 = that tensor + the gradient, bit for bit."""
    same = B - 1 if B > 1 else None
    f0, f1, w = lr.make_tap_inputs(B, HW, C, seed, same)
    gval = tap_gval(B, seed)
    ref64 = lg.tap_bwd_ref(f0, f1, w, gval, torch.float64)
    ref32 = lg.tap_bwd_ref(f0, f1, w, gval, torch.float32)
    assert bool(torch.isfinite(ref64).all())
    f0d, f1d, wd, gd = f0.to(device), f1.to(device), w.to(device), gval.to(device)
    got = torch.full((B, HW, C), float("nan"), device=device)
    lib.lpips_tap_bwd(f0d, f1d, wd, gd, B, HW, C, got, accumulate=False)
    what = f"lpips_tap_bwd B={B} HW={HW} C={C}"
    assert_within_factor(what, got, ref64, ref32)
    # the same rule on the pixels where f0 is not all zero: an all-zero pixel's q / 1e-10 is ten orders larger and would hide the rest
    live = (f0.abs().sum(-1) > 0)
    if bool(live.any()) and not bool(live.all()):
        assert_within_factor(what + " (pixels with |f0| > 0)", got.cpu()[live], ref64[live], ref32[live])
    if B > 1:
        assert float(got[0].abs().max()) == 0.0, f"{what}: gval = 0 gives {float(got[0].abs().max())!r}, not exactly 0"
        assert float(got[same].abs().max()) == 0.0, f"{what}: identical maps give {float(got[same].abs().max())!r}, not exactly 0"
    again = torch.full((B, HW, C), -3.0, device=device)
    lib.lpips_tap_bwd(f0d, f1d, wd, gd, B, HW, C, again, accumulate=False)
    assert torch.equal(got, again), f"{what}: two calls differ in their bits"
    pre = (torch.randn(B, HW, C, generator=torch.Generator().manual_seed(seed + 1)) + 2.0)
    acc = pre.clone().to(device)
    lib.lpips_tap_bwd(f0d, f1d, wd, gd, B, HW, C, acc, accumulate=True)
    assert torch.equal(acc.cpu(), pre + got.cpu()), f"{what}: accumulate: gf0 += gradient"
    # hifihr_lpips_tap_bwd_relu: the same sums where f0 > 0, exactly 0 elsewhere -- with and without an arriving gradient
    for prefill in (None, pre):
        m = torch.full((B, HW, C), float("nan"), device=device) if prefill is None else prefill.clone().to(device)
        lib.lpips_tap_bwd(f0d, f1d, wd, gd, B, HW, C, m, accumulate=prefill is not None, relu=True)
        full = got.cpu() if prefill is None else acc.cpu()
        assert torch.equal(m.cpu(), torch.where(f0 > 0, full, torch.zeros(()))), f"{what}: the ReLU-masked entry is not [f0 > 0] x the unmasked sum"


def tap_bwd_rejects_case(lib, device):
    """What hifihr_lpips_tap refuses (C % 4 != 0, C above the cap) and a NULL gval / gf0: HIFIHR_EINVAL, gf0 untouched; the cap is served."""
    cap = lib.lpips_tap_max_channels()
    B, HW = 2, 3
    for C in (6, cap + 4):
        f0, f1, w = torch.rand(B, HW, C).to(device), torch.rand(B, HW, C).to(device), torch.rand(C).to(device)
        g, out = torch.ones(B, device=device), torch.full((B, HW, C), 7.0, device=device)
        kc._contract_rejects(lambda: lib.lpips_tap_bwd(f0, f1, w, g, B, HW, C, out), [out], f"lpips_tap_bwd C={C}")
        kc._contract_rejects(lambda: lib.lpips_tap_bwd(f0, f1, w, g, B, HW, C, out, relu=True), [out], f"lpips_tap_bwd_relu C={C}")
    C = 8
    f0, f1, w = torch.rand(B, HW, C).to(device), torch.rand(B, HW, C).to(device), torch.rand(C).to(device)
    g, out = torch.ones(B, device=device), torch.full((B, HW, C), 7.0, device=device)
    for name, call in (("gval", lambda: lib.lpips_tap_bwd(f0, f1, w, None, B, HW, C, out)), ("gf0", lambda: lib.lpips_tap_bwd(f0, f1, w, g, B, HW, C, None)),
                       ("f1", lambda: lib.lpips_tap_bwd(f0, None, w, g, B, HW, C, out)), ("B = 0", lambda: lib.lpips_tap_bwd(f0, f1, w, g, 0, HW, C, out)),
                       ("HW = 0", lambda: lib.lpips_tap_bwd(f0, f1, w, g, B, 0, C, out)),
                       ("gval (relu)", lambda: lib.lpips_tap_bwd(f0, f1, w, None, B, HW, C, out, relu=True))):
        kc._contract_rejects(call, [out], f"lpips_tap_bwd NULL / bad {name}")
    tap_bwd_case(lib, device, 1, 2, cap, seed=5)


# ------------------------------------------------------------------------------------------------
# hifihr_lpips_maxpool_fwd / _bwd
# ------------------------------------------------------------------------------------------------
def pool_inputs(N, H, W, C, seed):
    """-> (x [N,C,H,W] with about 30 % exact zeros and positive values drawn from six levels -- ties in most windows --, gy on a 1/16 grid:
    every sum of gy values is exact in float32, so the float32 gather and torch's float64 backward must agree in every bit)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(1, 7, (N, C, H, W), generator=gen).float() / 4
    x = torch.where(torch.rand(N, C, H, W, generator=gen) < 0.3, torch.zeros(()), x)
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    gy = torch.randint(-64, 65, (N, C, OH, OW), generator=gen).float() / 16
    return x, gy


def pool_case(lib, device, N, H, W, C, seed=0):
    """forward == F.max_pool2d(x, 3, 2) bit for bit; backward == torch's float64 backward bit for bit (first maximum in row-major window
    order), dx overwritten, rows / columns that no window covers exactly 0, two calls bit-identical."""
    x, gy = pool_inputs(N, H, W, C, seed)
    y = F.max_pool2d(x, 3, 2)
    OH, OW = y.shape[2], y.shape[3]
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 2).backward(gy.double())
    want = x64.grad.permute(0, 2, 3, 1)
    xd, gyd = x.permute(0, 2, 3, 1).contiguous().to(device), gy.permute(0, 2, 3, 1).contiguous().to(device)
    out = torch.full((N, OH, OW, C), 7.0, device=device)
    lib.lpips_maxpool_fwd(xd, N, H, W, C, out)
    assert torch.equal(out.cpu(), y.permute(0, 2, 3, 1)), f"lpips_maxpool_fwd {(N, H, W, C)} (exact)"
    dx = torch.full((N, H, W, C), float("nan"), device=device)
    lib.lpips_maxpool_bwd(gyd, xd, N, H, W, C, dx)
    got = dx.cpu()
    assert torch.equal(got.double(), want), f"lpips_maxpool_bwd {(N, H, W, C)}: {int((got.double() != want).sum())} elements differ from torch's backward"
    assert float(got[:, 2 * OH + 1:].abs().sum()) == 0.0 and float(got[:, :, 2 * OW + 1:].abs().sum()) == 0.0, "uncovered rows / columns are not exactly 0"
    dx2 = torch.full((N, H, W, C), -3.0, device=device)
    lib.lpips_maxpool_bwd(gyd, xd, N, H, W, C, dx2)
    assert torch.equal(dx, dx2), "two calls differ in their bits"
    PRECISION.append((f"lpips_maxpool_fwd/bwd {(N, H, W, C)}", 0.0, 0.0))


def pool_rejects_case(lib, device):
    """C % 4 != 0, H < 3, W < 3, a NULL pointer: HIFIHR_EINVAL, outputs untouched."""
    for (N, H, W, C) in ((1, 5, 5, 6), (1, 2, 5, 8), (1, 5, 2, 8)):
        x, gy = torch.rand(N, H, W, C).to(device), torch.rand(N, 2, 2, C).to(device)
        y, dx = torch.full((N, 2, 2, C), 7.0, device=device), torch.full((N, H, W, C), 7.0, device=device)
        kc._contract_rejects(lambda: lib.lpips_maxpool_fwd(x, N, H, W, C, y), [y], f"lpips_maxpool_fwd {(N, H, W, C)}")
        kc._contract_rejects(lambda: lib.lpips_maxpool_bwd(gy, x, N, H, W, C, dx), [dx], f"lpips_maxpool_bwd {(N, H, W, C)}")
    N, H, W, C = 1, 5, 5, 8
    x, gy = torch.rand(N, H, W, C).to(device), torch.rand(N, 2, 2, C).to(device)
    y, dx = torch.full((N, 2, 2, C), 7.0, device=device), torch.full((N, H, W, C), 7.0, device=device)
    for name, call in (("fwd x", lambda: lib.lpips_maxpool_fwd(None, N, H, W, C, y)), ("fwd y", lambda: lib.lpips_maxpool_fwd(x, N, H, W, C, None)),
                       ("bwd gy", lambda: lib.lpips_maxpool_bwd(None, x, N, H, W, C, dx)), ("bwd x", lambda: lib.lpips_maxpool_bwd(gy, None, N, H, W, C, dx)),
                       ("bwd dx", lambda: lib.lpips_maxpool_bwd(gy, x, N, H, W, C, None))):
        kc._contract_rejects(call, [y, dx], f"lpips_maxpool NULL {name}")


# ------------------------------------------------------------------------------------------------
# hifihr_image_scale_to_nhwc4_bwd
# ------------------------------------------------------------------------------------------------
def scale_bwd_case(lib, device, B=2, H=9, W=7, seed=0):
    """gimg = g4[..., c] / scale[c] (closed form): within 1 ulp of the float32 expression (true division, as the forward), within the factor
    rule of float64, the fourth plane ignored, gimg overwritten."""
    gen = torch.Generator().manual_seed(seed)
    g4 = torch.randn(B, H, W, 4, generator=gen)
    sc32 = torch.tensor(lr.SCALE).view(1, 3, 1, 1)
    want32 = g4[..., :3].permute(0, 3, 1, 2) / sc32
    want64 = g4[..., :3].permute(0, 3, 1, 2).double() / sc32.double()
    out = torch.full((B, 3, H, W), float("nan"), device=device)
    lib.image_scale_to_nhwc4_bwd(g4.to(device), out, lr.SCALE)
    got = out.cpu()
    ulp = torch.abs(torch.nextafter(want32, torch.full_like(want32, float("inf"))) - want32)
    worst = float(((got - want32).abs() / ulp).max())
    print(f"[image_scale_bwd] max error {worst:.2f} ulp")
    assert worst <= 1.0, f"scaling backward off by {worst} ulp"
    assert_within_factor(f"image_scale_to_nhwc4_bwd {(B, H, W)}", got, want64, want32)
    g4b = g4.clone()
    g4b[..., 3] = 1e30                                     # the fourth plane does not reach the result
    out2 = torch.full((B, 3, H, W), -3.0, device=device)
    lib.image_scale_to_nhwc4_bwd(g4b.to(device), out2, lr.SCALE)
    assert torch.equal(out, out2)
    kc._contract_rejects(lambda: lib.image_scale_to_nhwc4_bwd(g4.to(device), out2, (0.458, 0.0, 0.45)), [out2], "image_scale_to_nhwc4_bwd scale = 0")
    kc._contract_rejects(lambda: lib.image_scale_to_nhwc4_bwd(None, out2, lr.SCALE), [out2], "image_scale_to_nhwc4_bwd NULL g4")


# ------------------------------------------------------------------------------------------------
# the AlexNet geometries' backward-data (hifihr_conv2d_bwd_data), with the convolution contract's bound
# ------------------------------------------------------------------------------------------------
def conv_dgrad_case(lib, device, N, H, W, C, K, R, stride, pad, seed=0):
    """hifihr_conv2d_bwd_data on one geometry against float64 autograd: err <= c sqrt(K ceil(R/s)^2) max|ref| (tests/kernel_cases.py)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(K, C, R, R, generator=gen, dtype=torch.float64) / (C * R * R) ** 0.5
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(gy)
    ref = x.grad.permute(0, 2, 3, 1)
    d = lambda t: t.float().to(device).contiguous()
    geo = (N, H, W, C, K, R, R, stride, pad)
    out = torch.full((N, H, W, C), 7.0, device=device)
    scratch = torch.empty(K * R * R * C, device=device)
    lib.conv2d_bwd_data(d(gy.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), out, scratch, *geo)
    Ld = K * -(-R // stride) * -(-R // stride)
    err, scale = float((out.cpu().double() - ref).abs().max()), float(ref.abs().max())
    print(f"[conv bwd_data] {geo}: err {err:.3e} bound {kc.CONV_CONTRACT_C['dgrad'] * Ld ** 0.5 * scale + 1e-12:.3e}")
    kc._contract_close("bwd_data", out, ref, Ld, f"bwd_data {geo}", "dgrad")


# ------------------------------------------------------------------------------------------------
# end to end: LPIPS(differentiable=True) against float64 autograd of the restatement with the same weights
# ------------------------------------------------------------------------------------------------
def kink_report(record):
    """How near the float64 reference comes to a point where its gradient jumps, for in0's half (the target's half gets no gradient, and
    the value is continuous in it).  -> (ReLU: the number of pre-activations within KINK_MARGIN x their layer's max |z| of 0; pool: the number
    of windows whose two largest values are closer than KINK_MARGIN x the pool input's max).  A window whose maximum is 0 is not counted:
    its input is a ReLU's output, every tap of it is an exact 0 whose pre-activation is <= 0, and whichever tap wins the ReLU passes nothing."""
    relu = 0
    for z in record["pre"]:
        relu += int((z.abs() < KINK_MARGIN * float(z.abs().max())).sum())
    pool = 0
    for p in record["pool"]:
        win = F.unfold(p.reshape(-1, 1, p.shape[2], p.shape[3]), 3, stride=2)            # [N*C, 9, windows]
        top = win.topk(2, dim=1).values
        pool += int(((top[:, 0] > 0) & ((top[:, 0] - top[:, 1]) < KINK_MARGIN * float(p.abs().max()))).sum())
    return relu, pool


def _kink_hinge(record, margin):
    """sum of (margin x scale - distance) over every pre-activation / pool window nearer than margin x scale to its kink (differentiable)."""
    total = 0.0
    for z in record["pre"]:
        total = total + F.relu(margin * float(z.detach().abs().max()) - z.abs()).sum()
    for p in record["pool"]:
        win = F.unfold(p.reshape(-1, 1, p.shape[2], p.shape[3]), 3, stride=2)
        top = win.topk(2, dim=1).values
        gap = top[:, 0] - top[:, 1]
        total = total + (F.relu(margin * float(p.detach().abs().max()) - gap) * (top[:, 0] > 0)).sum()
    return total


def clear_of_kinks(in0, in1, convs, lins, max_iter=60, shift=lr.SHIFT, scale=lr.SCALE):
    """-> in0 moved (by ~1e-5 per element, float64 on the CPU) until the reference satisfies kink_report == (0, 0).
    Why the inputs are moved rather than a seed chosen: of the ~3e4 .. 7e4 pre-activations of one case about 3e-4 lie within 1e-4 x max |z|
    of 0 whatever the seed (measured: 4 .. 32 of them and 2 .. 15 pool windows per case over six seeds each), so a clean seed turns up
    about once in e^10 .. e^30 draws.  Each round takes one Polyak step on the hinge of the offenders at twice the margin."""
    x = in0.double().clone()
    for _ in range(max_iter):
        rec = {"graph": True}
        xr = x.clone().requires_grad_(True)
        lg.lpips_alex_grad_ref(xr, in1, convs, lins, torch.float64, shift, scale, record=rec)
        if kink_report({"pre": [t.detach() for t in rec["pre"]], "pool": [t.detach() for t in rec["pool"]]}) == (0, 0):
            break
        h = _kink_hinge(rec, 2 * KINK_MARGIN)
        g, = torch.autograd.grad(h, xr)
        x = x - 1.25 * float(h.detach()) / float(g.pow(2).sum()) * g
    return x.float()


E2E_CACHE = {}


def e2e_reference(module, family, N, H, W, seed):
    """-> (in0, in1, gval, val64, grad64, val32, grad32): the case's inputs (lpips_cases.e2e_inputs, in0 cleared of kinks) and the float64 /
    float32 value and gradient of the restatement with the module's weights, computed once per case and shared.  ASSERTS the condition of
    the comparison: the float64 reference has no pre-activation and no pool window within KINK_MARGIN of a kink (kink_report)."""
    key = (family, N, H, W, seed)
    if key not in E2E_CACHE:
        in0, in1 = lc.e2e_inputs(family, N, H, W, seed)
        convs, lins = lr.module_weights(module)
        in0 = clear_of_kinks(in0, in1, convs, lins)
        gval = 0.5 + torch.rand(N, generator=torch.Generator().manual_seed(seed + 3))
        rec = {}
        v64, g64 = lg.lpips_value_and_grad(in0, in1, convs, lins, torch.float64, gval, record=rec)
        v32, g32 = lg.lpips_value_and_grad(in0, in1, convs, lins, torch.float32, gval)
        kinks = kink_report(rec)
        print(f"[lpips loss e2e] {family} {N}x{H}x{W}: pre-activations / pool windows within {KINK_MARGIN:g} of a kink: {kinks}")
        assert kinks == (0, 0), f"{family} {N}x{H}x{W}: the float64 reference is within {KINK_MARGIN:g} of {kinks} kinks"
        E2E_CACHE[key] = (in0, in1, gval, v64, g64, v32, g32)
    return E2E_CACHE[key]


def e2e_grad_case(diff, metric, family, N, H, W, seed):
    """LPIPS(differentiable=True) on the device: the value is the forward-only module's bit for bit, d sum_b gval[b] val[b] / d in0 is within
    the factor rule of float64 autograd, two backward passes give the same bits."""
    in0, in1, gval, v64, g64, v32, g32 = e2e_reference(diff, family, N, H, W, seed)
    x = in0.cuda().requires_grad_(True)
    val = diff(x, in1.cuda())
    assert tuple(val.shape) == (N, 1, 1, 1) and val.dtype == torch.float32
    with torch.no_grad():
        assert torch.equal(val.detach(), metric(in0.cuda(), in1.cuda())), "the differentiable forward is not the forward-only module's bit for bit"
    val.backward(gval.cuda().view(N, 1, 1, 1))
    got = x.grad.clone()
    what = f"LPIPS grad {family} {N}x{H}x{W}"
    assert_within_factor(what + " (value)", val.detach().reshape(-1), v64, v32)
    assert_within_factor(what, got, g64, g32)
    x.grad = None
    diff(x, in1.cuda()).backward(gval.cuda().view(N, 1, 1, 1))
    assert torch.equal(got, x.grad), f"{what}: two backward passes differ in their bits"
    return got
