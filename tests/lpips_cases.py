"""Kernel-level cases of the LPIPS entries (csrc/lpips.hip) shared by tests/test_hostsim_lpips.py (emulator, device='cpu') and
tests/test_gpu_lpips.py (device='cuda'); the style of tests/kernel_cases.py.  Every figure is printed before it is asserted."""
import torch
import torch.nn.functional as F

import kernel_cases as kc
import lpips_ref as lr

C_FWD = kc.CONV_CONTRACT_C["fwd"]


def tap_case(lib, device, B, HW, C, seed=0, identical_sample=None):
    """hifihr_lpips_tap against the float64 restatement: per sample |got - ref| <= c sqrt(C HW) |ref| + 1e-30 (the project's contract
    form, L = the number of summed terms; a dropped 4-channel group costs >= 1/96 of the value), an identical sample exactly 0.0,
    two calls bit-identical, the accumulate flag adds onto a prefilled val."""
    f0, f1, w = lr.make_tap_inputs(B, HW, C, seed, identical_sample)
    ref = lr.tap_ref(f0.double(), f1.double(), w.double())
    f0d, f1d, wd = f0.to(device), f1.to(device), w.to(device)
    partial = torch.full((lib.lpips_tap_partial_floats(B),), float("nan"), device=device)       # any contents
    val = torch.full((B,), 7.0, device=device)
    lib.lpips_tap(f0d, f1d, wd, B, HW, C, partial, val, accumulate=False)
    got = val.cpu().double()
    err, bound = (got - ref).abs(), C_FWD * (C * HW) ** 0.5 * ref.abs() + 1e-30
    worst = float((err / bound).max())
    print(f"[lpips_tap] B={B} HW={HW} C={C}: max |got - ref| / bound = {worst:.3f} (ref {ref.tolist()})")
    assert bool((err <= bound).all()), f"tap B={B} HW={HW} C={C}: err {err.tolist()} vs bound {bound.tolist()}"
    if identical_sample is not None:
        assert float(got[identical_sample]) == 0.0, f"identical maps give {float(got[identical_sample])!r}, not exactly 0.0"
    val2 = torch.full((B,), -3.0, device=device)
    lib.lpips_tap(f0d, f1d, wd, B, HW, C, torch.zeros_like(partial), val2, accumulate=False)
    assert torch.equal(val, val2), "two calls differ in their bits"
    pre = torch.rand(B, generator=torch.Generator().manual_seed(seed + 1)).to(device)
    acc = pre.clone()
    lib.lpips_tap(f0d, f1d, wd, B, HW, C, partial, acc, accumulate=True)
    assert torch.equal(acc.cpu(), pre.cpu() + val.cpu()), "accumulate: val += tap"
    return worst


def tap_rejects_case(lib, device):
    """C % 4 != 0 and C above the documented cap: HIFIHR_EINVAL, val untouched."""
    cap = lib.lpips_tap_max_channels()
    assert cap >= 384 and cap % 4 == 0, cap
    for C in (6, cap + 4):
        B, HW = 2, 3
        f0, f1, w = torch.rand(B, HW, C).to(device), torch.rand(B, HW, C).to(device), torch.rand(C).to(device)
        partial = torch.zeros(lib.lpips_tap_partial_floats(B), device=device)
        val = torch.full((B,), 7.0, device=device)
        kc._contract_rejects(lambda: lib.lpips_tap(f0, f1, w, B, HW, C, partial, val), [val], f"lpips_tap C={C}")
    # the cap itself is served
    tap_case(lib, device, 1, 2, cap, seed=5)


def pool_notap_case(lib, device, N, H, W, C, seed=0):
    """hifihr_maxpool2d_fwd_notap (3, 2, 0) == F.max_pool2d bit for bit, ties (post-ReLU zeros) included."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, C, H, W, generator=gen))
    y = F.max_pool2d(x, 3, 2, 0)
    OH, OW = y.shape[2], y.shape[3]
    xd = x.permute(0, 2, 3, 1).contiguous().to(device)
    out = torch.full((N, OH, OW, C), 7.0, device=device)
    lib.maxpool2d_fwd_notap(xd, N, H, W, C, 3, 2, 0, out)
    assert torch.equal(out.cpu(), y.permute(0, 2, 3, 1)), f"maxpool notap {(N, H, W, C)} (exact)"


def pool_rejects_case(lib, device):
    N, H, W, C = 1, 9, 9, 8
    x = torch.rand(N, H, W, C).to(device)
    for (k, s, p) in ((3, 2, 2), (4, 2, 0)):
        out = torch.full((N, 8, 8, C), 7.0, device=device)
        kc._contract_rejects(lambda: lib.maxpool2d_fwd_notap(x, N, H, W, C, k, s, p, out), [out], f"maxpool2d_fwd_notap {(k, s, p)}")
    # the training pool keeps its documented set: (3, 2, 0) is not in it
    out = torch.full((N, 4, 4, C), 7.0, device=device)
    tap = torch.full((N * 4 * 4 * C,), 9, dtype=torch.uint8, device=device)
    kc._contract_rejects(lambda: lib.maxpool2d_fwd(x, N, H, W, C, 3, 2, 0, out, tap), [out, tap], "maxpool2d_fwd (3, 2, 0)")


def scale_repack_case(lib, device, B=2, H=9, W=7, seed=0):
    """hifihr_image_scale_to_nhwc4 == (x - shift) / scale to 1 ulp, fourth plane exactly zero."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=gen) * 2 - 1
    want = ((x - torch.tensor(lr.SHIFT).view(1, 3, 1, 1)) / torch.tensor(lr.SCALE).view(1, 3, 1, 1)).permute(0, 2, 3, 1)
    out = torch.full((B, H, W, 4), 7.0, device=device)
    lib.image_scale_to_nhwc4(x.to(device), out, lr.SHIFT, lr.SCALE)
    got = out.cpu()
    assert float(got[..., 3].abs().max()) == 0.0, "fourth plane is not exactly zero"
    ulp = torch.abs(torch.nextafter(want, torch.full_like(want, float("inf"))) - want)
    worst = float(((got[..., :3] - want).abs() / ulp).max())
    print(f"[image_scale] max error {worst:.2f} ulp")
    assert worst <= 1.0, f"scaling repack off by {worst} ulp"


def conv_bias_relu_contract_case(lib, device, N, H, W, C, K, R, stride, pad, seed=0):
    """hifihr_conv2d_fwd with bias + ReLU on one geometry: err <= c sqrt(C R S) max|ref| (float64 reference)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    w = torch.randn(K, C, R, R, generator=gen, dtype=torch.float64) / (C * R * R) ** 0.5
    b = torch.randn(K, generator=gen, dtype=torch.float64)
    ref = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad)).permute(0, 2, 3, 1)
    OH, OW = ref.shape[1], ref.shape[2]
    d = lambda t: t.float().to(device).contiguous()
    y = torch.full((N, OH, OW, K), 7.0, device=device)
    lib.conv2d_fwd(d(x.permute(0, 2, 3, 1)), d(w.permute(0, 2, 3, 1)), d(b), y, N, H, W, C, K, R, R, stride, pad, act=1)
    err, scale = float((y.cpu().double() - ref).abs().max()), float(ref.abs().max())
    bound = C_FWD * (C * R * R) ** 0.5 * scale
    print(f"[conv bias+relu] {(N, H, W, C, K, R, stride, pad)}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert err <= bound, f"conv {(N, H, W, C, K, R, stride, pad)}: err {err:.3e} vs bound {bound:.3e} (max|ref| {scale:.3e})"


# ------------------------------------------------------------------------------------------------
# end to end: hifihr_amd.lpips.LPIPS against the float64 restatement with the same weights
# ------------------------------------------------------------------------------------------------
E2E_FACTOR = 64.0      # HIP error <= 64 x the float32 CPU restatement's own error: the direct kernels sum each output in 16-channel chunks
                       # (the convolution contract bounds that order by c sqrt(L), tens of roundings) where torch's CPU convolution sums in blocks


def e2e_inputs(family, N=4, H=224, W=224, seed=0):
    """-> (in0, in1) in [-1, 1], float32 on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(N, 3, H, W, generator=gen) * 2 - 1
    b = torch.rand(N, 3, H, W, generator=gen) * 2 - 1
    if family == "independent":
        return a, b
    if family == "masked":                 # the evaluation pass's shape: both images under one binary mask, -1 outside it
        m = (torch.rand(N, 1, H, W, generator=gen) > 0.6).float()
        return a * m + (m - 1), b * m + (m - 1)
    if family == "near":                   # what a good reconstruction gives
        return a, a + 1e-3 * torch.randn(N, 3, H, W, generator=gen)
    if family == "identical":
        return a, a.clone()
    raise ValueError(family)


def e2e_measure(module, in0, in1):
    """-> (largest relative error of the HIP path over the batch, the same of the float32 CPU restatement (r32), got, ref64)."""
    convs, lins = lr.module_weights(module)
    ref = lr.lpips_alex_ref(in0, in1, convs, lins, torch.float64).reshape(-1)
    r32v = lr.lpips_alex_ref(in0, in1, convs, lins, torch.float32).reshape(-1).double()
    with torch.no_grad():
        out = module(in0.cuda(), in1.cuda())
    assert tuple(out.shape) == (in0.shape[0], 1, 1, 1) and out.dtype == torch.float32
    got = out.reshape(-1).cpu().double()
    den = ref.abs().clamp_min(1e-300)
    return float(((got - ref).abs() / den).max()), float(((r32v - ref).abs() / den).max()), got, ref
