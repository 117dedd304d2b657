"""LPIPS(net="alex") on the device: the kernels of csrc/lpips.hip through the C ABI (the emulator's cases again, plus the real
sizes), hifihr_amd.lpips.LPIPS end to end against the float64 restatement of tests/lpips_ref.py, the weight loader, the
evaluation front-end and what the device executes.

End-to-end precision, measured on an MI355X (profiles/lpips_precision.txt has the figures of the run that wrote it): the
bound is 64 x r32, r32 = the largest relative error of the SAME restatement run in float32 by torch on the CPU against
float64, computed inside the test."""
import pytest
import torch

import kernel_cases as kc
import lpips_cases as lc
import lpips_ref as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


@pytest.fixture(scope="module")
def metric():
    from hifihr_amd.lpips import LPIPS
    return LPIPS(seed=0).cuda()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,same", [(2, 15 * 15, 64, 1), (3, 7 * 7, 192, 2), (1, 3 * 3, 384, None), (1, 3 * 3, 384, 0),
                                         (2, 5 * 3, 256, 1), (1, 1, 4, None), (1, 1, 4, 0),
                                         # the taps of a B = 32 call at 224 x 224
                                         (32, 3025, 64, 31), (32, 729, 192, 31), (32, 169, 384, 31), (32, 169, 256, 31)])
def test_lpips_tap(lib, B, HW, C, same):
    lc.tap_case(lib, "cuda", B, HW, C, seed=C + HW, identical_sample=same)


def test_lpips_tap_other_widths(lib):
    for C in (8, 100, 128, 176, 260, 320, 448):
        lc.tap_case(lib, "cuda", 2, 5, C, seed=C, identical_sample=1)
    lc.tap_case(lib, "cuda", 1, 64 * 4 * 2 + 3, 256, seed=3)


def test_lpips_tap_rejects(lib):
    lc.tap_rejects_case(lib, "cuda")


@pytest.mark.parametrize("N,H,W,C", [(2, 15, 15, 64), (1, 7, 9, 8), (1, 3, 3, 4), (16, 55, 55, 64), (16, 27, 27, 192)])
def test_maxpool_notap(lib, N, H, W, C):
    lc.pool_notap_case(lib, "cuda", N, H, W, C, seed=H + C)


def test_maxpool_notap_rejects(lib):
    lc.pool_rejects_case(lib, "cuda")


def test_image_scale_to_nhwc4(lib):
    lc.scale_repack_case(lib, "cuda")
    lc.scale_repack_case(lib, "cuda", B=3, H=224, W=224, seed=1)


@pytest.mark.parametrize("N,H,W,C,K,R,stride,pad", [(1, 31, 35, 4, 64, 11, 4, 2), (1, 7, 6, 64, 192, 5, 1, 2),
                                                    (8, 224, 224, 4, 64, 11, 4, 2), (8, 27, 27, 64, 192, 5, 1, 2)])
def test_alexnet_conv_geometries(lib, N, H, W, C, K, R, stride, pad):
    lc.conv_bias_relu_contract_case(lib, "cuda", N, H, W, C, K, R, stride, pad, seed=R)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,H,W", [("independent", 4, 224, 224), ("masked", 4, 224, 224), ("near", 4, 224, 224),
                                          ("independent", 3, 67, 95)])
def test_lpips_matches_float64_restatement(metric, family, N, H, W):
    """HIP path (direct kernels) vs float64 with the same seeded weights: largest relative error over the batch <= 64 x r32."""
    in0, in1 = lc.e2e_inputs(family, N, H, W, seed=H)
    rel, r32, got, ref = lc.e2e_measure(metric, in0, in1)
    print(f"[lpips e2e] {family} {N}x{H}x{W}: HIP rel err {rel:.3e}, r32 {r32:.3e}, ratio {rel / r32 if r32 > 0 else float('inf'):.2f} "
          f"(bound {lc.E2E_FACTOR:.0f}); values {got.tolist()}")
    assert bool((ref > 0).all()) and bool(torch.isfinite(got).all())
    assert rel <= lc.E2E_FACTOR * r32, f"{family}: HIP relative error {rel:.3e} > 64 x r32 = {lc.E2E_FACTOR * r32:.3e}"


@pytest.mark.parametrize("N,H,W", [(4, 224, 224), (3, 67, 95)])
def test_lpips_of_identical_images_is_exactly_zero(metric, N, H, W):
    in0, in1 = lc.e2e_inputs("identical", N, H, W, seed=H)
    with torch.no_grad():
        out = metric(in0.cuda(), in1.cuda())
    assert tuple(out.shape) == (N, 1, 1, 1)
    assert float(out.abs().max()) == 0.0, out.reshape(-1).tolist()


def test_lpips_is_deterministic_and_takes_unit_range_inputs(metric):
    in0, in1 = lc.e2e_inputs("independent", 2, 64, 80, seed=9)
    a, b = metric(in0.cuda(), in1.cuda()), metric(in0.cuda(), in1.cuda())
    assert torch.equal(a, b)
    # normalize=True: inputs in [0, 1], the rescale to [-1, 1] folded into the scaling constants
    c = metric((in0.cuda() + 1) / 2, (in1.cuda() + 1) / 2, normalize=True)
    assert float(((c - a).abs() / a.abs()).max()) <= 1e-4
    # the smallest input: one pixel left in the last three taps
    s0, s1 = lc.e2e_inputs("independent", 2, 31, 31, seed=3)
    rel, r32, got, ref = lc.e2e_measure(metric, s0, s1)
    print(f"[lpips e2e] 31x31: rel {rel:.3e} r32 {r32:.3e}")
    assert rel <= lc.E2E_FACTOR * r32


# ---- loader --------------------------------------------------------------------------------------------------------------------
def _seeded_tensors(seed=11):
    gen = torch.Generator().manual_seed(seed)
    convs = [(torch.randn(k, c, r, r, generator=gen) / (c * r * r) ** 0.5, torch.randn(k, generator=gen) * 0.1) for (c, k, r, *_x) in lr.ALEX]
    lins = [torch.rand(1, k, 1, 1, generator=gen) / k for (_, k, *_x) in lr.ALEX]
    return convs, lins


def _both_layouts(convs, lins):
    feat_idx, slices = (0, 3, 6, 8, 10), (1, 2, 3, 4, 5)
    tv = {"classifier.1.weight": torch.zeros(8, 8), "classifier.1.bias": torch.zeros(8)}          # ignored
    alex_pth, full = {}, {"scaling_layer.shift": torch.tensor(lr.SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(lr.SCALE).view(1, 3, 1, 1)}
    for i, ((w, b), lin) in enumerate(zip(convs, lins)):
        tv[f"features.{feat_idx[i]}.weight"], tv[f"features.{feat_idx[i]}.bias"] = w, b
        alex_pth[f"lin{i}.model.1.weight"] = lin
        full[f"net.slice{slices[i]}.{feat_idx[i]}.weight"], full[f"net.slice{slices[i]}.{feat_idx[i]}.bias"] = w, b
        full[f"lin{i}.model.1.weight"] = lin
    return (tv, alex_pth), (full,)


def test_loader_accepts_both_key_layouts():
    from hifihr_amd.lpips import LPIPS, load_state_dict_lpips
    convs, lins = _seeded_tensors()
    two, one = _both_layouts(convs, lins)
    a = load_state_dict_lpips(LPIPS(seed=1), *two).cuda()
    b = load_state_dict_lpips(LPIPS(seed=2), *one).cuda()
    in0, in1 = lc.e2e_inputs("independent", 2, 96, 64, seed=4)
    va, vb = a(in0.cuda(), in1.cuda()), b(in0.cuda(), in1.cuda())
    assert torch.equal(va, vb) and float(va.min()) > 0
    for m in (a, b):                                  # the loaded values are the seeded tensors, frozen
        for conv, (w, bias), p, lin in zip(m.convs, convs, m.lins, lins):
            assert torch.equal(conv.weight.cpu(), w) and torch.equal(conv.bias.cpu(), bias) and torch.equal(p.cpu(), lin.reshape(-1))
        assert not any(p.requires_grad for p in m.parameters()) and not m.training
    rel, r32, _, _ = lc.e2e_measure(a, in0, in1)      # ... and they are what the forward uses
    assert rel <= lc.E2E_FACTOR * r32
    # a missing tensor is named, and nothing is loaded
    c = LPIPS(seed=3)
    before = [p.clone() for p in c.parameters()]
    lacking = {k: v for k, v in one[0].items() if k != "lin3.model.1.weight"}
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        load_state_dict_lpips(c, lacking)
    assert all(torch.equal(p, q) for p, q in zip(c.parameters(), before))
    with pytest.raises(KeyError, match=r"features\.6\.bias"):
        load_state_dict_lpips(c, {k: v for k, v in two[0].items() if k != "features.6.bias"}, two[1])


# ---- front-end -----------------------------------------------------------------------------------------------------------------
def _eval_batches(B=3):
    gen = torch.Generator().manual_seed(2)
    for _ in range(2):
        out = {"joints": torch.rand(B, 21, 3, generator=gen).cuda(), "mano_verts": torch.rand(B, 778, 3, generator=gen).cuda(),
               "re_img": torch.rand(B, 3, 224, 224, generator=gen).cuda()}
        ex = {"imgs": torch.rand(B, 3, 224, 224, generator=gen).cuda(), "segms_gt": (torch.rand(B, 224, 224, generator=gen) > 0.6).long().cuda()}
        yield out, ex


def test_evaluator_reports_lpips(metric):
    from hifihr_amd.evaluate import Evaluator
    ev, plain, direct = Evaluator(lpips_fn=metric), Evaluator(), []
    for out, ex in _eval_batches():
        ev.collect(out, ex, "FreiHand")
        plain.collect(out, ex, "FreiHand")
        m = ex["segms_gt"].unsqueeze(1).float()
        direct.append(metric(out["re_img"] * m * 2 - 1, m * ex["imgs"] * 2 - 1).mean())
    s = ev.summary()
    want = float(torch.stack(direct).mean())
    assert s["lpips"] is not None and s["lpips"] > 0 and s["lpips"] == s["lpips"] and s["lpips"] != float("inf")
    assert s["lpips"] == want, (s["lpips"], want)
    assert 0 < s["psnr"] < 30 and 0 < s["ssim"] < 1
    assert plain.summary()["lpips"] is None


def test_refusals(metric):
    from hifihr_amd._lib import HifihrError
    from hifihr_amd.lpips import LPIPS
    with pytest.raises(NotImplementedError):
        LPIPS(net="vgg")
    with pytest.raises(NotImplementedError):
        LPIPS(net="squeeze")
    x = torch.rand(1, 3, 64, 64) * 2 - 1
    with pytest.raises(HifihrError):
        metric(x, x.clone())                                            # CPU tensors
    g = x.cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        metric(g, x.cuda())
    with pytest.raises(NotImplementedError):
        metric(x.cuda(), g)
    with torch.no_grad():                                               # ... and fine where no gradient is recorded
        assert float(metric(g, x.cuda())) == 0.0
    with pytest.raises(ValueError):
        metric(torch.rand(1, 3, 30, 64).cuda(), torch.rand(1, 3, 30, 64).cuda())
    with pytest.raises(ValueError):
        metric(torch.rand(1, 3, 64, 64).cuda(), torch.rand(2, 3, 64, 64).cuda())


# ---- what the device executes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["reference", "fast"])
def test_lpips_runs_on_the_hand_written_kernels(precision):
    """One LPIPS forward under the profiler (the check of tests/test_gpu_e2e.py's training-step test): no Tensile / rocBLAS / hipBLASLt /
    MIOpen / CK kernel, and between the last convolution and the result at most five launches that are not hifihr:: kernels."""
    from torch.profiler import ProfilerActivity, profile
    from hifihr_amd.lpips import LPIPS
    m = LPIPS(conv_precision=precision).cuda()
    in0, in1 = [t.cuda() for t in lc.e2e_inputs("independent", 4, 224, 224, seed=1)]
    for _ in range(2):
        m(in0, in1)
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            m(in0, in1)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    except Exception as e:                               # noqa: BLE001 -- the tracer is a measurement aid: its absence is not a failure of the metric
        pytest.skip(f"torch.profiler / roctracer unavailable on this box: {type(e).__name__}: {e}")
    kernels = [n for n in names if not (n.lower().startswith(("memcpy", "memset")) or "Memcpy" in n or "Memset" in n)]
    if len(kernels) < 8:
        pytest.skip(f"the tracer returned {len(kernels)} kernel records for a forward of >= 19 launches: profiler unavailable on this box")
    print(f"[lpips {precision}] {len(kernels)} launches: {kernels}")
    library = [n for n in kernels if n.startswith("Cijk_") or "miopen" in n.lower() or "rocblas" in n.lower() or "hipblaslt" in n.lower()
               or "ck::" in n or "tensile" in n.lower()]
    assert not library, sorted(set(library))
    assert any("lpips_tap_kernel" in n for n in kernels) and any("image_scale_to_nhwc4_kernel" in n for n in kernels)
    trunk = [i for i, n in enumerate(kernels) if "hifihr::" in n and "lpips_tap" not in n]          # repack, pools, convolutions
    tail = kernels[trunk[-1] + 1:]
    foreign = [n for n in tail if "hifihr::" not in n]
    assert len(foreign) <= 5, foreign
    assert len([n for n in kernels if "hifihr::" not in n]) <= 12, kernels
