"""The `lpips` loss term on the device: the backward kernels of csrc/lpips.hip through the C ABI (the emulator's cases again),
hifihr_amd.lpips.LPIPS(differentiable=True) end to end against float64 autograd of the restatement (tests/lpips_grad_ref.py), its
capture into a hipGraph, and the term inside LossFunction.

Precision rule (tests/lpips_cases.py): HIP error against float64 <= 64 x the float32 CPU restatement's own error on the same inputs, as
max |error| / max |float64 result|; profiles/lpips_loss_precision.txt holds the figures of the run that wrote it.  The end-to-end
inputs are the families of lpips_cases.e2e_inputs with in0 moved off the ReLU kinks and pool ties (lpips_loss_cases.clear_of_kinks: the
float64 reference alone must keep 1e-4 of each layer's max |z| away from them, which is asserted)."""
import warnings

import pytest
import torch

import lpips_loss_cases as ll
import lpips_ref as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


@pytest.fixture(scope="module")
def diff():
    from hifihr_amd.lpips import LPIPS
    return LPIPS(seed=0, differentiable=True).cuda()


@pytest.fixture(scope="module")
def metric():
    from hifihr_amd.lpips import LPIPS
    return LPIPS(seed=0).cuda()


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 64, 100, 128, 192, 256, 260, 384, 400, 512])
def test_lpips_tap_bwd(lib, C):
    for B, HW in ((1, 1), (3, 5), (1, 17)):
        ll.tap_bwd_case(lib, "cuda", B, HW, C, seed=C + HW)


@pytest.mark.parametrize("B,HW,C", [(1, 1030, 64), (3, 520, 384), (1, 260, 256)])
def test_lpips_tap_bwd_many_pixel_blocks(lib, B, HW, C):
    ll.tap_bwd_case(lib, "cuda", B, HW, C, seed=C)


def test_lpips_tap_bwd_rejects(lib):
    ll.tap_bwd_rejects_case(lib, "cuda")


@pytest.mark.parametrize("H,W", [(3, 3), (7, 8), (15, 16)])
def test_lpips_maxpool(lib, H, W):
    for C in (4, 64, 192):
        ll.pool_case(lib, "cuda", 2, H, W, C, seed=H + C)


def test_lpips_maxpool_rejects(lib):
    ll.pool_rejects_case(lib, "cuda")


def test_image_scale_to_nhwc4_bwd(lib):
    ll.scale_bwd_case(lib, "cuda")


@pytest.mark.parametrize("N,H,W,C,K,R,stride,pad", [(1, 31, 35, 4, 64, 11, 4, 2), (1, 7, 6, 64, 192, 5, 1, 2),
                                                    (2, 70, 77, 4, 64, 11, 4, 2)])      # the stem again: two samples, more than 64 pixels per phase
def test_alexnet_conv_backward_data(lib, N, H, W, C, K, R, stride, pad):
    ll.conv_dgrad_case(lib, "cuda", N, H, W, C, K, R, stride, pad, seed=R)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
# (N, H, W) = (3, 35, 47): maps of 8x11, 3x5, 1x2;  (2, 63, 67): 15x16, 7x7, 3x3
@pytest.mark.parametrize("N,H,W", [(3, 35, 47), (2, 63, 67)])
@pytest.mark.parametrize("family", ["independent", "near", "masked"])
def test_lpips_gradient_matches_float64_autograd(diff, metric, family, N, H, W):
    ll.e2e_grad_case(diff, metric, family, N, H, W, seed=H)


@pytest.mark.parametrize("N,H,W", [(3, 35, 47), (2, 63, 67)])
def test_gradient_of_identical_images_is_exactly_zero(diff, metric, N, H, W):
    import lpips_cases as lc
    in0, in1 = lc.e2e_inputs("identical", N, H, W, seed=H)
    x = in0.cuda().requires_grad_(True)
    val = diff(x, in1.cuda())
    assert torch.equal(val.detach(), metric(in0.cuda(), in1.cuda())) and float(val.detach().abs().max()) == 0.0
    val.sum().backward()
    assert tuple(x.grad.shape) == (N, 3, H, W) and float(x.grad.abs().max()) == 0.0, float(x.grad.abs().max())


def test_module_contract(diff, metric):
    """The default module still refuses gradients; the differentiable one refuses a target that requires one, stays frozen and in eval
    mode, and without a gradient to record runs the forward-only path."""
    x = (torch.rand(1, 3, 40, 40) * 2 - 1).cuda()
    g = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        metric(g, x)
    with pytest.raises(NotImplementedError):
        diff(x, g)
    with pytest.raises(NotImplementedError):
        diff(g, g)
    assert not diff.training and not diff.train().training and not any(p.requires_grad for p in diff.parameters())
    out = diff(g.detach(), x + 0.1)
    assert not out.requires_grad and torch.equal(out, metric(g.detach(), x + 0.1))
    with torch.no_grad():
        assert not diff(g, x + 0.1).requires_grad
    val = diff(g, x + 0.1)
    val.sum().backward()
    assert all(p.grad is None for p in diff.parameters()) and float(g.grad.abs().max()) > 0


def test_loss_backward_is_captured_into_a_graph(diff):
    """Forward + backward on static inputs under torch.cuda.graph: the replay matches the eager gradient within the precision rule (here:
    bit for bit is not required of it), two replays are bit-equal."""
    N, H, W = 2, 63, 67
    in0, in1, gval, v64, g64, v32, g32 = ll.e2e_reference(diff, "independent", N, H, W, H)
    x, y, gv = in0.cuda().requires_grad_(True), in1.cuda(), gval.cuda().view(N, 1, 1, 1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                                   # warm-up on the side stream: allocations, the weight re-layouts
            x.grad = None
            diff(x, y).backward(gv)
        eager = x.grad.clone()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    with torch.cuda.graph(graph):
        val = diff(x, y)
        val.backward(gv)
    static_grad = x.grad
    static_grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    first, first_val = static_grad.clone(), val.detach().clone()
    ll.assert_within_factor("LPIPS grad, graph replay", first, g64, g32)
    e, _ = ll.rel_errors(first, eager.cpu().double(), eager.cpu())           # replay against eager, on the same scale
    _, r32 = ll.rel_errors(eager, g64, g32)
    print(f"[LPIPS grad, graph replay] against eager: rel err {e:.3e} (bound {ll.FACTOR:.0f} x r32 = {ll.FACTOR * r32:.3e})")
    assert e <= ll.FACTOR * r32, "the replay does not match the eager gradient"
    static_grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_grad, first) and torch.equal(val.detach(), first_val), "two replays differ in their bits"


# ---- the loss term -------------------------------------------------------------------------------------------------------------
def _loss_inputs(B=2, H=47, seed=5):
    gen = torch.Generator().manual_seed(seed)
    re_img, imgs = torch.rand(B, 3, H, H, generator=gen), torch.rand(B, 3, H, H, generator=gen)
    seg = torch.zeros(B, H, H, dtype=torch.long)
    seg[:, 8:36, 10:40] = 1                                  # a block, so that whole receptive fields lie inside and outside the mask
    seg[:, 20:24, 20:30] = 0
    return re_img, imgs, seg


def test_loss_term(diff):
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    import lpips_grad_ref as lg
    args = options.make_args()
    assert args.lambda_lpips == 0.01
    re_img, imgs, seg = _loss_inputs()
    B = re_img.shape[0]
    convs, lins = lr.module_weights(diff)
    m = seg.unsqueeze(1).float()
    shift, scale = tuple((1.0 + s) / 2.0 for s in lr.SHIFT), tuple(s / 2.0 for s in lr.SCALE)      # normalize=True folded into the constants
    # the composite, moved off the kinks of the reference: inside the mask it is re_img, outside it the image (which is also the target --
    # the target's half has no kink to keep away from: it gets no gradient)
    comp = ll.clear_of_kinks(re_img * m + imgs * (1 - m), imgs, convs, lins, shift=shift, scale=scale)
    re_img, imgs = torch.where(m > 0, comp, re_img), torch.where(m > 0, imgs, comp)
    refs = {}
    for dt in (torch.float64, torch.float32):
        r = re_img.to(dt).clone().requires_grad_(True)
        rec = {}
        val = lg.lpips_alex_grad_ref(r * m.to(dt) + imgs.to(dt) * (1 - m.to(dt)), imgs, convs, lins, dt, shift, scale, record=rec)
        loss = args.lambda_lpips * val.mean()
        loss.backward()
        refs[dt] = (loss.detach(), r.grad, rec)
    assert ll.kink_report(refs[torch.float64][2]) == (0, 0)
    fn = LossFunction(lpips=diff)
    r = re_img.cuda().requires_grad_(True)
    outputs, examples = {"re_img": r}, {"imgs": imgs.cuda(), "segms_gt": seg.cuda()}
    dic = fn(examples, outputs, ["lpips"], "FreiHand", args)
    assert list(dic) == ["lpips"] and dic["lpips"].dim() == 0
    ll.assert_within_factor("loss_dic['lpips']", dic["lpips"].detach().reshape(1), refs[torch.float64][0].reshape(1), refs[torch.float32][0].reshape(1))
    fn.total(dic, ["lpips"]).backward()
    ll.assert_within_factor("d lpips / d re_img", r.grad, refs[torch.float64][1], refs[torch.float32][1])
    outside = (m == 0).expand_as(r.grad)
    assert float(r.grad.cpu()[outside].abs().max()) == 0.0, "the gradient outside the mask is not exactly 0"
    assert float(r.grad.cpu()[~outside].abs().max()) > 0
    # without the name: no module is built, no key
    plain = LossFunction()
    dic2 = plain(examples, {"re_img": r.detach()}, ["mtex"], "FreiHand", args)
    assert "lpips" not in dic2 and plain.lpips_loss is None


def test_loss_term_builds_its_module_on_first_use():
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.lpips import LPIPS
    args = options.make_args()
    re_img, imgs, seg = _loss_inputs()
    fn = LossFunction()
    assert fn.lpips_loss is None
    outputs, examples = {"re_img": re_img.cuda().requires_grad_(True)}, {"imgs": imgs.cuda(), "segms_gt": seg.cuda()}
    with pytest.warns(UserWarning, match="SEEDED"):
        a = fn(examples, outputs, ["lpips"], "FreiHand", args)["lpips"]
    assert isinstance(fn.lpips_loss, LPIPS) and fn.lpips_loss.differentiable and a.requires_grad
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # warned once
        b = fn(examples, outputs, ["lpips"], "FreiHand", args)["lpips"]
    assert torch.equal(a.detach(), b.detach())


# ---- inside the training step --------------------------------------------------------------------------------------------------
def _model(tables):
    from hifihr_amd.models import Model
    torch.manual_seed(0)
    return Model(True, torch.device("cuda"), False, "mano", False, "res18", mano_tables=tables).cuda().train()


def _batch(model, B, args):
    from hifihr_amd import synth
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda")
    return data_dic(synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, first_index=0, device=dev), "FreiHand", "training", args, device=dev)


def test_step_with_and_without_the_name(synth_tables):
    """Model + LossFunction at B = 2: with `lpips` added to the default list every other term keeps its bits and the new one is the module's
    value on the composite; the captured step with the term replays, its `lpips` has the bits of the eager step's, the parameters move."""
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, forward_backward
    from test_gpu_e2e import _warm_eager
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        B = 2
        base = options.baseline_config2_args(train_batch=B)
        args = options.baseline_config2_args(train_batch=B, losses=base.losses + ["lpips"])
        model, model2 = _model(synth_tables), _model(synth_tables)
        model2.load_state_dict(model.state_dict())
        ex = _batch(model, B, args)
        root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
        with torch.no_grad():
            out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
        lex = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
        lf = LossFunction()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            d0, d1 = lf(lex, out, base.losses, "FreiHand", base), lf(lex, out, args.losses, "FreiHand", args)
        assert set(d1) == set(d0) | {"lpips"} and all(torch.equal(d0[k], d1[k]) for k in d0)
        seg = lex["segms_gt"].unsqueeze(1)
        want = args.lambda_lpips * lf.lpips_loss(out["re_img"] * seg + lex["imgs"] * (1 - seg), lex["imgs"], normalize=True).mean()
        assert torch.equal(d1["lpips"], want) and bool(torch.isfinite(want)) and float(want) > 0
        opt, opt2 = FusedAdam(FlatParams(model), lr=1e-4), FusedAdam(FlatParams(model2), lr=1e-4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            g = GraphedTrainStep(model2, LossFunction(), opt2, ex, args, warmup=2)
            before = opt2.flatp.flat.detach().clone()
            _warm_eager(model, opt, ex, args)              # the first eager step of a model dispatches other kernels than every later one
            _, dic_e = forward_backward(model, LossFunction(), opt, ex, args)
        loss_g, dic_g = g()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_g)) and torch.equal(dic_e["lpips"].detach(), dic_g["lpips"].detach())
        assert float((opt2.flatp.flat.detach() - before).abs().max()) > 0.0
        loss_g2, _ = g()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss_g2))
        g.release()
    finally:
        torch.cuda.set_stream(prev)
