"""The soft silhouette and its losses on the MI355X: hifihr_soft_sil_fwd / _bwd and hifihr_soft_sil_loss_fwd / _bwd through the C ABI on
the cases of tests/test_hostsim_soft_silhouette.py (tests/soft_sil_cases.py; reference: the float64 restatement of tests/soft_sil_ref.py),
and the Python surface end to end: ops.soft_silhouette / ops.soft_sil_losses, Model(soft_silhouette=True), the loss terms "sil_soft" /
"iou_soft", the eager and the captured training step."""
import pytest
import torch

import soft_sil_cases as sc
import soft_sil_ref as sr

pytestmark = pytest.mark.gpu
_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


def test_known_answers(lib):
    sc.known_answers_case(lib, "cuda")


@pytest.mark.parametrize("case", sc.RANDOM_CASES, ids=_ids)
def test_random_meshes_match_the_restatement(lib, case):
    sc.random_case(lib, "cuda", *case)


def test_mano_topology_matches_the_restatement(lib, synth_tables):
    sc.mano_case(lib, "cuda", synth_tables, 64)


def test_mano_topology_at_full_size(lib, synth_tables):
    """B = 2, H = 224, sigma = 1e-4: what the model runs (14 x 14 tiles, seven passes of the face list).  The float64 restatement runs on the
    GPU, the float32 one of the admission rule on the CPU; the pairs inside the participation gap: soft_sil_cases.mano_case."""
    sc.mano_case(lib, "cuda", synth_tables, 224, ref_device="cuda")


def test_outputs_are_fully_written_and_repeatable(lib):
    sc.buffers_case(lib, "cuda")


def test_refusals_leave_the_outputs_untouched(lib):
    sc.refusal_case(lib, "cuda")


@pytest.mark.parametrize("shape", sc.LOSS_SHAPES, ids=_ids)
def test_losses_match_the_float64_formulas(lib, shape):
    sc.losses_case(lib, "cuda", *shape)


def test_losses_take_a_float_mask(lib):
    sc.losses_case(lib, "cuda", 2, 17, mask_dtype=torch.float32)


def test_empty_image_gives_nan_like_iou(lib):
    sc.losses_nan_case(lib, "cuda")


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_ops_match_the_restatement_through_autograd(lib):
    """ops.soft_silhouette (default blur_radius) -> ops.soft_sil_losses -> backward to the vertices, against the float64 restatement of the
    same chain; the bounds are those of the kernel cases (the losses add 1e-6)."""
    from hifihr_amd import ops
    H, B, F, sigma, kind, seed = sc.RANDOM_CASES[5]
    verts, faces, cam, _ = sc.make_inputs(H, B, F, kind, seed)
    mask = (torch.rand(B, H, H, generator=torch.Generator().manual_seed(1)) > 0.5).long()
    handle = ops.RendererHandle(faces.numpy(), verts.shape[1], image_size=H, aa=1)
    v = verts.cuda().requires_grad_(True)
    alpha = ops.soft_silhouette(handle, v, cam.cuda(), sigma)
    assert tuple(alpha.shape) == (B, 1, H, H)
    out = ops.soft_sil_losses(alpha, mask.cuda(), 0.005, 1e-3)
    (out * torch.tensor([3.0, 100.0], device="cuda")).sum().backward()
    # the restatement: d loss / d alpha by autograd in float64, then through the silhouette with that as w
    ref0 = sr.soft_silhouette(verts, faces, cam, H, sc.f32(sigma), sc.f32(sr.default_blur(sigma)))
    a = ref0["alpha"].clone().requires_grad_(True)
    lo = sr.losses(a.unsqueeze(1), mask, sc.f32(0.005), sc.f32(1e-3))
    (lo * torch.tensor([3.0, 100.0], dtype=torch.float64)).sum().backward()
    ref = sr.soft_silhouette(verts, faces, cam, H, sc.f32(sigma), sc.f32(sr.default_blur(sigma)), w=a.grad)
    assert ref["gap"] >= sr.GAP
    e = sc.errors(alpha.detach()[:, 0].double().cpu(), ref["S"], v.grad.double().cpu(), ref)
    rel = ((out.detach().double().cpu() - lo.detach()).abs() / lo.detach().abs()).max()
    print(f"[soft_sil] ops chain: alpha {e['alpha']:.3f} grad_max {e['grad_max']:.3f} grad_l2 {e['grad_l2']:.3f} of their bounds; losses {float(rel):.2e}")
    assert e["alpha"] <= 1.0 and e["grad_max"] <= 1.0 and e["grad_l2"] <= 1.0 and float(rel) <= 1e-5


def _batch(model, B, args, graded=False):
    from hifihr_amd import synth
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda")
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, first_index=0, device=dev)
    if graded:
        from test_gpu_e2e import graded_images
        sample["trans_images"] = graded_images(sample["trans_images"])
    return data_dic(sample, "FreiHand", "training", args, device=dev)


def _model(tables, **kw):
    from hifihr_amd.models import Model
    torch.manual_seed(0)
    return Model(True, torch.device("cuda"), False, "mano", False, "res18", mano_tables=tables, **kw).cuda().train()


def _check_soft_output(out, B, H):
    soft = out["re_sil_soft"]
    assert tuple(soft.shape) == (B, 1, H, H) and float(soft.min()) >= 0.0 and float(soft.max()) <= 1.0
    centre = out["face_id"][:, 1::3, 1::3] >= 0                       # the centre sample of the aa = 3 grid is the pixel centre
    covered = (out["re_sil"][:, 0] == 255) & centre
    assert int(covered.sum()) > 100 and float(soft[:, 0][covered].min()) >= 0.5


def test_model_outputs_with_and_without_the_option(synth_tables):
    from hifihr_amd import options
    args = options.baseline_config2_args(train_batch=2)
    off, off2, on = _model(synth_tables), _model(synth_tables, soft_silhouette=False), _model(synth_tables, soft_silhouette=True, soft_sil_sigma=1e-4)
    ex = _batch(off, 2, args)
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    with torch.no_grad():
        outs = [m("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root) for m in (off, off2, on)]
    assert set(outs[0]) == set(outs[1]) and "re_sil_soft" not in outs[0]
    assert set(outs[2]) == set(outs[0]) | {"re_sil_soft"}
    assert torch.equal(outs[0]["re_sil"], outs[2]["re_sil"]) and torch.equal(outs[0]["_rgba"], outs[2]["_rgba"])      # same seed, same weights
    _check_soft_output(outs[2], 2, 224)


def test_nimble_tail_emits_the_soft_silhouette(synth_tables):
    from hifihr_amd import ops, options, synth
    from hifihr_amd.models import Model
    from hifihr_amd.nimble_tables import synthetic_nimble_tables
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda")
    args = options.baseline_config3_args(train_batch=2, pretrain="res18", hand_model="nimble")
    torch.manual_seed(0)
    kw = dict(nimble_tables=synthetic_nimble_tables(0), mano_tables=synth_tables)
    model = Model(True, dev, False, "nimble", False, "res18", soft_silhouette=True, **kw).to(dev).train()
    mano, rend = ops.ManoLayerHandle(synth_tables), ops.RendererHandle(synth_tables.faces, 778, image_size=224, aa=3)
    ex = data_dic(synth.make_batch(mano, rend, 2, device=dev), "FreiHand", "training", args, device=dev)
    with torch.no_grad():
        out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=ex["joints"][:, args.ROOT, :].unsqueeze(1))
    _check_soft_output(out, 2, 224)


def _head_grads(model):
    enc = model.hand_encoder
    return {name: max((float(p.grad.abs().max()) if p.grad is not None else 0.0) for p in mod.parameters())
            for name, mod in (("shape", enc.shape_reg), ("pose", enc.pose_reg))}


def test_soft_terms_move_the_shape_and_pose_heads(synth_tables):
    """The point of the feature: with ONLY the hard `sil` / `iou` terms the hand encoder's gradient is exactly zero; with only their soft
    counterparts it is not.  Also: the step with the two terms added to the default list gives a finite loss, and the one-launch total
    equals the stack-and-sum form."""
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import forward_backward
    base = options.baseline_config2_args(train_batch=2)
    model = _model(synth_tables, soft_silhouette=True)
    opt = FusedAdam(FlatParams(model), lr=1e-6)
    ex = _batch(model, 2, base)
    grads = {}
    for tag, losses in (("all", base.losses + ["sil_soft", "iou_soft"]), ("soft", ["sil_soft", "iou_soft"]), ("hard", ["sil", "iou"])):
        args = options.baseline_config2_args(train_batch=2, losses=losses)
        lf = LossFunction()
        loss, dic = forward_backward(model, lf, opt, ex, args)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(dic[k])) for k in losses), {k: float(dic[k]) for k in losses}
        stacked = torch.stack([dic[k].detach() for k in losses]).sum()
        assert abs(float(loss) - float(stacked)) <= 1e-6 * abs(float(stacked)), (tag, float(loss), float(stacked))
        if tag != "hard":
            assert [names for _, _, names in lf._total_parts][-1] == ["sil_soft", "iou_soft"]
        grads[tag] = _head_grads(model)
    print("[soft_sil] max |grad| of the shape / pose heads:", grads)
    assert grads["hard"] == {"shape": 0.0, "pose": 0.0}
    assert grads["soft"]["shape"] > 0.0 and grads["soft"]["pose"] > 0.0 and grads["all"]["shape"] > 0.0 and grads["all"]["pose"] > 0.0


def test_graphed_step_with_the_option_matches_the_eager_step(synth_tables):
    """test_gpu_e2e.test_graphed_step_matches_eager_step with the option on and the two terms requested, one step, the same tolerance."""
    from test_gpu_e2e import _GRAPH_LOSS_RTOL
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, forward_backward, train_step
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        B, lr = 4, 1e-6
        base = options.baseline_config2_args(train_batch=B)
        args = options.baseline_config2_args(train_batch=B, losses=base.losses + ["sil_soft", "iou_soft"])
        model, model2 = _model(synth_tables, soft_silhouette=True), _model(synth_tables, soft_silhouette=True)
        model2.load_state_dict(model.state_dict())
        ex = _batch(model, B, args, graded=True)
        opt, opt2 = FusedAdam(FlatParams(model), lr=lr), FusedAdam(FlatParams(model2), lr=lr)
        g = GraphedTrainStep(model2, LossFunction(), opt2, ex, args, warmup=2)
        bufs = [b.clone() for b in model.buffers()]         # one eager forward + backward first: later steps dispatch what the graph replays
        forward_backward(model, LossFunction(), opt, ex, args)
        with torch.no_grad():
            for b, s0 in zip(model.buffers(), bufs):
                b.copy_(s0)
        loss_e, dic_e = train_step(model, LossFunction(), opt, ex, args)
        loss_g, dic_g = g()
        torch.cuda.synchronize()
        for k in ("sil_soft", "iou_soft"):                  # the forward of the new kernels has the same bits on every call
            assert torch.equal(dic_e[k].detach(), dic_g[k].detach()), (k, float(dic_e[k]), float(dic_g[k]))
        rel = abs(float(loss_e) - float(loss_g)) / max(1.0, abs(float(loss_e)))
        print(f"[soft_sil] graph vs eager: loss {float(loss_e):.6f} / {float(loss_g):.6f}, relative {rel:.2e} (bound {_GRAPH_LOSS_RTOL})")
        assert rel <= _GRAPH_LOSS_RTOL and bool(torch.isfinite(loss_g))
        g.release()
    finally:
        torch.cuda.set_stream(prev)


def _step_kernels(model, args, ex):
    """Counter of the kernels of one warmed eager step, read as test_gpu_e2e.test_training_step_runs_on_the_hand_written_kernels reads
    them.  The tracer drops a record now and then and never invents one: three steps are profiled and every kernel name counts as often as
    the step that showed it most."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import train_step
    opt = FusedAdam(FlatParams(model), lr=1e-6)
    for _ in range(3):
        train_step(model, LossFunction(), opt, ex, args)
    torch.cuda.synchronize()
    merged = Counter()
    for _ in range(3):
        try:                                                 # only the tracer may be missing: the step itself runs outside the try
            prof = profile(activities=[ProfilerActivity.CUDA])
            prof.__enter__()
        except Exception as e:                               # noqa: BLE001 -- as in test_gpu_e2e: the tracer is a measurement aid
            pytest.skip(f"torch.profiler / roctracer unavailable on this box: {type(e).__name__}: {e}")
        try:
            train_step(model, LossFunction(), opt, ex, args)
            torch.cuda.synchronize()
        finally:
            try:
                prof.__exit__(None, None, None)
                names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
            except Exception as e:                           # noqa: BLE001
                pytest.skip(f"torch.profiler / roctracer unavailable on this box: {type(e).__name__}: {e}")
        merged |= Counter(n for n in names if not (n.lower().startswith(("memcpy", "memset")) or "Memcpy" in n or "Memset" in n))
    if sum(merged.values()) < 50:
        pytest.skip(f"the tracer returned {sum(merged.values())} kernel records for a whole step: profiler unavailable on this box")
    return merged


def test_option_off_launches_what_it_launched_before(synth_tables):
    """What is asserted: a step with the option off launches NONE of the new kernels, and the step with the option and the two terms on adds
    exactly the seven new kernels in eight launches (forward: vertex pass, tiles, loss sums, finish; backward: loss, vertex pass, tiles,
    projection) plus a few of the runtime's and autograd's own (the fill of the NDC-gradient buffer, the sum of the two gradients of the
    vertices).  Model() and Model(soft_silhouette=False) are one code path: their equal counts are printed and compared only to show
    that the tracer's figures repeat; this tree cannot run the commit before it, so "as before" rests on the off path not containing a
    line of the new code (models.py: the two `if self.soft_silhouette` blocks; losses.py: the `sil_soft` / `iou_soft` block), on the
    unchanged bounds of test_gpu_e2e.test_training_step_runs_on_the_hand_written_kernels and on the benchmark's launch count."""
    import re
    from hifihr_amd import options
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        B = 4
        args = options.baseline_config2_args(train_batch=B)
        args_on = options.baseline_config2_args(train_batch=B, losses=args.losses + ["sil_soft", "iou_soft"])
        default, off, on = _model(synth_tables), _model(synth_tables, soft_silhouette=False), _model(synth_tables, soft_silhouette=True)
        ex = _batch(default, B, args, graded=True)
        k_default, k_off, k_on = _step_kernels(default, args, ex), _step_kernels(off, args, ex), _step_kernels(on, args_on, ex)
        soft = lambda ks: {re.search(r"soft_sil_\w+_kernel", n).group(0): c for n, c in ks.items() if "soft_sil" in n}
        n_default, n_off, n_on = (sum(k.values()) for k in (k_default, k_off, k_on))
        print(f"[soft_sil] kernel launches per step: default {n_default}, option off {n_off}, option on {n_on} (new: {soft(k_on)})")
        assert not soft(k_default) and not soft(k_off)
        assert k_default == k_off, (k_default - k_off, k_off - k_default)
        assert set(soft(k_on)) == sc.KERNELS and sum(soft(k_on).values()) == 8 and soft(k_on)["soft_sil_vertex_kernel"] == 2
        assert n_off + 8 <= n_on <= n_off + 14
    finally:
        torch.cuda.set_stream(prev)
