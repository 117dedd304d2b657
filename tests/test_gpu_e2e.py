"""GPU end-to-end parity: one training step of the HIP path (hifihr_amd.Model + LossFunction + FusedAdam) against
the CPU oracle step (oracle/model_oracle.py) from identical weights and inputs -- loss terms to 1e-4
(BASELINE.json north_star), rendered pixels to 1e-4, face indices bit-exact, parameter update to 1e-6."""
import numpy as np
import pytest
import torch

import kernel_cases as kc

pytestmark = pytest.mark.gpu


def graded_images(imgs):
    """Uniform-noise images differ from one another only in their noise, so the pooled features of the samples of a batch are
    nearly equal and the head's BatchNorm1d divides by a tiny across-sample variance: a 1e-7 rounding difference becomes 1e-4 of
    the loss.  Real photographs are not like that.  Give every sample its own brightness, contrast and a low-frequency ramp of
    its own orientation (still in [0, 1)), which conditions the batch statistics the way distinct photographs do."""
    B, _, H, W = imgs.shape
    i = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    gain = 0.25 + 0.6 * i / max(B - 1, 1)
    ang = 2.399963 * i                                                   # golden angle: orientations spread over the circle
    yy = torch.linspace(-1, 1, H).view(1, 1, H, 1); xx = torch.linspace(-1, 1, W).view(1, 1, 1, W)
    ramp = 0.5 + 0.5 * (torch.cos(ang) * xx + torch.sin(ang) * yy) / 1.4143
    tint = torch.stack([0.5 + 0.5 * torch.cos(ang.view(B) + c * 2.0944) for c in range(3)], 1).view(B, 3, 1, 1)
    out = gain * imgs.cpu() + (1 - gain) * ramp * tint
    return out.clamp_(0, 0.999999).to(imgs.device)


ORACLE_RATIO = {}                # what: the largest err / bound of the two oracle comparisons below (tests/switch_arm_child.py reports it)


def _setup(B, graded=False):
    from hifihr_amd import options, synth
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.traineval import data_dic
    from oracle.model_oracle import OracleModel
    tables = synthetic_mano_tables(0)
    args = options.baseline_config2_args(train_batch=B)
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = Model(True, dev, False, "mano", False, "res18", mano_tables=tables).to(dev).train()
    ref = OracleModel(tables).train()
    missing, unexpected = ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=False)
    assert not missing, missing
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, first_index=0, device=dev)
    if graded:
        sample["trans_images"] = graded_images(sample["trans_images"])
    ex = data_dic(sample, "FreiHand", "training", args, device=dev)
    ex_cpu = {k: v.cpu() for k, v in ex.items()}
    return tables, args, model, ref, ex, ex_cpu


def test_train_step_losses_match_oracle():
    """Whole step, encoder included: every loss term within 1e-4 of the CPU oracle (BASELINE.json north_star)."""
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import train_step
    from oracle.model_oracle import oracle_step
    B = 4          # BatchNorm1d over a batch of 2 is a sign function of tiny feature differences; 4 is well conditioned
    tables, args, model, ref, ex, ex_cpu = _setup(B)
    rloss, rdic, rout = oracle_step(ref, ex_cpu, args, None)
    flat = FlatParams(model)
    opt = FusedAdam(flat, lr=1e-4)
    before = flat.flat.clone()
    loss, dic = train_step(model, LossFunction(), opt, ex, args)
    torch.cuda.synchronize()
    report = {k: (float(dic[k].detach()), float(rdic[k].detach())) for k in args.losses}
    print("loss terms (hip, oracle):", report)
    ORACLE_RATIO["loss terms"] = max(abs(a - b) / (1e-4 * max(1.0, abs(b))) for a, b in report.values())
    for k, (a, b) in report.items():
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b, report)
    assert abs(float(loss) - float(rloss)) <= 1e-4 * max(1.0, abs(float(rloss)))
    moved = (flat.flat - before).abs()
    assert float(moved.max()) <= 1.01e-4 and float((moved > 0).float().mean()) > 0.5     # Adam's first step: |dp| <= lr


def test_backward_chain_matches_oracle_from_features():
    """Gradients of the HIP chain (losses -> renderer -> joints -> LBS -> regression heads) w.r.t. the encoder
    features and every head parameter vs the oracle's autograd, from IDENTICAL features (this isolates the
    hand-written kernels from MIOpen-vs-CPU conv rounding, which train-mode BatchNorm amplifies)."""
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.traineval import trans_proj_j2d
    from oracle.model_oracle import oracle_step
    B = 6
    tables, args, model, ref, ex, ex_cpu = _setup(B)
    with torch.no_grad():
        low, feat = model.base_encoder(ex["imgs"])
    low_g, feat_g = low.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    low_c, feat_c = low.cpu().clone().requires_grad_(True), feat.cpu().clone().requires_grad_(True)
    rloss, rdic, _ = oracle_step(ref, ex_cpu, args, None, features=(low_c, feat_c))
    rloss.backward()
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    out = model.forward_from_features("FreiHand", True, ex["imgs"], low_g, feat_g, Ks=ex["Ps"], root_xyz=root)
    e2 = dict(ex); e2["joints"] = ex["joints"] - root; e2["verts"] = ex["verts"] - root
    out["j2d"] = trans_proj_j2d(out, ex["Ks"], root_xyz=root)
    dic = LossFunction()(e2, out, args.losses, "FreiHand", args)
    loss = sum(dic[k] for k in args.losses)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(rloss)) <= 1e-4 * max(1.0, abs(float(rloss)))
    pairs = [("d/d feat", feat_g.grad, feat_c.grad), ("d/d low", low_g.grad, low_c.grad)]
    rgrads = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        if name.startswith("base_encoder"):
            continue
        if name in ("hand_encoder.base_layers.0.bias", "hand_encoder.base_layers.3.bias"):
            continue        # a bias in front of BatchNorm: the true gradient is exactly 0, both sides hold rounding noise
        rg = rgrads[name].grad
        if rg is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        pairs.append((name, p.grad, rg))
    gmax = max(float(r.abs().max()) for _, _, r in pairs)
    errs = []
    for name, g, r in pairs:
        scale = max(float(r.abs().max()), 1e-4 * gmax)        # pre-BatchNorm biases have an exactly-zero true gradient
        errs.append((float((g.detach().cpu() - r).abs().max()) / scale, name))
    print("worst relative gradient errors:", sorted(errs, reverse=True)[:6])
    ORACLE_RATIO["chain gradients"] = max(errs)[0] / 5e-3
    assert max(errs)[0] < 5e-3, sorted(errs, reverse=True)[:6]


def test_forward_outputs_match_oracle():
    B = 2
    tables, args, model, ref, ex, ex_cpu = _setup(B)
    model.eval(); ref.eval()                       # BN running stats: deterministic comparison of the whole chain
    root = ex["joints"][:, 9, :].unsqueeze(1)
    with torch.no_grad():
        out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
        rout = ref("FreiHand", True, ex_cpu["imgs"], Ks=ex_cpu["Ps"], root_xyz=root.cpu())
    np.testing.assert_allclose(out["joints"].cpu().numpy(), rout["joints"].numpy(), atol=1e-5)
    np.testing.assert_allclose(out["mano_verts"].cpu().numpy(), rout["mano_verts"].numpy(), atol=1e-5)
    fid, rfid = out["face_id"].cpu().numpy(), rout["face_id"].numpy()
    # the encoders run on different back-ends (MIOpen vs CPU ATen), so vertices differ by ~1e-6 and a handful of
    # samples on triangle edges may flip; everything else must be identical
    assert (fid != rfid).mean() < 2e-4
    diff = (out["re_img"].cpu() - rout["re_img"]).abs()
    assert float(diff.mean()) < 1e-4 and float((diff > 1e-3).float().mean()) < 2e-3
    assert float((out["re_sil"].cpu() != rout["re_sil"]).float().mean()) < 2e-3


def test_adam_kernel_vs_torch():
    from hifihr_amd._lib import get_lib
    kc.adam_case(get_lib(), "cuda", n=12_600_003, wd=0.0, steps=3)
    kc.adam_case(get_lib(), "cuda", n=1003, wd=0.01, steps=3)


def test_ssim_kernel_full_size(golden_dir):
    """Fused SSIM at the BASELINE size (32x3x224x224) vs the torch restatement, and vs the reference's own scalar for
    the seeded 2x3x224x224 pair of tests/golden/ssim.npz."""
    import os
    from hifihr_amd import ops
    from hifihr_amd._lib import get_lib
    from oracle.loss_oracle import ssim as ssim_torch
    g = np.load(os.path.join(golden_dir, "ssim.npz"))
    kc.ssim_case(get_lib(), "cuda", g["a"], g["b"], g["ssim"], g["ga"])
    gen = torch.Generator().manual_seed(12)
    A = torch.rand(2, 3, 224, 224, generator=gen); B = torch.rand(2, 3, 224, 224, generator=gen)
    assert abs(float(ops.ssim(A.cuda(), B.cuda())) - float(g["ssim224"])) < 2e-6
    gen = torch.Generator().manual_seed(3)
    a = torch.rand(32, 3, 224, 224, generator=gen)
    b = (a * (torch.rand(32, 1, 224, 224, generator=gen) > 0.7)).contiguous()
    ac = a.cuda().requires_grad_(True)
    v = ops.ssim(ac, b.cuda())
    v.backward()
    ar = a.cuda().requires_grad_(True)
    vr = ssim_torch(ar, b.cuda())
    vr.backward()
    assert abs(float(v) - float(vr)) < 5e-6
    assert float((ac.grad - ar.grad).abs().max()) <= 5e-4 * float(ar.grad.abs().max())


# Bounds of the graph-vs-eager tests, against what tools/noise_floor.py MEASURES between two EAGER replicas that start from identical
# weights (gpurun_out/noise_*.txt, round 5; float-atomic ordering in backward, which Adam turns into +-lr steps of the weights whose
# gradient is rounding noise):
#   uniform-noise images, B = 8:  loss spread 1.6e-5 / 2.6e-4 / 5.4e-4 after 1 / 2 / 3 steps -- the old 2e-4 bound sat INSIDE the noise
#   graded images (graded_images), B = 8:  5.9e-6 / 6.7e-6 / 9.2e-6;  graph vs eager 1.9e-6 / 5.5e-6 / 4.2e-6 / 1.1e-5
# so the tests run on graded images and assert 2e-4: >= 18 x the worst graph-vs-eager value observed.  Every comparison prints
# observed / bound.
_GRAPH_LOSS_RTOL = 2e-4


def _check(tag, observed, bound):
    print(f"[margin] {tag}: observed {observed:.3e}  bound {bound:.3e}  observed/bound {observed / bound:.3f}")
    assert observed <= bound, (tag, observed, bound)


def _weights_agree(flat, flat2, lr, steps):
    # Adam moves a weight by at most ~lr per step whatever its gradient: replicas whose rounding-noise gradients have opposite signs
    # part by <= 2 lr per step (observed: 3.2e-6 ... 6.1e-6 after 4 steps at lr 1e-6 -- by construction AT that limit, so the max is
    # asserted at three times the limit and only catches gross corruption); the MEAN is the sensitive quantity: observed 1.2e-9 ... 1.6e-8
    d = (flat.flat - flat2.flat).abs()
    _check("max |w_eager - w_graph|", float(d.max()), 6 * lr * steps)
    _check("mean |w_eager - w_graph|", float(d.mean()), 0.15 * lr)


def _warm_eager(model, opt, ex, args):
    """The FIRST eager step of a model runs before the per-step weight re-layout has its Winograd-domain filters, i.e. on other kernels
    than every later step (tools/determinism_probe.py).  One forward + backward without an optimizer step, batch-norm buffers put back:
    from here on the eager step dispatches exactly what a captured step replays."""
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.traineval import forward_backward
    bufs = [b.clone() for b in model.buffers()]
    forward_backward(model, LossFunction(), opt, ex, args)
    with torch.no_grad():
        for b, s0 in zip(model.buffers(), bufs):
            b.copy_(s0)
    torch.cuda.synchronize()


def _sync_state(dst, src):
    """(model, flat, opt) <- (model, flat, opt): weights, Adam moments, step counter, every module buffer."""
    (dm, df, do), (sm, sf, so) = dst, src
    with torch.no_grad():
        df.flat.copy_(sf.flat); do.exp_avg.copy_(so.exp_avg); do.exp_avg_sq.copy_(so.exp_avg_sq)
        for b, s0 in zip(dm.buffers(), sm.buffers()):
            b.copy_(s0)
    do.step_count = so.step_count
    torch.cuda.synchronize()


def _assert_same_bits(tag, dic_a, dic_b, terms):
    """The FORWARD of the step is bit-reproducible (no float atomics on it that survive rounding: the batch-norm statistics are fp64
    sums): from identical weights and the same batch a replayed graph and the eager step must produce identical loss terms."""
    bad = [k for k in terms if not torch.equal(dic_a[k].detach(), dic_b[k].detach())]
    print(f"[exact] {tag}: {len(terms) - len(bad)} of {len(terms)} loss terms bit-identical" + (f"; differing: {bad}" if bad else ""))
    assert not bad, (tag, {k: (float(dic_a[k]), float(dic_b[k])) for k in bad})


def test_graphed_step_matches_eager_step():
    """The hipGraph-replayed training step performs the same update as the eager step (same weights, same batch)."""
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, train_step
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        B, lr = 8, 1e-6                                    # tiny lr: isolates the graph mechanics from Adam's sign noise
        tables, args, model, ref, ex, ex_cpu = _setup(B, graded=True)
        model2 = Model(True, torch.device("cuda"), False, "mano", False, "res18", mano_tables=tables).cuda().train()
        model2.load_state_dict(model.state_dict())
        flat = FlatParams(model); opt = FusedAdam(flat, lr=lr)
        flat2 = FlatParams(model2); opt2 = FusedAdam(flat2, lr=lr)
        before = flat2.flat.clone()
        rm_before = model2.base_encoder.encoder1.model.bn1.running_mean.clone()
        g = GraphedTrainStep(model2, LossFunction(), opt2, ex, args, warmup=3)
        torch.cuda.synchronize()
        # warm-up + capture are free of side effects: weights, Adam state, step counter, batch-norm running statistics
        assert torch.equal(flat2.flat, before) and opt2.step_count == 0 and float(opt2.exp_avg.abs().max()) == 0.0
        assert torch.equal(model2.base_encoder.encoder1.model.bn1.running_mean, rm_before)
        _warm_eager(model, opt, ex, args)
        for step in range(2):
            loss_e, dic_e = train_step(model, LossFunction(), opt, ex, args)
            loss_g, dic_g = g()
            torch.cuda.synchronize()
            if step == 0:          # identical weights: the forward must agree bit for bit (later steps start from weights that differ by backward's atomic noise)
                _assert_same_bits("step 0, graph vs eager", dic_e, dic_g, list(args.losses) + ["loss"])
            _check(f"step {step} |loss_eager - loss_graph| / loss", abs(float(loss_e) - float(loss_g)) / max(1.0, abs(float(loss_e))), _GRAPH_LOSS_RTOL)
        _weights_agree(flat, flat2, lr, 2)
        assert opt2.step_count == 2 and opt.step_count == 2
    finally:
        torch.cuda.set_stream(prev)


def test_light_branch_is_joined_after_backward_with_a_detached_trunk():
    """ops.side_branch (the light estimator beside the hand-encoder / MANO chain) with a trunk whose features do NOT require grad
    (heads-only fine-tuning): the branch's convolutions write their weight gradients straight into the flat gradient buffer on the
    side stream and no input gradient carries the join back to the main stream -- prepared_weights.__exit__ must join the branch
    explicitly (ops.side_branch.join_pending), eager AND captured (an un-joined stream fails the capture).  Light-estimator
    gradients with the branch equal those of the single-stream step; the captured step replays and moves the light estimator."""
    from hifihr_amd import ops
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, forward_backward
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        tables, args, model, ref, ex, ex_cpu = _setup(4, graded=True)
        enc = model.encode
        model.encode = lambda images: tuple(t.detach() for t in enc(images))      # low_features / features carry no gradient
        flat = FlatParams(model); opt = FusedAdam(flat, lr=1e-4)
        light = [p for p in model.light_estimator.parameters()]
        _warm_eager(model, opt, ex, args)

        def light_grads(branches):
            old = ops._BRANCHES
            ops._BRANCHES = branches
            try:
                forward_backward(model, LossFunction(), opt, ex, args)
                # what Adam would read, on the step's own stream, with no device-wide synchronisation in between
                g = torch.cat([p.grad.reshape(-1).clone() for p in light])
            finally:
                ops._BRANCHES = old
            torch.cuda.synchronize()
            return g
        assert ops._BRANCHES, "the branch is on by default"
        g_off = light_grads(False)
        for rep in range(3):
            g_on = light_grads(True)
            assert not ops.side_branch._pending, "prepared_weights.__exit__ left a branch un-joined"
            _check(f"rep {rep} |g_light(branch) - g_light(inline)| / max|g|", float((g_on - g_off).abs().max()) / float(g_off.abs().max()), 1e-4)
        assert float(g_off.abs().max()) > 0
        trunk_g = [p.grad for p in model.base_encoder.parameters() if p.grad is not None]
        assert all(float(t.abs().max()) == 0.0 for t in trunk_g)                    # the detached trunk received nothing
        # captured: the constructor raises if the capture ends with an un-joined side stream
        w0 = torch.cat([p.detach().reshape(-1).clone() for p in light])
        step = GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=2)
        for _ in range(2):
            loss, dic = step()
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        w1 = torch.cat([p.detach().reshape(-1) for p in light])
        assert float((w1 - w0).abs().max()) > 0, "the replayed step did not update the light estimator"
        step.release()
    finally:
        torch.cuda.set_stream(prev)


def test_training_step_runs_on_the_hand_written_kernels():
    """What the device executes during one (warmed, eager) training step of BASELINE configs[1] at its batch: kernels of libhifihr.so --
    no Tensile / rocBLAS / hipBLASLt / MIOpen kernel (a silent library fallback would pass every parity test), at most a handful of ATen
    elementwise kernels (autograd's own accumulation, the gradient buffer's fill), and a launch count in the range the profiles report
    (profiles/r05_steady_state_res18.md: 200 in the replayed graph)."""
    from torch.profiler import ProfilerActivity, profile
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import train_step
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        B = 32
        tables, args, model, ref, ex, ex_cpu = _setup(B, graded=True)
        flat = FlatParams(model); opt = FusedAdam(flat, lr=1e-6)
        for _ in range(3):
            train_step(model, LossFunction(), opt, ex, args)
        torch.cuda.synchronize()
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                train_step(model, LossFunction(), opt, ex, args)
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        except Exception as e:                               # noqa: BLE001 -- the tracer is a measurement aid: its absence is not a failure of the step
            pytest.skip(f"torch.profiler / roctracer unavailable on this box: {type(e).__name__}: {e}")
        kernels = [n for n in names if not (n.lower().startswith(("memcpy", "memset")) or "Memcpy" in n or "Memset" in n)]
        if len(kernels) < 50:
            pytest.skip(f"the tracer returned {len(kernels)} kernel records for a whole step: profiler unavailable on this box")
        library = [n for n in kernels if n.startswith("Cijk_") or "miopen" in n.lower() or "rocblas" in n.lower() or "hipblaslt" in n.lower()
                   or "ck::" in n or "tensile" in n.lower()]
        assert not library, sorted(set(library))
        ours = [n for n in kernels if "hifihr::" in n]
        aten = [n for n in kernels if n.startswith(("void at::native", "at::native"))]
        other = sorted(set(n for n in kernels if n not in ours and n not in aten and "rocclr" not in n))
        print(f"[step] {len(kernels)} kernel launches: {len(ours)} hifihr, {len(aten)} ATen {sorted(set(a[:70] for a in aten))}, other {other}")
        assert not other, other
        # (this batch comes from data_dic, not from the batch kernel that emits the step's own terms: index_select / sub for root_xyz and
        # the root-relative ground truth are ATen here.  roctracer drops a share of the records: no lower bound beyond "a whole step")
        assert len(aten) <= 12, sorted(set(aten))            # 7 observed
        assert 100 <= len(kernels) <= 260, len(kernels)
    finally:
        torch.cuda.set_stream(prev)


def test_graph_replay_survives_an_evaluation_pass_in_between():
    """train (graph) -> evaluate (model.eval(), a LARGER batch) -> train (graph) == the same sequence on the eager step.
    An evaluation forward must not disturb what the captured graph holds: it requests no batch-norm statistics buffer (round 1
    leaked a dirty one into the pool whose address the graph had baked in) and scratch that grows keeps the old tensor alive.
    A SECOND eager replica walks the same sequence: its distance from the first is the noise floor of this very run, printed next to
    every graph-vs-eager distance (the assertion itself is the absolute bound above, >= 18 x the floor measured on graded images)."""
    from hifihr_amd import synth
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, data_dic, train_step
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        B, lr = 8, 1e-6
        tables, args, model, ref, ex, ex_cpu = _setup(B, graded=True)
        dev = torch.device("cuda")

        def replica():
            m = Model(True, dev, False, "mano", False, "res18", mano_tables=tables).cuda().train()
            m.load_state_dict(model.state_dict())
            f = FlatParams(m)
            return m, f, FusedAdam(f, lr=lr)
        model2, flat2, opt2 = replica()                    # the graphed one
        model3, flat3, opt3 = replica()                    # eager, like `model`: the noise floor
        big = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, 2 * B, first_index=100, device=dev)
        big["trans_images"] = graded_images(big["trans_images"])
        big = data_dic(big, "FreiHand", "training", args, device=dev)
        flat = FlatParams(model); opt = FusedAdam(flat, lr=lr)
        g = GraphedTrainStep(model2, LossFunction(), opt2, ex, args)

        def evaluate(m):
            m.eval()
            with torch.no_grad():
                root = big["joints"][:, args.ROOT, :].unsqueeze(1)
                out = m("FreiHand", False, big["imgs"], Ks=big["Ps"], root_xyz=root)
            m.train()
            return out["joints"]

        _warm_eager(model, opt, ex, args)
        _warm_eager(model3, opt3, ex, args)

        def step(tag, exact=False):
            loss_e, dic_e = train_step(model, LossFunction(), opt, ex, args)
            loss_f, _ = train_step(model3, LossFunction(), opt3, ex, args)
            loss_g, dic_g = g()
            torch.cuda.synchronize()
            if exact:
                _assert_same_bits(f"{tag}, graph vs eager from identical state", dic_e, dic_g, list(args.losses) + ["loss"])
            ref_ = max(1.0, abs(float(loss_e)))
            print(f"[floor] {tag}: eager-vs-eager {abs(float(loss_e) - float(loss_f)) / ref_:.3e}")
            _check(f"{tag} |loss_eager - loss_graph| / loss", abs(float(loss_e) - float(loss_g)) / ref_, _GRAPH_LOSS_RTOL)
        for rnd in range(2):
            step(f"round {rnd}", exact=(rnd == 0))
            je, jf, jg = evaluate(model), evaluate(model3), evaluate(model2)
            print(f"[floor] round {rnd} evaluation joints: eager-vs-eager {float((je - jf).abs().max()):.3e}")
            _check(f"round {rnd} evaluation joints max diff", float((je - jg).abs().max()), 1e-4)
        step("after the evaluations")
        _weights_agree(flat, flat2, lr, 3)
        # ... and the BIT-EXACT form of the same statement: put the graphed replica into the eager one's state (weights, Adam moments, step
        # counter, batch-norm buffers) behind ANOTHER evaluation pass of both, then step both -- the replayed forward must reproduce the eager
        # one bit for bit.  A dirty statistics buffer or a stale scratch address baked into the graph shows up here with no tolerance to hide in.
        evaluate(model); evaluate(model2)
        _sync_state((model2, flat2, opt2), (model, flat, opt))
        step("after an evaluation pass", exact=True)
    finally:
        torch.cuda.set_stream(prev)


@pytest.mark.parametrize("config,B,image_size,aa", [(3, 4, 224, 3), (5, 4, 224, 3), (3, 48, 224, 3), (5, 16, 512, 1), (5, 16, 512, 3)])
def test_nimble_config_compositions_match_oracle_from_features(config, B, image_size, aa):
    """BASELINE configs[2] / configs[4] as they run here (EfficientNet-b3, MANO + the vertex-colour texture stand-in for the
    unavailable NIMBLE layer, VGG19 perceptual loss with seeded weights; configs[4] in the HO-3D conventions): every loss
    term of the reference's JSON loss list within 1e-4 of the CPU oracle and the gradients w.r.t. the encoder features,
    from identical features (the encoder itself is pinned by test_gpu_conv / the golden EfficientNet vectors)."""
    from hifihr_amd import options, synth
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.traineval import data_dic, trans_proj_j2d
    from oracle.model_oracle import OracleModel, oracle_step
    # (3, 48, 224, 3) = BASELINE configs[2] at its real batch; (5, 16, 512, *) = configs[4] per GPU at its 512^2 render resolution
    dat = "FreiHand" if config == 3 else "HO3D"
    args = options.baseline_config3_args(train_batch=B) if config == 3 else options.baseline_config5_args(train_batch=B)
    tables = synthetic_mano_tables(0)
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = Model(True, dev, False, "mano", False, "effb3", mano_tables=tables, texture_stand_in=10, image_size=image_size,
                  aa_factor=aa).to(dev).train()
    ref = OracleModel(tables, pretrain="effb3", texture_stand_in=10, image_size=image_size, aa=aa).train()
    missing, _ = ref.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, strict=False)
    assert not missing, missing
    sample = synth.make_batch(model.hand_layer.handle, model.renderer_p3d, B, first_index=40, device=dev, image_size=image_size)
    if dat == "HO3D":
        sample = synth.to_ho3d_sample(sample, crop=2 * image_size if image_size == 224 else image_size)
    ex = data_dic(sample, dat, "training", args, device=dev, image_size=image_size)
    ex_cpu = {k: v.cpu() for k, v in ex.items()}
    with torch.no_grad():
        low, feat = model.encode(ex["imgs"])
    low_g, feat_g = low.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    low_c, feat_c = low.cpu().clone().requires_grad_(True), feat.cpu().clone().requires_grad_(True)
    rloss, rdic, _ = oracle_step(ref, ex_cpu, args, None, features=(low_c, feat_c), dat_name=dat)
    rloss.backward()
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    out = model.forward_from_features(dat, True, ex["imgs"], low_g, feat_g, Ks=ex["Ps"], root_xyz=root)
    e2 = dict(ex)
    if dat != "HO3D":
        e2["joints"] = ex["joints"] - root; e2["verts"] = ex["verts"] - root
    out["j2d"] = trans_proj_j2d(out, ex["Ks"], root_xyz=root)
    dic = LossFunction()(e2, out, args.losses, dat, args)
    loss = sum(dic[k] for k in args.losses)
    loss.backward()
    torch.cuda.synchronize()
    report = {k: (float(dic[k].detach()), float(rdic[k].detach())) for k in args.losses}
    print("loss terms (hip, oracle):", report)
    for k, (a, b) in report.items():
        assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b, report)
    # the perceptual term carries lambda = 1e-8: also compare it unscaled
    pa, pb = report["perceptual"][0] / args.lambda_percep, report["perceptual"][1] / args.lambda_percep
    assert abs(pa - pb) <= 1e-4 * max(1.0, abs(pb)), (pa, pb)
    for name, g, r in (("d/d feat", feat_g.grad, feat_c.grad), ("d/d low", low_g.grad, low_c.grad)):
        err = float((g.cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-12)
        assert err < 5e-3, (name, err)


def test_overfitting_one_batch_reduces_every_supervised_term():
    """System-level check of the gradients and the fused Adam: 80 steps on ONE fixed batch (graph replay) must drive the
    3-D supervision terms down by a large factor -- the encoder can memorise 8 images even though they are noise."""
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep
    B = 8
    tables, args, model, ref, ex, ex_cpu = _setup(B)
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        flat = FlatParams(model)
        opt = FusedAdam(flat, lr=1e-3)
        step = GraphedTrainStep(model, LossFunction(), opt, ex, args)
        loss0, dic0 = step()
        first = {k: float(dic0[k]) for k in ("joint_3d", "vert_3d")}
        for _ in range(80):
            loss, dic = step()
        last = {k: float(dic[k]) for k in ("joint_3d", "vert_3d")}
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(prev)
    print("overfit:", first, "->", last)
    assert all(torch.isfinite(torch.tensor(v)) for v in last.values())
    for k in first:
        assert last[k] < 0.5 * first[k], (k, first[k], last[k])


def test_deferred_weight_gradient_transforms_equal_the_immediate_ones():
    """ops._DeferredDw (the F(4x4) weight-gradient transforms and the 64 -> 64 slab sums of a step as one launch each in front of the optimizer)
    against HIFIHR_DEFER_DW=0's per-layer launches: the same flat gradient, bit for bit on the deferred layers (same slabs, same per-item
    arithmetic), after one backward AND after a second backward inside the same scope (gradient accumulation: the second pass must not
    disturb the slabs the first one left for the flush)."""
    from hifihr_amd import ops
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import _forward_backward
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        tables, args, model, ref, ex, ex_cpu = _setup(4, graded=True)
        flat = FlatParams(model); opt = FusedAdam(flat, lr=1e-4)
        _warm_eager(model, opt, ex, args)
        bufs = [b.clone() for b in model.buffers()]
        wts = [(n, p) for n, p in model.named_parameters() if p.dim() == 4 and p.shape[2] == 3 and p.shape[0] >= 64]

        def grads(defer, twice, early=True):
            with torch.no_grad():
                for b, s0 in zip(model.buffers(), bufs):
                    b.copy_(s0)
            old, old_early = ops._DEFER_DW.on, ops._DEFER_DW.early
            ops._DEFER_DW.on, ops._DEFER_DW.early = defer, early
            try:
                with ops.prepared_weights(async_wgrad=False):
                    _forward_backward(model, LossFunction(), opt, ex, args, "FreiHand")
                    if twice:                        # a second forward + backward in the SAME scope, accumulating (no zero_grad in between)
                        zg = opt.zero_grad
                        opt.zero_grad = lambda set_to_none=False: None
                        try:
                            _forward_backward(model, LossFunction(), opt, ex, args, "FreiHand")
                        finally:
                            opt.zero_grad = zg
            finally:
                ops._DEFER_DW.on, ops._DEFER_DW.early = old, old_early
            torch.cuda.synchronize()
            return {n: p.grad.clone() for n, p in wts}
        for twice in (False, True):
            # early: the launch forks to a side stream where the backward reaches the stem's pooling (ops._DeferredDw.flush_early) and is
            # joined in front of the optimizer; not early: one launch at the scope's exit
            n0 = ops._DEFER_DW.n_early
            g_early = grads(True, twice, early=True)
            assert ops._DEFER_DW.n_early > n0, "the early flush never ran: the ResNet stem's pooling backward should trigger it"
            n1 = ops._DEFER_DW.n_early
            g_late, g_imm = grads(True, twice, early=False), grads(False, twice)
            assert ops._DEFER_DW.n_early == n1
            worst = 0.0
            for n in g_imm:
                scale = float(g_imm[n].abs().max())
                for g_def in (g_early, g_late):
                    d = float((g_def[n] - g_imm[n]).abs().max())
                    # the products' float atomics elsewhere in backward reorder between two runs: the transforms themselves add nothing
                    assert d <= 2e-4 * scale + 1e-9, (n, twice, d, scale)
                    worst = max(worst, d / max(scale, 1e-30))
            print(f"[margin] deferred (early and late flush) vs immediate weight gradients, second backward in scope = {twice}: worst |diff| / max|g| = {worst:.2e} (bound 2e-4)")
    finally:
        torch.cuda.set_stream(prev)


def test_bench_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR`: the plain run prints the headline line alone (what `--full` adds is
    absent), with `steps` == 2 and a positive `ms_per_step`; DIR holds the last timed step's loss, loss terms and parameters as finite
    float32 arrays, and its loss is the one the line reports."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
                        "--cache", "64", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:]); print(r.stderr[-3000:])
    assert r.returncode == 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "images/sec" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True
    assert not any(k in d for k in ("cpu_baseline", "roofline", "roofline_kernels", "resident_batch"))
    files = sorted(os.listdir(out))
    assert "loss.npy" in files and "params.npy" in files and any(f.startswith("loss_") for f in files)
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    for f in files:
        a = np.load(out / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    assert float(np.load(out / "loss.npy")) == np.float32(d["loss"])
