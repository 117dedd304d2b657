"""The depth map and the depth loss on the MI355X: hifihr_render_depth_fwd / _bwd and hifihr_depth_loss_fwd / _bwd through the C ABI on the
cases of tests/test_hostsim_depth.py (tests/depth_cases.py; references: oracle/raster_oracle.c and the restatements of tests/depth_ref.py),
one captured graph of all four entries, and the Python surface end to end: ops.render_depth / ops.depth_loss, Model(render_depth=True),
the loss term "depth", synth.make_batch(depth=True), Evaluator(depth=True).  B <= 2 and image_size <= 32 throughout."""
import numpy as np
import pytest
import torch

import depth_cases as dc
import depth_ref as dr

pytestmark = pytest.mark.gpu
_ids = lambda g: "-".join(str(v) for v in g)
NEW_PROFILE_NAMES = {"render_depth_fwd", "render_depth_bwd", "depth_loss_fwd", "depth_loss_bwd"}


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


def test_known_answers(lib):
    dc.known_answers_case(lib, "cuda")


@pytest.mark.parametrize("kind", dc.KINDS)
def test_depth_has_the_bits_of_the_rasteriser(lib, kind):
    dc.bit_equality_case(lib, "cuda", kind)


def test_mano_topology_has_the_bits_of_the_rasteriser(lib, synth_tables):
    dc.mano_bits_case(lib, "cuda", synth_tables)


@pytest.mark.parametrize("case", dc.GRAD_CASES, ids=_ids)
def test_gradient_matches_float64_autograd(lib, case):
    dc.gradient_case(lib, "cuda", *case)


def test_gradient_is_finite_on_the_denominator_clamp(lib):
    dc.clamp_case(lib, "cuda")


@pytest.mark.parametrize("shape", dc.LOSS_SHAPES, ids=_ids)
def test_loss_pair_matches_the_ordered_float64_restatement(lib, shape):
    dc.loss_case(lib, "cuda", *shape)


def test_loss_without_a_valid_pixel_and_single_pixel(lib):
    dc.loss_edge_cases(lib, "cuda")


def test_refusals_leave_the_outputs_untouched(lib):
    dc.refusal_case(lib, "cuda")


def test_captured_graph_replays_the_eager_bits(lib):
    """The forward, the loss and both backwards captured in ONE graph (a chain, no parallel branch): depth, hits, sums, out and gdepth
    replay to the eager bits; gverts (float atomics) is held to the gradient bound of the kernel cases against float64 autograd."""
    H, aa, B, F, seed = dc.GRAD_CASES[3]
    verts, faces, cam, _ = dc.grad_inputs(H, aa, B, F, seed)
    V, lam, trunc = verts.shape[1], 0.8, 0.0
    dev = torch.device("cuda")
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        with dc.Renderer(lib, faces, V, H, aa) as r:
            v, c = verts.to(dev), cam.to(dev)
            fid = dc.kernel_face_id(lib, dev, r, verts, cam)
            target = torch.full((B, H, H), 0.6, device=dev)
            gout = torch.tensor([1.7], device=dev)
            ws = torch.empty(lib.render_depth_workspace_bytes(r.h, B), dtype=torch.uint8, device=dev)

            def buffers():
                return dict(depth=torch.full((B, 1, H, H), float("nan"), device=dev), hits=torch.full((B, H, H), -5, dtype=torch.int32, device=dev),
                            sums=torch.full((B, 2), -3e300, dtype=torch.float64, device=dev), out=torch.full((1,), float("nan"), device=dev),
                            gdepth=torch.full((B, 1, H, H), float("nan"), device=dev), gverts=torch.full((B, V, 3), float("nan"), device=dev))

            def chain(o):
                lib.render_depth_fwd(r.h, v, c, fid, o["depth"], o["hits"])
                lib.depth_loss_fwd(o["depth"], o["hits"], target, None, lam, trunc, o["sums"], o["out"])
                lib.depth_loss_bwd(o["depth"], o["hits"], target, None, o["sums"], gout, lam, trunc, o["gdepth"])
                lib.render_depth_bwd(r.h, v, c, fid, o["gdepth"], o["hits"], o["gverts"], ws)

            eager = buffers()
            chain(eager)
            torch.cuda.synchronize()
            cap = buffers()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=torch.cuda.current_stream()):
                chain(cap)
            for t in cap.values():                         # the capture itself ran nothing: poison again, then replay
                t.fill_(-7)
            graph.replay()
            torch.cuda.synchronize()
            for k in ("depth", "hits", "sums", "out", "gdepth"):
                assert torch.equal(eager[k].view(torch.uint8), cap[k].view(torch.uint8)), f"{k}: the replay differs from the eager bits"
            assert float(eager["out"]) > 0 and int((eager["hits"] > 0).sum()) > 0
            # gverts of both against float64 autograd of the same chain
            vr = verts.double().requires_grad_(True)
            d = dr.depth_torch(vr, cam, faces, fid.cpu(), eager["hits"].cpu(), H, aa)
            d.backward(eager["gdepth"].cpu().double().reshape(B, H, H))
            ref, scale = vr.grad, float(vr.grad.abs().max())
            v32 = verts.clone().requires_grad_(True)
            dr.depth_torch(v32, cam, faces, fid.cpu(), eager["hits"].cpu(), H, aa, dtype=torch.float32).backward(eager["gdepth"].cpu().reshape(B, H, H))
            bound = dc.GRAD_FACTOR * float((v32.grad.double() - ref).abs().max()) / scale
            for tag, got in (("eager", eager["gverts"]), ("replay", cap["gverts"])):
                err = float((got.cpu().double() - ref).abs().max()) / scale
                print(f"[depth] captured chain, gverts {tag}: {err:.3e} (bound {bound:.3e})")
                assert err <= bound
            del graph
    finally:
        torch.cuda.set_stream(prev)


# ---- Python surface -----------------------------------------------------------------------------------------------------------------
H_MODEL, AA_MODEL, B_MODEL = 32, 3, 2


def _model(tables, **kw):
    from hifihr_amd.models import Model
    torch.manual_seed(0)
    return Model(True, torch.device("cuda"), False, "mano", False, "res18", mano_tables=tables, image_size=H_MODEL, aa_factor=AA_MODEL, **kw).cuda().train()


@pytest.fixture(scope="module")
def scene(synth_tables):
    """One synthetic batch with depths at image_size 32, its examples, and the camera make_batch drew it with (the same expressions on the
    same device: the same bits)."""
    from hifihr_amd import ops, options, synth
    from hifihr_amd.traineval import data_dic
    dev = torch.device("cuda")
    mano = ops.ManoLayerHandle(synth_tables)
    rend = ops.RendererHandle(synth_tables.faces, 778, image_size=H_MODEL, aa=AA_MODEL)
    sample = synth.make_batch(mano, rend, B_MODEL, first_index=3, device=dev, image_size=H_MODEL, depth=True)
    plain = synth.make_batch(mano, rend, B_MODEL, first_index=3, device=dev, image_size=H_MODEL)
    args = options.baseline_config2_args(train_batch=B_MODEL)
    ex = data_dic(sample, "FreiHand", "training", args, device=dev, image_size=H_MODEL)
    Kp, s = sample["trans_Ks"].to(dev), float(H_MODEL)
    cam = torch.stack([-(Kp[:, 0, 0] * 2 / s), -(Kp[:, 1, 1] * 2 / s), -(Kp[:, 0, 2] - s / 2) * 2 / s, -(Kp[:, 1, 2] - s / 2) * 2 / s], dim=-1).contiguous()
    return dict(sample=sample, plain=plain, ex=ex, cam=cam, rend=rend, args=args, verts=sample["trans_verts"].to(dev).contiguous())


def _render(rend, verts, cam):
    from hifihr_amd import ops
    B, dev = verts.shape[0], verts.device
    _, fid = ops.render(rend, verts, torch.ones(778, 3, device=dev), cam, torch.zeros(B, 3, device=dev),
                        torch.tensor([0.0, 0.0, -1.0], device=dev).repeat(B, 1))
    return fid


def test_synthetic_batch_carries_depths_and_is_otherwise_unchanged(scene):
    from hifihr_amd import synth
    sample, plain = scene["sample"], scene["plain"]
    assert set(sample) == set(plain) | {"depths"}
    for k in plain:
        assert torch.equal(sample[k], plain[k]), k
    d = sample["depths"]
    assert tuple(d.shape) == (B_MODEL, H_MODEL, H_MODEL) and d.dtype == torch.float32
    covered = sample["trans_masks"][:, 0] > 0
    assert int(covered.sum()) > 20 and bool((d[covered] > 0.3).all()) and bool((d[covered] < 1.0).all()) and not bool(d[~covered].any())
    assert torch.equal(scene["ex"]["depths"].cpu(), d)
    assert torch.equal(synth.mesh_depths(scene["rend"], scene["verts"], scene["cam"]).cpu(), d)


def test_term_is_zero_on_the_same_pose_and_follows_a_shift_in_z(scene, synth_tables):
    """`depth` against the synthetic depths of the same pose is exactly 0.  Against a pose shifted along Z by delta it is lambda_depth * delta
    to fp32 rounding on fully covered pixels -- pz of a translated mesh is not exactly pz + delta at a fixed sample, so the comparison is with
    the restatement of both maps, and the closed form is only printed.  One descent step along the negative gradient reduces it, and
    Evaluator(depth=True) reports the term at lambda = 1."""
    from hifihr_amd import evaluate, ops, options
    from hifihr_amd.losses import LossFunction
    rend, cam, verts, ex = scene["rend"], scene["cam"], scene["verts"], scene["ex"]
    lam, delta = 2.5, 0.0125
    args = options.baseline_config2_args(train_batch=B_MODEL, losses=["depth"], lambda_depth=lam)

    def term(v, examples=ex, a=args):
        depth, hits = ops.render_depth(rend, v, cam, _render(rend, v, cam))
        dic = LossFunction()(examples, {"re_depth": depth, "_re_depth_hits": hits}, ["depth"], "FreiHand", a)
        return dic["depth"], depth, hits

    zero, d0, h0 = term(verts)
    assert float(zero) == 0.0 and tuple(d0.shape) == (B_MODEL, 1, H_MODEL, H_MODEL) and h0.dtype == torch.int32
    shifted = (verts + torch.tensor([0.0, 0.0, delta], device=verts.device)).contiguous().requires_grad_(True)
    fid1 = _render(rend, shifted.detach(), cam)
    _, h1 = ops.render_depth(rend, shifted.detach(), cam, fid1)
    full = ((h0 == AA_MODEL ** 2) & (h1 == AA_MODEL ** 2)).long()          # pixels fully covered before and after the shift
    assert int(full.sum()) > 10
    ex_full = dict(ex, segms_gt=full)
    value, d1, _ = term(shifted, ex_full)
    val = float(value.detach())
    # the restatement of the same number: float32 maps of both poses on the renderer's own face_id, the loss in float64
    faces = np.asarray(synth_tables.faces)
    want_d1, want_h1, _ = dr.depth_f32(shifted.detach().cpu().numpy(), cam.cpu().numpy(), faces, fid1.cpu().numpy(), H_MODEL, AA_MODEL)
    assert np.array_equal(want_d1.view(np.int32), d1.detach().cpu().numpy().reshape(want_d1.shape).view(np.int32))
    sums = dr.loss_sums_ordered(want_d1.reshape(B_MODEL, -1), want_h1.reshape(B_MODEL, -1), ex["depths"].cpu().numpy().reshape(B_MODEL, -1),
                                full.cpu().numpy().reshape(B_MODEL, -1), 0.0)
    want = dr.loss_value(sums, lam)
    print(f"[depth] shift by {delta}: term {val:.8e}, restatement {float(want):.8e}, lambda * delta {lam * delta:.8e}, "
          f"fully covered pixels {int(full.sum())}")
    assert dc.ulp_distance(np.asarray([val], np.float32), np.asarray([want], np.float32)) <= 1
    # one descent step: the farthest-moving vertex goes half of delta towards the target
    value.backward()
    g = shifted.grad
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 and float(g[..., 2].sum()) > 0
    stepped = (shifted.detach() - (0.5 * delta / float(g.abs().max())) * g).contiguous()
    after, _, _ = term(stepped, ex_full)
    print(f"[depth] descent step: {val:.6e} -> {float(after):.6e}")
    assert float(after) < val
    # the evaluation number: the term at lambda = 1
    ev = evaluate.Evaluator(depth=True)
    out = {"joints": torch.zeros(B_MODEL, 21, 3, device=verts.device), "mano_verts": torch.zeros(B_MODEL, 778, 3, device=verts.device),
           "re_depth": d1.detach(), "_re_depth_hits": h1}
    ev.collect(out, ex_full, "FreiHand")
    one, _, _ = term(shifted.detach(), ex_full, options.baseline_config2_args(losses=["depth"], lambda_depth=1.0))
    mae = ev.summary()["depth_mae"]
    assert abs(mae - float(one)) <= 2e-7 * float(one), (mae, float(one))
    assert abs(float(evaluate.depth_error(d1.detach(), h1, ex["depths"], full)) - mae) <= 1e-12


def _profiled_step(model, ex, args, losses):
    """Output keys and PROFILE launch names of one forward + backward."""
    from hifihr_amd import ops
    from hifihr_amd.losses import LossFunction
    root = ex["joints"][:, args.ROOT, :].unsqueeze(1)
    ops.PROFILE.enable()
    try:
        out = model("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
        e2 = dict(ex, joints=ex["joints"] - root, verts=ex["verts"] - root)
        dic = LossFunction()(e2, out, losses, "FreiHand", args)
        torch.stack([dic[k] for k in losses]).sum().backward()
        torch.cuda.synchronize()
        names = [e[0] for e in ops.PROFILE.events]
    finally:
        ops.PROFILE.disable()
        ops.PROFILE.events = []
    model.zero_grad(set_to_none=True)
    return out, names, dic


def test_model_emits_the_depth_map_only_with_the_option(synth_tables, scene):
    """Model(render_depth=True) at image_size 32, B = 2: re_depth is ops.render_depth on the forward's own face_id, bit for bit.  With the
    option off (or not given) the output keys and the PROFILE launch names of a forward + backward are those of a model built without
    the keyword, and none of the new names is among them; with it on, exactly the four new brackets are added."""
    from collections import Counter
    from hifihr_amd import ops, options
    ex = scene["ex"]
    base = options.baseline_config2_args(train_batch=B_MODEL)
    default, off, on = _model(synth_tables), _model(synth_tables, render_depth=False), _model(synth_tables, render_depth=True)
    o_def, n_def, _ = _profiled_step(default, ex, base, base.losses)
    o_off, n_off, _ = _profiled_step(off, ex, base, base.losses)
    args_on = options.baseline_config2_args(train_batch=B_MODEL, losses=base.losses + ["depth"])
    o_on, n_on, dic = _profiled_step(on, ex, args_on, args_on.losses)
    assert set(o_def) == set(o_off) and not {"re_depth", "_re_depth_hits"} & set(o_off)
    assert Counter(n_def) == Counter(n_off) and not NEW_PROFILE_NAMES & set(n_off), sorted(set(n_off))
    assert set(o_on) == set(o_off) | {"re_depth", "_re_depth_hits"}
    assert Counter(n_on) - Counter(n_off) == Counter(NEW_PROFILE_NAMES) and not Counter(n_off) - Counter(n_on)
    assert torch.equal(o_on["_rgba"], o_off["_rgba"]) and torch.equal(o_on["face_id"], o_off["face_id"])            # same seed, same weights
    cam = on.camera_from_K(ex["Ps"])
    depth, hits = ops.render_depth(on.renderer_p3d, o_on["skin_verts"].detach(), cam, o_on["face_id"])
    assert torch.equal(depth, o_on["re_depth"].detach()) and torch.equal(hits, o_on["_re_depth_hits"])
    assert tuple(depth.shape) == (B_MODEL, 1, H_MODEL, H_MODEL) and torch.equal(hits > 0, o_on["re_sil"][:, 0] > 0)
    assert bool(torch.isfinite(dic["depth"])) and float(dic["depth"].detach()) >= 0.0
    # the term reaches the hand encoder's heads
    grads = [float(p.grad.abs().max()) for p in on.hand_encoder.parameters() if p.grad is not None]
    assert not grads                                                      # (_profiled_step cleared them)
    root = ex["joints"][:, base.ROOT, :].unsqueeze(1)
    out = on("FreiHand", True, ex["imgs"], Ks=ex["Ps"], root_xyz=root)
    ops.depth_loss(out["re_depth"], out["_re_depth_hits"], ex["depths"]).backward()
    moved = max(float(p.grad.abs().max()) for p in on.hand_encoder.pose_reg.parameters() if p.grad is not None)
    assert moved > 0.0
