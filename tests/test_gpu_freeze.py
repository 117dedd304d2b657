"""GPU: training with frozen parameters (checkpoint.freeze_model_modules / rec_freeze and finer patterns), from single autograd functions to
the whole step.  The backward passes of ops.py do each other's work (paired products, fork residuals, shared dx, the _WinoLink hand-off), and
every such hand-off is a place where "this input needs no gradient" can drop or misplace someone else's.  tests/freeze_cases.py holds the
case bodies and the five assertions every case makes; the reference is float64 CPU autograd of the same operation with our ReLU patterns,
requires_grad on the same leaves only.  Every case runs with its parameters as flat-buffer targets (_hifihr_direct_grad, pre-zeroed .grad)
and with gradients handed to autograd; inside ops.prepared_weights() and without a scope where the function distinguishes them."""
import argparse

import numpy as np
import pytest
import torch

import freeze_cases as fc

pytestmark = pytest.mark.gpu

DIRECT = pytest.mark.parametrize("direct", [True, False], ids=["direct", "autograd"])
MODE = pytest.mark.parametrize("direct,scope", fc.MODES, ids=fc.MODE_IDS)


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


@pytest.fixture(scope="module")
def geoms(lib):
    G = dict(fc._geoms(lib))
    G["c64"] = tuple(G["c64"]) + (64, 64)
    return G


# ---- A. single autograd functions over every requires-grad pattern -------------------------------------------------------------------------
# _Conv2dMFMA.  (kind, pattern, fork, want_stats); left out, because tests/test_gpu_conv.py's dispatch cases name them: {x, w} without fork
# on every geometry, c64 with x only / w only / x only + fork, {x, w} + fork on s2, {x, w} + statistics on f4 and s2, {x, w, b} on light.
# New in substance: w only on f4 / f2 (the wino_w branch with its own dy transform), b only on light, fork with a frozen filter on s2.
_X, _W, _XW = frozenset("x"), frozenset("w"), frozenset("xw")
CONV_ROWS = ([(k, p, False, False) for k in ("f4", "f2", "s2") for p in (_X, _W)]
             + [(k, p, True, False) for k in ("f4", "f2") for p in (_X, _XW)] + [("s2", _X, True, False), ("c64", _XW, True, False)]
             + [(k, p, False, True) for k in ("f4", "s2") for p in (_X, _W)]
             + [("light", p, False, False) for p in fc.subsets("xwb", skip=["xwb"])])


def _conv_id(row):
    kind, pattern, fork, stats = row
    return f"{kind}-{fc.sid(pattern)}" + ("-fork" if fork else "") + ("-stats" if stats else "")


@MODE
@pytest.mark.parametrize("row", CONV_ROWS, ids=_conv_id)
def test_conv2d_requires_grad_patterns(geoms, monkeypatch, row, direct, scope):
    kind, pattern, fork, stats = row
    log = fc.run_case(fc.conv_case(geoms[kind], kind, pattern, fork=fork, want_stats=stats), monkeypatch, direct=direct, scope=scope)
    if kind in ("f4", "f2") and pattern == _W:
        # the Winograd weight gradient alone: the forward product and the Y' . V product, no backward-data product of either form
        N, H, W, C, K = geoms[kind]
        m = 4 if kind == "f4" else 2
        assert sorted(d for _, d in log) == ["gemm", "gemm-tn"], log
        assert {g for g, _ in log} == {("wino", N, H, W, C, K, m)}, log


PAIR_ROWS = [(p, None) for p in fc.subsets(["x", "w1", "w2"])] + [(frozenset(["x", "w1", "w2"]), [True, False]), (frozenset(["x", "w1", "w2"]), [False, True])]


@MODE
@pytest.mark.parametrize("row", PAIR_ROWS, ids=lambda r: fc.sid(r[0]) + ("" if r[1] is None else "-gy2none" if r[1][0] else "-gy1none"))
def test_conv2d_pair_requires_grad_patterns(geoms, monkeypatch, row, direct, scope):
    """conv1 + downsample[0] of a stage's first block: the three shapes of _Conv2dPair.backward (plus1x1 with both weight gradients, plus1x1
    with one, the fork fallback) under every subset of {x, w1, w2}, and with one output only reaching the loss."""
    pattern, use = row
    fc.run_case(fc.pair_case(geoms["s2"], pattern, use=use), monkeypatch, direct=direct, scope=scope)


BN_KINDS = {"relu_res": ("relu", True), "relu": ("relu", False), "linear": (None, False), "swish": ("swish", False)}


@DIRECT
@pytest.mark.parametrize("momentum", [0.1, 0], ids=["momentum0.1", "momentum0"])
@pytest.mark.parametrize("kind", list(BN_KINDS))
def test_bn_act_requires_grad_patterns(lib, kind, momentum, direct):
    """_BNAct computes dgamma / dbeta whatever needs_input_grad says: every subset of {x, gamma, beta, residual}; momentum 0 (what rec_freeze
    sets) leaves the running statistics bit-unchanged although the train-mode kernels still use batch statistics."""
    act, residual = BN_KINDS[kind]
    for pattern in fc.subsets(["x", "gamma", "beta"] + (["residual"] if residual else [])):
        try:
            fc.run_case(fc.bn_act_case(act, residual, pattern, momentum), direct=direct, tol=fc.BN_TOL)
        except AssertionError as e:
            raise AssertionError(f"pattern {fc.sid(pattern)}: {e}") from e


@DIRECT
@pytest.mark.parametrize("momentum", [0.1, 0], ids=["momentum0.1", "momentum0"])
def test_bn_relu_maxpool_requires_grad_patterns(lib, momentum, direct):
    for pattern in fc.subsets(["x", "gamma", "beta"]):
        try:
            fc.run_case(fc.bn_pool_case(pattern, momentum), direct=direct, tol=fc.BN_TOL)
        except AssertionError as e:
            raise AssertionError(f"pattern {fc.sid(pattern)}: {e}") from e


@DIRECT
@pytest.mark.parametrize("with_bn,momentum", [(False, 0.1), (True, 0.1), (True, 0)], ids=["plain", "bn", "bn-momentum0"])
def test_linear_requires_grad_patterns(lib, with_bn, momentum, direct):
    names = ["x", "w", "b"] + (["gamma", "beta"] if with_bn else [])
    for pattern in fc.subsets(names):
        try:
            fc.run_case(fc.linear_case(with_bn, pattern, momentum), direct=direct, tol=fc.BN_TOL if with_bn else fc.CONV_TOL)
        except AssertionError as e:
            raise AssertionError(f"pattern {fc.sid(pattern)}: {e}") from e


GROUP_ROWS = ([(frozenset(f), sg, None) for sg in (True, False) for f in [()] + [tuple(s) for s in fc.subsets([0, 1, 2])] if sg or len(f) < 3]
              + [(frozenset(), True, u) for u in range(3)] + [(frozenset([0]), True, 0)])


@DIRECT
@pytest.mark.parametrize("row", GROUP_ROWS, ids=lambda r: "frozen" + "".join(map(str, sorted(r[0]))) + ("-dx" if r[1] else "-nodx")
                         + ("" if r[2] is None else f"-unused{r[2]}"))
def test_linear_group_requires_grad_patterns(lib, row, direct):
    """_LinearGroup shares ONE dx between the members that read the same input and returns it from the first of them: every subset of
    members frozen (with only member 0 frozen the shared dx still is the sum of both members' products), the shared input with and
    without a gradient (only_train_texture: some heads frozen, the base features carry none), one member's output unused."""
    frozen, shared_grad, unused = row
    fc.run_case(fc.linear_group_case(frozen, shared_grad, unused), direct=direct)


@MODE
@pytest.mark.parametrize("which", ["params", "input", "both"])
def test_squeeze_excite_requires_grad_patterns(lib, which, direct, scope):
    fc.run_case(fc.se_case(which), direct=direct, scope=scope, tol=fc.SE_TOL)


@DIRECT
@pytest.mark.parametrize("which", ["params", "input", "both"])
def test_dwconv_requires_grad_patterns(lib, which, direct):
    fc.run_case(fc.dw_case(which), direct=direct)


@DIRECT
@pytest.mark.parametrize("which", ["params", "input", "both"])
def test_mmpool_requires_grad_patterns(lib, which, direct):
    """(p alone: a frozen trunk under a trainable mixing scalar -- once a NotImplementedError)"""
    fc.run_case(fc.mmpool_case(which), direct=direct)


# ---- B. chains that hand work between backward passes --------------------------------------------------------------------------------------
WINO_ROWS = [(n, None) for n in fc.WINO_CHAIN_PATTERNS] + [("only_f2_trains", {"HIFIHR_BN_WINO_BWD": "0"})]


@MODE
@pytest.mark.parametrize("row", WINO_ROWS, ids=lambda r: r[0] + ("-unfused_bwd" if r[1] else ""))
def test_wino_link_chain_requires_grad_patterns(geoms, monkeypatch, row, direct, scope):
    """_BNActWinoConv hands its batch-norm apply (dx, dgamma, dbeta) to the PRODUCER's backward through the _WinoLink.  "only_f2_trains": the
    first convolution, F1's batch-norm and filter frozen, the input without a gradient, F2's batch-norm and filter trainable flat-buffer
    parameters -- autograd never calls F1's backward, so F2 must apply its batch-norm itself: dgamma / dbeta / dw match, the reduction
    buffer is back in the pool, nothing is left deferred.  (Before the hand-off asked needs_input_grad[0]: dgamma / dbeta never written,
    link.red never released, the flags left True.)"""
    name, env = row
    fc.run_case(fc.wino_chain_case(geoms["f4"], fc.WINO_CHAIN_PATTERNS[name]), monkeypatch, direct=direct, scope=scope, tol=fc.BN_TOL, env=env)


@MODE
@pytest.mark.parametrize("x_grad", [True, False], ids=["xgrad", "xfrozen"])
@pytest.mark.parametrize("pattern", fc.BLOCK_PATTERNS)
def test_basic_block_chain_requires_grad_patterns(geoms, monkeypatch, pattern, x_grad, direct, scope):
    """A stage's first BasicBlock (stride 2, downsample branch) and the block after it at the s2 -> f4 geometries, bound 2e-4 of
    test_resnet18_trunk_backward_given_the_same_relu_pattern."""
    N = geoms["f4"][0]
    case, _ = fc.block_chain_case(N, 28, 28, pattern, x_grad, monkeypatch)
    fc.run_case(case, monkeypatch, direct=direct, scope=scope, tol=fc.BN_TOL)


# ---- C. the reference's own freeze modes on the model -------------------------------------------------------------------------------------
def _frozen_names(model):
    return {n for n, p in model.named_parameters() if not p.requires_grad}


@pytest.mark.parametrize("mode", ["only_train_texture", "only_train_regressor"])
def test_backward_chain_from_features_with_frozen_modules(mode):
    """test_backward_chain_matches_oracle_from_features (B = 6, its 5e-3 relative bound) after checkpoint.freeze_model_modules, the same-named
    parameters of the OracleModel frozen too: every trainable non-encoder parameter's gradient within the bound, every frozen one None.
    only_train_texture freezes the encoder, so the features carry no gradient either (the heads' shared input, the light branch's input)."""
    from hifihr_amd import checkpoint
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.traineval import trans_proj_j2d
    from oracle.model_oracle import oracle_step
    from test_gpu_e2e import _setup
    tables, args, model, ref, ex, ex_cpu = _setup(6)
    frozen_roots = checkpoint.freeze_model_modules(model, argparse.Namespace(**{mode: True}))
    assert frozen_roots
    frozen = _frozen_names(model)
    for n, p in ref.named_parameters():
        p.requires_grad_(n not in frozen)
    feat_grad = mode == "only_train_regressor"
    with torch.no_grad():
        low, feat = model.base_encoder(ex["imgs"])
    low_g, feat_g = low.clone().requires_grad_(feat_grad), feat.clone().requires_grad_(feat_grad)
    low_c, feat_c = low.cpu().clone().requires_grad_(feat_grad), feat.cpu().clone().requires_grad_(feat_grad)
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
    pairs = [("d/d feat", feat_g.grad, feat_c.grad), ("d/d low", low_g.grad, low_c.grad)] if feat_grad else []
    if not feat_grad:
        assert feat_g.grad is None and low_g.grad is None
    rgrads = dict(ref.named_parameters())
    trainable = 0
    for name, p in model.named_parameters():
        if name in frozen:
            assert p.grad is None, f"frozen {name} has a gradient"
            continue
        if name.startswith("base_encoder"):
            continue
        if name in ("hand_encoder.base_layers.0.bias", "hand_encoder.base_layers.3.bias"):
            continue        # a bias in front of BatchNorm: the true gradient is exactly 0, both sides hold rounding noise
        rg = rgrads[name].grad
        if rg is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, f"trainable {name} has no gradient"
        pairs.append((name, p.grad, rg))
        trainable += 1
    assert trainable > 0
    gmax = max(float(r.abs().max()) for _, _, r in pairs)
    errs = []
    for name, g, r in pairs:
        scale = max(float(r.abs().max()), 1e-4 * gmax)
        errs.append((float((g.detach().cpu() - r).abs().max()) / scale, name))
    print(mode, "worst relative gradient errors:", sorted(errs, reverse=True)[:6])
    assert max(errs)[0] < 5e-3, sorted(errs, reverse=True)[:6]


def _frozen_state(model, roots):
    """(frozen parameters, batch-norm running statistics below the frozen roots), cloned"""
    params = {n: p.detach().clone() for n, p in model.named_parameters() if not p.requires_grad}
    bufs = {}
    for r in roots:
        sub = model
        for part in r.split("."):
            sub = getattr(sub, part)
        bufs.update({f"{r}.{n}": b.detach().clone() for n, b in sub.named_buffers() if "running" in n})
    return params, bufs


def _assert_frozen_state(model, state, tag):
    params, bufs = state
    named, nbufs = dict(model.named_parameters()), dict(model.named_buffers())
    moved = [n for n, v in params.items() if not torch.equal(named[n].detach(), v)]
    assert not moved, f"{tag}: frozen parameters moved: {moved[:6]}"
    moved = [n for n, v in bufs.items() if not torch.equal(nbufs[n], v)]
    assert not moved, f"{tag}: running statistics below a frozen root moved: {moved[:6]}"


def test_whole_step_with_only_train_texture():
    """freeze_model_modules(only_train_texture) -> FlatParams -> FusedAdam -> two eager steps, then the captured step replayed twice: frozen
    parameters and the running statistics below the frozen roots bit-identical throughout, every un-frozen sub-module moves, the step-0
    loss terms within the north_star bound (1e-4 max(1, |b|)) of an un-frozen replica's from the same weights (freezing changes no forward
    value; unprepared frozen filters may run on other kernels, hence the bound rather than bit-equality), no side branch left pending."""
    from hifihr_amd import checkpoint, ops
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, train_step
    from test_gpu_e2e import _setup
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        tables, args, model, ref, ex, ex_cpu = _setup(4, graded=True)
        replica = Model(True, torch.device("cuda"), False, "mano", False, "res18", mano_tables=tables).cuda().train()
        replica.load_state_dict(model.state_dict())
        roots = checkpoint.freeze_model_modules(model, argparse.Namespace(only_train_texture=True))
        assert roots == ["base_encoder", "hand_encoder.base_layers", "hand_encoder.pose_reg", "hand_encoder.shape_reg"]
        state = _frozen_state(model, roots)
        assert state[0] and state[1]
        flat = FlatParams(model); opt = FusedAdam(flat, lr=1e-4)
        assert flat.param_count() == sum(p.numel() for p in model.parameters() if p.requires_grad)
        flat_r = FlatParams(replica); opt_r = FusedAdam(flat_r, lr=1e-4)
        start = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
        start0 = {n: p.detach().clone() for n, p in replica.named_parameters()}
        loss0, dic0 = train_step(model, LossFunction(), opt, ex, args)
        loss_r, dic_r = train_step(replica, LossFunction(), opt_r, ex, args)
        torch.cuda.synchronize()
        for k in list(args.losses) + ["loss"]:
            a, b = float(dic0[k].detach()), float(dic_r[k].detach())
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (k, a, b)
        train_step(model, LossFunction(), opt, ex, args)
        torch.cuda.synchronize()
        _assert_frozen_state(model, state, "two eager steps")
        assert not [n for n, p in model.named_parameters() if not p.requires_grad and p.grad is not None]
        assert not [n for n, p in model.named_parameters() if getattr(p, "_hifihr_grad_deferred", False)]
        # every un-frozen sub-module moves -- those that move in the un-frozen replica, that is: the MANO model reads the pose and shape heads
        # only (trans / rot / scale reach no loss, as in the reference's model) and their parameters stay put in any mode
        rnamed = dict(replica.named_parameters())
        root_of = lambda n: ".".join(n.split(".")[:2])
        live = {root_of(n) for n, v in start0.items() if not torch.equal(rnamed[n].detach(), v)}
        trainable_roots = sorted({root_of(n) for n in start} & live)
        assert trainable_roots == ["light_estimator.base_layers", "light_estimator.light_reg"] and "hand_encoder.pose_reg" in live
        named = dict(model.named_parameters())
        for r in trainable_roots:
            assert any(not torch.equal(named[n].detach(), v) for n, v in start.items() if n.startswith(r + ".")), f"nothing in {r} moved"
        step = GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=2)
        before = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
        for _ in range(2):
            loss, dic = step()
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        _assert_frozen_state(model, state, "captured step")
        assert not ops.side_branch._pending, "a side branch was left un-joined"
        assert not [n for n, p in model.named_parameters() if getattr(p, "_hifihr_grad_deferred", False)]
        for r in trainable_roots:
            assert any(not torch.equal(named[n].detach(), v) for n, v in before.items() if n.startswith(r + ".")), f"replay: nothing in {r} moved"
        step.release()
    finally:
        torch.cuda.set_stream(prev)


def test_late_freeze_fails_on_the_host():
    """requires_grad turned off on a parameter that already lives in a FlatParams: flat Adam cannot honour it (its moments keep moving the
    parameter), so the next train_step / graphed-step construction raises a ValueError naming it before any launch -- nothing has moved --
    and ops._direct_grad no longer calls its pinned buffer a gradient target."""
    from hifihr_amd import ops
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, train_step
    from test_gpu_e2e import _setup
    tables, args, model, ref, ex, ex_cpu = _setup(2)
    flat = FlatParams(model); opt = FusedAdam(flat, lr=1e-4)
    p = model.base_encoder.encoder1.model.layer2[0].bn1.weight
    assert ops._direct_grad(p)
    p.requires_grad_(False)
    assert not ops._direct_grad(p) and p.grad is not None
    before, bufs = flat.flat.clone(), [b.clone() for b in model.buffers()]
    with pytest.raises(ValueError, match=r"base_encoder\.encoder1\.model\.layer2\.0\.bn1\.weight"):
        train_step(model, LossFunction(), opt, ex, args)
    with pytest.raises(ValueError, match=r"base_encoder\.encoder1\.model\.layer2\.0\.bn1\.weight"):
        GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=1)
    torch.cuda.synchronize()
    assert torch.equal(flat.flat, before) and opt.step_count == 0 and not opt.graph_mode
    assert all(torch.equal(a, b) for a, b in zip(model.buffers(), bufs)), "a launch ran before the check"
    p.requires_grad_(True)                                  # thawed again: the step runs
    loss, _ = train_step(model, LossFunction(), opt, ex, args)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss))
