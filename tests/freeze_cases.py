"""Shared bodies of tests/test_gpu_freeze.py: training with frozen parameters, from single autograd functions to block chains.

Every case is a `Case`: our forward, the float64 CPU autograd restatement of the same operation (ReLU patterns taken from OUR forward, as
tests/test_gpu_conv.py::_run_dispatch_case does) and the leaves, whose requires_grad flags ARE the pattern under test -- the reference side
gives requires_grad to the same leaves only.  `run_case` runs forward + backward twice and asserts, for every case:

  1. outputs match the reference;
  2. every leaf that requires a gradient has one and it matches;
  3. every leaf that does not ends with .grad None -- or, where it carried a pre-set gradient buffer (direct mode: the parameter looks like
     one that FlatParams pinned and that was frozen afterwards), that buffer bit-unchanged;
  4. ops._ZERO_POOL's free lists hold as many buffers after the second iteration as after the first (a slot buffer acquired and never
     released shows as a shrinking or growing pool);
  5. no parameter is left with _hifihr_grad_deferred == True.

Bounds (none is new): 5e-5 (outputs, input gradients) / 1e-4 (parameter gradients) of _run_dispatch_case for the convolutions, 2e-4 behind a
batch-norm (bn_wino_* dispatch cases, kernel_cases.bn_act_case, linear_case, the trunk test), 3e-5 / 3e-4 of kernel_cases.se_case for
squeeze-excite; running statistics: rtol 1e-5 / 1e-4 (mean / variance), atol 1e-6 of kernel_cases.bn_act_case."""
import contextlib
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from test_gpu_conv import _bn_wino_setup, _conv_setup, _geoms, _leaf, _pair_setup, _param, _rand, _run_dispatch_case  # noqa: F401

SENTINEL = 0.375                  # what a frozen parameter's pre-set gradient buffer holds (direct mode)
EPS = 1e-5
CONV_TOL, BN_TOL, SE_TOL = (5e-5, 1e-4), (2e-4, 2e-4), (3e-5, 3e-4)
MODES = [(True, True), (True, False), (False, True), (False, False)]            # (direct, scope)
MODE_IDS = ["direct-scope", "direct-noscope", "autograd-scope", "autograd-noscope"]


class Case:
    def __init__(self, fwd, ref, inputs, params, use=None, after=None, finish=None, zero_grads=None):
        """fwd() -> our outputs; ref(ours, *leaves64) -> float64 outputs (ours: our outputs, detached, CPU, float64); inputs / params: the
        leaves (parameters get the direct-gradient treatment); use: which outputs reach the loss (None: all); after(): extra assertions
        behind each iteration; finish(iterations): extra assertions at the end (running statistics); zero_grads: {leaf index: absolute
        bound} for leaves whose true gradient is exactly zero (a bias in front of a train-mode batch-norm: kernel_cases.linear_case)."""
        self.fwd, self.ref, self.inputs, self.params, self.use, self.after, self.finish = fwd, ref, inputs, params, use, after, finish
        self.zero_grads = zero_grads or {}


def subsets(names, skip=()):
    """every non-empty subset of `names` (as frozensets), without those in `skip`"""
    out = [frozenset(c) for r in range(1, len(names) + 1) for c in itertools.combinations(names, r)]
    return [s for s in out if s not in {frozenset(k) for k in skip}]


def sid(s):
    return "+".join(sorted(s)) if s else "none"


def pool_count():
    from hifihr_amd import ops
    return sum(len(v) for v in ops._ZERO_POOL.free.values())


def close(a, b, rel, what):
    err, top = float((a.detach().cpu().double() - b.detach()).abs().max()), float(b.detach().abs().max())
    assert err <= rel * top + 1e-6, f"{what}: {err:.3e} of max {top:.3e} (bound {rel:g})"


def run_case(case, monkeypatch=None, *, direct, scope=True, tol=CONV_TOL, env=None, iterations=2):
    """-> the second iteration's ops.PROFILE.conv_log"""
    from hifihr_amd import ops
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    c = case
    for p in c.params:
        p._hifihr_direct_grad = direct
    pools, kept = [], {}
    pool, fresh = ops._ZERO_POOL, []

    def counting_acquire(n, device):                   # (an instance attribute over the class's method: ops.py is not touched)
        if not pool.free.get((n, device)):
            fresh[-1] += 1
        return type(pool).acquire(pool, n, device)
    monkeypatch_pool = contextlib.ExitStack()
    pool.acquire = counting_acquire
    monkeypatch_pool.callback(lambda: pool.__dict__.pop("acquire", None))
    with monkeypatch_pool:
        base, outs, use, log = _iterate(c, ops, direct, scope, iterations, pools, kept, fresh)
    assert pools[-1] == pools[0], f"_ZERO_POOL free buffers after each iteration: {pools}"
    # a buffer acquired and never released also shows as the NEXT iteration allocating a new one instead of finding it in the free list
    assert fresh[-1] == 0, f"_ZERO_POOL.acquire had to allocate in the last iteration (per iteration: {fresh}): a buffer was not released"
    _compare(c, outs, base, use, tol, direct, kept)
    if c.finish is not None:
        c.finish(iterations)
    return log


def _iterate(c, ops, direct, scope, iterations, pools, kept, fresh):
    base = None
    for it in range(iterations):
        fresh.append(0)
        for t in c.inputs:
            t.grad = None
        for i, p in enumerate(c.params):
            if not direct:
                p.grad = None
            elif p.requires_grad:
                p.grad = torch.zeros_like(p)
            else:                                      # frozen, yet pinned to a gradient buffer: the buffer must come back untouched
                p.grad = torch.full_like(p, SENTINEL)
                kept[i] = p.grad
        ops.PROFILE.enable()
        ops.PROFILE.conv_log.clear()
        try:
            with (ops.prepared_weights() if scope else contextlib.nullcontext()):
                outs = c.fwd()
                if base is None:
                    base = [_rand(o.shape, 99 + i) for i, o in enumerate(outs)]
                use = c.use if c.use is not None else [True] * len(outs)
                sum((o * g.cuda()).sum() for o, g, u in zip(outs, base, use) if u).backward()
            torch.cuda.synchronize()
            log = list(ops.PROFILE.conv_log)
        finally:
            ops.PROFILE.disable()
            ops.PROFILE.conv_log.clear()
        pools.append(pool_count())
        left = [i for i, p in enumerate(c.params) if getattr(p, "_hifihr_grad_deferred", False)]
        assert not left, f"iteration {it}: parameters {left} left with _hifihr_grad_deferred"
        if c.after is not None:
            c.after()
    return base, outs, use, log


def _compare(c, outs, base, use, tol, direct, kept):
    ours = [o.detach().cpu().double() for o in outs]
    leaves = c.inputs + c.params
    leaves64 = [t.detach().cpu().double().requires_grad_(t.requires_grad) for t in leaves]
    r = c.ref(ours, *leaves64)
    sum((o * g.double()).sum() for o, g, u in zip(r, base, use) if u).backward()
    for i, (a, b) in enumerate(zip(ours, r)):
        close(a, b, tol[0], f"output {i}")
    for i, (t, t64) in enumerate(zip(leaves, leaves64)):
        is_param = i >= len(c.inputs)
        if t.requires_grad:
            if t64.grad is None:                       # the reference's graph never reaches it (an output left out of the loss)
                assert t.grad is None or float(t.grad.abs().max()) == 0.0, f"leaf {i}: a gradient although nothing reaches it"
                continue
            assert t.grad is not None, f"no gradient for leaf {i}"
            if i in c.zero_grads:
                assert float(t64.grad.abs().max()) <= 1e-12 and float(t.grad.abs().max()) <= c.zero_grads[i], f"leaf {i}: gradient of a true zero"
                continue
            close(t.grad, t64.grad, tol[1] if is_param else tol[0], f"gradient of leaf {i}")
        elif is_param and direct:
            buf = kept[i - len(c.inputs)]
            assert t.grad is not None and t.grad.data_ptr() == buf.data_ptr() and bool((buf == SENTINEL).all()), f"frozen leaf {i}: its pre-set gradient buffer was written"
        else:
            assert t.grad is None, f"frozen leaf {i} ended with a gradient"


def _set_flags(leaves, names, pattern):
    for t, n in zip(leaves, names):
        t.requires_grad_(n in pattern)


_DRAIN = {}


def drain_stats(y, stats):
    """A convolution's batch statistics nobody reads: consumed (and the slot buffer cleaned and released) by a throw-away batch-norm, so that
    the pool accounting of run_case sees the buffer come back, as it does in a network."""
    from hifihr_amd import ops
    C = y.shape[1]
    bn = _DRAIN.get(C)
    if bn is None:
        bn = _DRAIN[C] = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        ops.bn_act(y.detach(), stats, bn, None, False)


# ---- A. single autograd functions ----------------------------------------------------------------------------------------------------------
def conv_case(geom, kind, pattern, fork=False, want_stats=False):
    """_Conv2dMFMA at one of _geoms()'s geometries; kind: "f4" / "f2" / "c64" (3x3, stride 1), "s2" (3x3, stride 2), "light" (bias + ReLU)."""
    from hifihr_amd import ops
    if kind == "light":
        fwd, ref, inputs, params = _conv_setup(*geom, 3, 1, 0, call="bias_act")
        _set_flags(inputs + params, ["x", "w", "b"], pattern)
        return Case(fwd, ref, inputs, params)
    stride = 2 if kind == "s2" else 1
    _, ref, inputs, params = _conv_setup(*geom, 3, stride, 1, fork=fork)
    _set_flags(inputs + params, ["x", "w"], pattern)
    x, w = inputs[0], params[0]

    def fwd():
        r = ops.conv2d(x, w, stride, 1, want_stats=want_stats, fork=fork)
        r = r if isinstance(r, tuple) else (r,)
        if want_stats:
            drain_stats(r[0], r[1])
        return [r[0]] + ([r[-1]] if fork else [])
    return Case(fwd, ref, inputs, params)


def pair_case(geom, pattern, use=None):
    from hifihr_amd import ops
    _, ref, inputs, params = _pair_setup(*geom)
    _set_flags(inputs + params, ["x", "w1", "w2"], pattern)
    x, (w1, w2) = inputs[0], params

    def fwd():
        y1, s1, y2, s2 = ops.conv2d_pair(x, w1, w2, 2)
        drain_stats(y1, s1); drain_stats(y2, s2)
        return [y1, y2]
    return Case(fwd, ref, inputs, params, use=use)


def _bn_module(C, momentum, seed, dims=2):
    bn = (torch.nn.BatchNorm2d if dims == 2 else torch.nn.BatchNorm1d)(C, eps=EPS, momentum=momentum).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * _rand((C,), seed)); bn.bias.copy_(0.1 * _rand((C,), seed + 1))
        bn.running_mean.copy_(0.1 * _rand((C,), seed + 2)); bn.running_var.copy_(1 + 0.1 * _rand((C,), seed + 3).abs())
    return bn


def _running_check(bn, momentum, box):
    """-> finish(iterations): momentum 0: the running statistics bit-identical to what they were; else the float64 update of `iterations`
    steps on the batch statistics of box["z"] (the float64 input of the batch-norm, channels in dim 1)"""
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()

    def finish(iterations):
        if momentum == 0:
            assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0), "running statistics moved at momentum 0"
            return
        z = box["z"].detach().transpose(0, 1).reshape(rm0.numel(), -1)
        rm, rv = rm0.cpu().double(), rv0.cpu().double()
        for _ in range(iterations):
            rm = (1 - momentum) * rm + momentum * z.mean(1)
            rv = (1 - momentum) * rv + momentum * z.var(1, unbiased=True)
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), rv.numpy(), rtol=1e-4, atol=1e-6)
    return finish


BN_SHAPE = (4, 256, 14, 14)       # the smallest of test_bn_act_kernels
BN_POOL_SHAPE = (5, 12, 9, 8)     # the smallest of test_bn_relu_maxpool_stem (N, C, H, W)


def bn_act_case(act, residual, pattern, momentum):
    """_BNAct: act "relu" / None / "swish"; pattern: subset of {x, gamma, beta, residual}"""
    from hifihr_amd import ops
    N, C, H, W = BN_SHAPE
    x = _leaf(_rand((N, C, H, W), 31, 1.5) + 0.3)
    res = _leaf(_rand((N, C, H, W), 32)) if residual else None
    bn = _bn_module(C, momentum, 33)
    inputs, params = [x] + ([res] if residual else []), [bn.weight, bn.bias]
    _set_flags(inputs + params, ["x"] + (["residual"] if residual else []) + ["gamma", "beta"], pattern)
    box = {}

    def fwd():
        return [ops.bn_act(x, None, bn, res, {"relu": True, None: False, "swish": "swish"}[act])]

    def ref(ours, x64, *rest):
        r64 = rest[0] if residual else None
        g64, b64 = rest[-2:]
        box["z"] = x64
        z = F.batch_norm(x64, None, None, g64, b64, True, 0.0, EPS)
        if residual:
            z = z + r64
        if act == "relu":
            z = z * (ours[0] > 0)
        elif act == "swish":
            z = z * torch.sigmoid(z)
        return [z]
    return Case(fwd, ref, inputs, params, finish=_running_check(bn, momentum, box))


def bn_pool_case(pattern, momentum):
    """_BNReluMaxPool at the smallest shape the fused kernels take; the statistics come from the library's own pass, as ops.bn_act takes them"""
    from hifihr_amd import ops
    from hifihr_amd._lib import get_lib
    lib = get_lib()
    N, C, H, W = BN_POOL_SHAPE
    assert lib.bn_relu_maxpool_supported(N, H, W, C)
    x = _leaf(_rand((N, C, H, W), 41, 1.5) + 0.3)
    bn = _bn_module(C, momentum, 43)
    inputs, params = [x], [bn.weight, bn.bias]
    _set_flags(inputs + params, ["x", "gamma", "beta"], pattern)
    box = {}

    def fwd():
        stats = ops._ZERO_POOL.acquire(lib.bn_stats_floats(C), x.device)
        lib.bn_stats(x.detach(), N * H * W, C, stats)
        y = ops.bn_relu_maxpool(x, stats, bn)
        assert y.grad_fn is None or type(y.grad_fn).__name__.startswith("_BNReluMaxPool"), y.grad_fn
        return [y]

    def ref(ours, x64, g64, b64):
        box["z"] = x64
        return [F.max_pool2d(F.relu(F.batch_norm(x64, None, None, g64, b64, True, 0.0, EPS)), 3, 2, 1)]
    return Case(fwd, ref, inputs, params, finish=_running_check(bn, momentum, box))


LINEAR_SHAPE = (8, 512, 128)      # B of tests/heads_fixture.py's he_mano512, the heads' first layer


def linear_case(with_bn, pattern, momentum=0.1):
    """_Linear (+ BatchNorm1d) + ReLU; pattern: subset of {x, w, b, gamma, beta}"""
    from hifihr_amd import ops
    B, I, O = LINEAR_SHAPE
    x = _leaf(_rand((B, I), 51))
    lin = torch.nn.Linear(I, O).cuda()
    with torch.no_grad():
        lin.weight.copy_(_rand((O, I), 52, I ** -0.5)); lin.bias.copy_(_rand((O,), 53, 0.1))
    bn = _bn_module(O, momentum, 54, dims=1) if with_bn else None
    inputs, params = [x], [lin.weight, lin.bias] + ([bn.weight, bn.bias] if with_bn else [])
    _set_flags(inputs + params, ["x", "w", "b", "gamma", "beta"], pattern)
    box = {}

    def fwd():
        return [ops.linear(x, lin, act=True, bn=bn)]

    def ref(ours, x64, w64, b64, g64=None, be64=None):
        z = F.linear(x64, w64, b64)
        if with_bn:
            box["z"] = z
            z = F.batch_norm(z, None, None, g64, be64, True, 0.0, EPS)
        return [z * (ours[0] > 0)]
    return Case(fwd, ref, inputs, params, finish=_running_check(bn, momentum, box) if with_bn else None,
                zero_grads={2: 1e-4} if with_bn else None)


GROUP_SHAPES = [(512, 128, True), (512, 128, True), (128, 10, False)]        # he_mano512: two heads' first layers on the shared base, a last layer


def linear_group_case(frozen, shared_grad, unused=None):
    """_LinearGroup: members 0 and 1 read the SAME input, member 2 its own; frozen: the members whose weight and bias are frozen; shared_grad:
    the shared input (and member 2's) requires a gradient; unused: the member whose output does not reach the loss."""
    from hifihr_amd import ops
    B = LINEAR_SHAPE[0]
    xs = _leaf(_rand((B, 512), 61), shared_grad)
    x2 = _leaf(_rand((B, 128), 62), shared_grad)
    lins = []
    for i, (I, O, _) in enumerate(GROUP_SHAPES):
        lin = torch.nn.Linear(I, O).cuda()
        with torch.no_grad():
            lin.weight.copy_(_rand((O, I), 63 + 2 * i, I ** -0.5)); lin.bias.copy_(_rand((O,), 64 + 2 * i, 0.1))
        lin.weight.requires_grad_(i not in frozen); lin.bias.requires_grad_(i not in frozen)
        lins.append(lin)
    params = [p for lin in lins for p in (lin.weight, lin.bias)]

    def fwd():
        return ops.linear_group([(xs, lins[0], True), (xs, lins[1], True), (x2, lins[2], False)])

    def ref(ours, xs64, x264, *p64):
        ys = [F.linear(xi, p64[2 * i], p64[2 * i + 1]) for i, xi in enumerate((xs64, xs64, x264))]
        return [y * (o > 0) if GROUP_SHAPES[i][2] else y for i, (y, o) in enumerate(zip(ys, ours))]
    use = [i != unused for i in range(3)]
    return Case(fwd, ref, [xs, x2], params, use=use)


SE_SHAPE = (8, 2304, 7, 7, 96)    # the smallest of test_squeeze_excite (B, C, H, W, SQ)
DW_SHAPE = (8, 816, 14, 14, 5, 1)  # the smallest of test_dwconv_kernels (N, C, H, W, K, stride)
MMPOOL_SHAPE = (4, 1536, 7, 7)    # the smallest of test_mmpool


def se_case(which):
    """_SqueezeExcite; which: "params" / "input" / "both" """
    from hifihr_amd import ops
    B, C, H, W, SQ = SE_SHAPE
    x = _leaf(_rand((B, C, H, W), 71), which != "params")
    pg = which != "input"
    w1, b1 = _param(_rand((SQ, C, 1, 1), 72, C ** -0.5), pg), _param(_rand((SQ,), 73, 0.1), pg)
    w2, b2 = _param(_rand((C, SQ, 1, 1), 74, SQ ** -0.5), pg), _param(_rand((C,), 75, 0.1), pg)

    def fwd():
        return [ops._SqueezeExcite.apply(x, w1, b1, w2, b2)]

    def ref(ours, x64, a, ab, c, cb):
        z1 = F.linear(x64.mean((2, 3)), a.reshape(SQ, C), ab)
        gate = torch.sigmoid(F.linear(z1 * torch.sigmoid(z1), c.reshape(C, SQ), cb))
        return [x64 * gate[:, :, None, None]]
    return Case(fwd, ref, [x], [w1, b1, w2, b2])


def dw_case(which):
    from hifihr_amd import ops
    from hifihr_amd.effnet import static_same_pad
    N, C, H, W, K, stride = DW_SHAPE
    pad4 = static_same_pad(K, stride)
    x = _leaf(_rand((N, C, H, W), 81), which != "params")
    w = torch.nn.Parameter((_rand((C, 1, K, K), 82) / K).cuda(), requires_grad=which != "input")

    def fwd():
        return [ops.dwconv2d(x, w, stride, pad4)]

    def ref(ours, x64, w64):
        return [F.conv2d(F.pad(x64, tuple(pad4)), w64, None, stride, 0, 1, C)]
    return Case(fwd, ref, [x], [w])


def mmpool_case(which):
    from hifihr_amd import ops
    B, C, H, W = MMPOOL_SHAPE
    x = _leaf(_rand((B, C, H, W), 91), which != "params")
    p = torch.nn.Parameter(torch.full((1,), 0.3).cuda(), requires_grad=which != "input")

    def fwd():
        return [ops.mmpool(x, p)]

    def ref(ours, x64, p64):
        s = torch.sigmoid(p64)
        return [(F.adaptive_max_pool2d(x64, (1, 1)) * s + F.adaptive_avg_pool2d(x64, (1, 1)) * (1 - s)).reshape(B, C)]
    return Case(fwd, ref, [x], [p])


# ---- B. chains that hand work between backward passes -------------------------------------------------------------------------------------
WINO_CHAIN_LEAVES = ["x0", "w0", "g1", "b1", "w1", "g2", "b2", "w2"]
WINO_CHAIN_PATTERNS = {
    "all": set(WINO_CHAIN_LEAVES),
    "f1_filter_frozen": set(WINO_CHAIN_LEAVES) - {"w1"},
    "f2_bn_frozen": set(WINO_CHAIN_LEAVES) - {"g2", "b2"},
    "only_f2_trains": {"g2", "b2", "w2"},              # nothing upstream of F2's input requires a gradient: F1's backward never runs
}


def wino_chain_case(geom, pattern):
    """conv2d(1x1, want_stats) -> bn_act_wino_conv (F1) -> bn_act_wino_conv (F2: its input is F1's raw output and _WinoLink) -> loss on F2's
    output, as BasicBlock chains them.  The two ReLU patterns: float64 batch-norm of OUR raw convolution outputs (the activations are never
    stored), as test_resnet18_trunk_backward_given_the_same_relu_pattern takes them."""
    from hifihr_amd import ops
    N, H, W, C, K = geom
    assert C == K
    x0 = _leaf(_rand((N, 64, H, W), 21))
    w0 = _param(_rand((C, 64, 1, 1), 22, 0.125))
    w1 = _param(_rand((K, C, 3, 3), 24, (9 * C) ** -0.5))
    w2 = _param(_rand((K, K, 3, 3), 27, (9 * K) ** -0.5))
    bn1, bn2 = _bn_module(C, 0.1, 25), _bn_module(K, 0.1, 28)
    inputs, params = [x0], [w0, bn1.weight, bn1.bias, w1, bn2.weight, bn2.bias, w2]
    _set_flags(inputs + params, WINO_CHAIN_LEAVES, pattern)
    box = {}

    def fwd():
        y0, st0 = ops.conv2d(x0, w0, 1, 0, want_stats=True)
        y1, st1, _ = ops.bn_act_wino_conv(y0, st0, bn1, None, w1, True)
        assert y1._hifihr_link is not None
        y2, _, _ = ops.bn_act_wino_conv(y1, st1, bn2, None, w2, False)
        box["y0"], box["y1"], box["link"] = y0.detach(), y1.detach(), y1._hifihr_link
        return [y2]

    def after():
        assert box["link"].red is None and box["link"].g is None, "F1's _WinoLink still holds F2's reduction buffer: nobody consumed the hand-off"

    def ref(ours, x64, w064, g1, b1, w164, g2, b2, w264):
        bn = lambda t, g, b: F.batch_norm(t, None, None, g, b, True, 0.0, EPS)
        m1 = bn(box["y0"].cpu().double(), g1.detach(), b1.detach()) > 0
        m2 = bn(box["y1"].cpu().double(), g2.detach(), b2.detach()) > 0
        a1 = bn(F.conv2d(x64, w064), g1, b1) * m1
        a2 = bn(F.conv2d(a1, w164, None, 1, 1), g2, b2) * m2
        return [F.conv2d(a2, w264, None, 1, 1)]
    return Case(fwd, ref, inputs, params, after=after)


BLOCK_PATTERNS = ["first_block_frozen", "convs_frozen", "bns_frozen"]


def block_chain_case(N, H, W, pattern, x_grad, monkeypatch):
    """network.BasicBlock(64 -> 128, stride 2, downsample) and the BasicBlock(128 -> 128) behind it (which takes the first one's output
    un-normalised, as in Resnet_4C) against oracle.torch_modules.BasicBlockRef in float64 with OUR ReLU patterns imposed.
    -> (case, blocks): parameters in named_parameters order of Sequential(block1, block2)."""
    import torch.nn as nn
    from hifihr_amd import checkpoint, network, ops
    import oracle.torch_modules as tm
    torch.manual_seed(7)
    b1 = network.BasicBlock(64, 128, 2, nn.Sequential(network.Conv2dMFMA(64, 128, 1, 2, 0), nn.BatchNorm2d(128)))
    b2 = network.BasicBlock(128, 128)
    b1.lazy_out = True
    net = nn.Sequential(b1, b2).cuda().train()
    with torch.no_grad():
        for i, m in enumerate(net.modules()):
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(1 + 0.1 * _rand((128,), 300 + i)); m.bias.copy_(0.1 * _rand((128,), 400 + i))
    if pattern == "first_block_frozen":
        checkpoint.rec_freeze(b1)                         # requires_grad off, batch-norm momentum 0: the reference's module-granular freeze
    else:
        for m in net.modules():
            if isinstance(m, network.Conv2dMFMA if pattern == "convs_frozen" else nn.BatchNorm2d):
                for p in m.parameters():
                    p.requires_grad_(False)
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    x = _leaf(_rand((N, 64, H, W), 201), x_grad)
    masks = []
    real_bn_act, real_fused = ops.bn_act, ops.bn_act_wino_conv

    def rec_bn_act(xx, stats, bn, residual=None, relu=True):
        y = real_bn_act(xx, stats, bn, residual, relu)
        if relu is True:
            masks.append((y.detach() > 0).cpu())
        return y

    def rec_fused(xx, stats, bn, residual, w, want_stats):
        z = F.batch_norm(xx.detach().double(), None, None, bn.weight.detach().double(), bn.bias.detach().double(), True, 0.0, bn.eps)
        if residual is not None:
            z = z + residual.detach().double()
        masks.append((z > 0).cpu())
        return real_fused(xx, stats, bn, residual, w, want_stats)
    frozen_bufs = [(n, b.clone()) for n, b in b1.named_buffers() if "running" in n] if pattern == "first_block_frozen" else []

    def fwd():
        masks.clear()
        monkeypatch.setattr(ops, "bn_act", rec_bn_act)
        monkeypatch.setattr(ops, "bn_act_wino_conv", rec_fused)
        try:
            return [net(x)]
        finally:
            monkeypatch.setattr(ops, "bn_act", real_bn_act)
            monkeypatch.setattr(ops, "bn_act_wino_conv", real_fused)

    def ref(ours, x64, *p64):
        assert len(masks) == 4, len(masks)                # two per BasicBlock, in execution order
        r1 = tm.BasicBlockRef(64, 128, 2, nn.Sequential(nn.Conv2d(64, 128, 1, 2, 0, bias=False), nn.BatchNorm2d(128)))
        r2 = tm.BasicBlockRef(128, 128)
        rnet = nn.Sequential(r1, r2).double().train()
        assert [n for n, _ in rnet.named_parameters()] == names
        it = iter(masks)
        real_relu = tm.F.relu

        def masked_relu(t, inplace=False):
            m = next(it)
            assert m.shape == t.shape
            return t * m.to(t.dtype)
        tm.F.relu = masked_relu
        try:
            y = torch.func.functional_call(rnet, dict(zip(names, p64)), (x64,))
        finally:
            tm.F.relu = real_relu
        return [y]

    def finish(iterations):
        for n, b0 in frozen_bufs:
            assert torch.equal(dict(b1.named_buffers())[n], b0), f"frozen block: {n} moved"
    return Case(fwd, ref, [x], params, finish=finish), (b1, b2)
