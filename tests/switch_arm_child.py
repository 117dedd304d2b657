"""One arm of tests/switch_arms.py in a process of its own (not collected by pytest):

    python tests/switch_arm_child.py ARM DEVICE [JSON of the default process's dispatch geometries]

DEVICE is `cpu` (the emulator library, tests/hostsim) or `cuda` (the product library).  The parent sets the arm's environment: most of the
switches are cached at import or at first use, so every arm -- `default` too -- needs a fresh process.  Runs the arm's cases through the
shared case bodies (tests/kernel_cases.py, tests/test_gpu_conv.py, tests/test_gpu_e2e.py: their own bounds) and answers the arm's witness
queries; `default` answers the queries of EVERY arm of the device, which is what each arm's answers are compared with.  Prints one JSON
line, the last line of stdout:

    {"arm", "device", "cases": [{"case", "accepted", "ratio"}], "witness": [...] (default: {arm: [...]}), "geoms", "seconds", ...}

ratio: the largest err / bound the case's assertions saw.  Any failed assertion: the traceback on stderr and a non-zero exit."""
import contextlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import switch_arms as sa  # noqa: E402

T0 = time.time()
_MEMO = {}


class _Env:
    """what _run_dispatch_case wants of pytest's monkeypatch"""

    def setenv(self, k, v):
        os.environ[k] = v


_DEVICE = [None]


def _route(name):
    """a route of kernel_cases.GEMM_ROUTES -- on the emulator only: it stands in for a device the emulator does not have"""
    import kernel_cases as kc
    return kc.gemm_route(name) if (name and _DEVICE[0] == "cpu") else contextlib.nullcontext()


def _key(q):
    return json.dumps(q, sort_keys=True)


def _ratio_logs():
    import kernel_cases as kc
    return [kc.CONV_CONTRACT_LOG, kc.LAYER_CONTRACT_LOG]


def _worst_ratio():
    return max([float(row[2]) for log in _ratio_logs() for row in log.values()] + [0.0])


# ---- the dispatch cases of tests/test_gpu_conv.py, on the geometries the DEFAULT process picked -------------------------------------------
def _dispatch_geoms(lib, given):
    import test_gpu_conv as tg
    if "geoms" not in _MEMO:
        _MEMO["geoms"] = {k: tuple(v) for k, v in given.items()} if given else tg._geoms(lib)
        tg._geoms = lambda _lib: _MEMO["geoms"]          # (an arm's predicates may refuse what the default process picked: same layers in both)
    return _MEMO["geoms"]


def _stem_block_geom(lib):
    """the smallest image on which the stem kernel, its 3-channel weight gradient and the fused batch-norm + pool all run"""
    import test_gpu_conv as tg
    return tg._pick([(1, 8, 28), (1, 8, 56), (2, 8, 56), (2, 16, 56), (2, 56, 56), (4, 56, 56)],
                    lambda N, H, W: (lib.conv2d_describe(N, H, W, 4, 64, 7, 7, 2, 3, 0) == "conv_stem_kernel"
                                     and lib.conv2d_bwd_weight_c3_supported(N, H, W, 64, 7, 7, 2, 3)
                                     and lib.bn_relu_maxpool_supported(N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)), "the stem block")


def _stem_block_setup(N, H, W):
    """-> (fwd, ref, inputs, params) in _run_dispatch_case's form: the 7x7 / stride 2 stem on an NHWC4 image with statistics, then
    ops.bn_relu_maxpool.  The float64 reference takes OUR ReLU and arg-max pattern (as _conv_setup does for ReLU): of every 3x3 window it
    reads the tap whose value is nearest to our output, and nothing where ours is zero -- which side of zero a float rounds to, and which
    of two near-equal taps wins, is not the dispatch's business."""
    import torch
    import torch.nn.functional as F
    import test_gpu_conv as tg
    from hifihr_amd import ops
    x = tg._rand((N, 4, H, W), N + H + 4)
    x[:, 3] = 0
    x = tg._leaf(x, False)
    w = tg._param(tg._rand((64, 3, 7, 7), 71, (3 * 49) ** -0.5))
    bn = torch.nn.BatchNorm2d(64).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * tg._rand((64,), 25)); bn.bias.copy_(0.1 * tg._rand((64,), 26))

    def fwd():
        h, st = ops.conv2d(x, w, 2, 3, want_stats=True)
        return [ops.bn_relu_maxpool(h, st, bn)]

    def ref(ours, x64, w64, g64, b64):
        z = F.batch_norm(F.conv2d(x64[:, :3], w64, None, 2, 3), None, None, g64, b64, True, 0.0, bn.eps)
        win = F.pad(z, (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2).reshape(*ours[0].shape, 9)
        tap = (win.detach() - ours[0].unsqueeze(-1)).abs().argmin(-1, keepdim=True)
        got, live = win.gather(-1, tap).squeeze(-1), ours[0] > 0
        # the pattern is ours, the forward is not: the tap we took is the window's maximum, and what we zeroed was not positive -- both
        # to the 2e-4 the outputs are held to (a pool that returned another tap, or dropped a positive output, fails here in either arm)
        top = win.detach().max(-1).values
        bound = 2e-4 * float(top.abs().max()) + 1e-6
        assert float(torch.where(live, top - got.detach(), torch.zeros_like(top)).max()) <= bound, "a pooled output is not its window's maximum"
        assert float(torch.where(live, torch.zeros_like(top), top).max()) <= bound, "a positive window maximum came out as zero"
        return [got * live]
    return fwd, ref, [x], [w, bn.weight, bn.bias]


def _defer_chain_setup(lib, c64, f4):
    """What stands around ops._DEFER_DW in a step, in one prepared_weights scope: the stem block (whose pooling backward is where the early
    flush fires), behind it a 64 -> 64 layer (its weight gradient's slab sum is deferred: add_halo), and beside them an F(4x4) layer (its
    weight-gradient transform is deferred: add) built LAST, so that autograd runs its backward first and the early flush finds both jobs.
    Every weight gradient against float64: a deferred launch that is lost, runs twice or runs before its slabs are complete shows there."""
    import torch.nn.functional as F
    import test_gpu_conv as tg
    from hifihr_amd import ops
    N, H, W = c64
    assert (lib.conv2d_describe(N, 4 * H, 4 * W, 4, 64, 7, 7, 2, 3, 0) == "conv_stem_kernel" and lib.conv2d_bwd_weight_c3_supported(N, 4 * H, 4 * W, 64, 7, 7, 2, 3)
            and lib.bn_relu_maxpool_supported(N, 2 * H, 2 * W, 64)), "the stem block in front of the 64 -> 64 layer"
    sfwd, sref, sin, spar = _stem_block_setup(N, 4 * H, 4 * W)
    wc = tg._param(tg._rand((64, 64, 3, 3), 73, (9 * 64) ** -0.5))
    ffwd, fref, fin, fpar = tg._conv_setup(*f4, 3, 1, 1)

    def fwd():
        p = sfwd()[0]
        return [p, ops.conv2d(p, wc, 1, 1)] + ffwd()

    def ref(ours, x64, x2, w64, g64, b64, wc64, wf64):
        p = sref(ours[:1], x64, w64, g64, b64)[0]
        return [p, F.conv2d(p, wc64, None, 1, 1)] + fref(ours[2:], x2, wf64)
    return fwd, ref, sin + fin, spar + [wc] + fpar


def _bn_block_setup(N, H, W, C, K):
    """test_gpu_conv._bn_wino_setup's block as network.BasicBlock writes it: batch-norm + ReLU inside the next convolution's Winograd input
    transform where ops.bn_wino_fusable says so, else ops.bn_act and a convolution of its own.  The same float64 reference either way."""
    import torch
    import torch.nn.functional as F
    import test_gpu_conv as tg
    from hifihr_amd import ops
    x0 = tg._leaf(tg._rand((N, 64, H, W), 21))
    w0 = tg._param(tg._rand((C, 64, 1, 1), 22, 0.125), False)
    res = tg._leaf(tg._rand((N, C, H, W), 23))
    w = tg._param(tg._rand((K, C, 3, 3), 24, (9 * C) ** -0.5))
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * tg._rand((C,), 25)); bn.bias.copy_(0.1 * tg._rand((C,), 26))

    def fwd():
        xr, st = ops.conv2d(x0, w0, 1, 0, want_stats=True)
        if ops.bn_wino_fusable(xr, w, bn, 1, 1):
            y, _, out = ops.bn_act_wino_conv(xr, st, bn, res, w, False)
        else:
            out = ops.bn_act(xr, st, bn, res, True)
            y = ops.conv2d(out, w, 1, 1)
        return [y, out]

    def ref(ours, x64, r64, w064, w64, g64, b64):
        z = F.batch_norm(F.conv2d(x64, w064), None, None, g64, b64, True, 0.0, bn.eps) + r64
        a = z * (ours[1] > 0)
        return [F.conv2d(a, w64, None, 1, 1), a]
    return fwd, ref, [x0, res], [w0, w, bn.weight, bn.bias]


def _pair_block_setup(N, H, W, C, K):
    """test_gpu_conv._pair_setup's two convolutions as network.BasicBlock writes them: ONE launch where ops.conv2d_pair_ok says so, else
    the strided 3x3 with statistics and a fork, and the 1x1 twin on the alias the fork hands back.  The same float64 reference either way."""
    import test_gpu_conv as tg
    from hifihr_amd import ops
    _, ref, (x,), (w1, w2) = tg._pair_setup(N, H, W, C, K)

    def fwd():
        if ops.conv2d_pair_ok(x, w1, w2, 2):
            y1, _, y2, _ = ops.conv2d_pair(x, w1, w2, 2)
        else:
            y1, _, xa = ops.conv2d(x, w1, 2, 1, want_stats=True, fork=True)
            y2, _ = ops.conv2d(xa, w2, 2, 0, want_stats=True)
        return [y1, y2]
    return fwd, ref, [x], [w1, w2]


def _resolve_log(G, tags):
    """[(tag, direction)] of tests/switch_arms.py -> the ops.PROFILE.conv_log entries they stand for"""
    d9 = lambda N, H, W, C, K, R, st, pd: (N, H, W, C, K, R, R, st, pd)
    N, H, W, C, K = G["f4"]
    ns, hs, ws_, cs, ks = G["s2"]
    nc, hc, wc = G["c64"]
    st_ = G["stem"]
    n2, h2, w2, c2, k2 = G["f2"]
    names = {"f4": ("wino", N, H, W, C, K, 4), "f4T": ("wino", N, H, W, K, C, 4), "f4m2": ("wino", N, H, W, C, K, 2), "f4Tm2": ("wino", N, H, W, K, C, 2),
             "f2": ("wino", n2, h2, w2, c2, k2, 2), "f2T": ("wino", n2, h2, w2, k2, c2, 2), "f2d": d9(n2, h2, w2, c2, k2, 3, 1, 1),
             "f4d": d9(N, H, W, C, K, 3, 1, 1), "p1": d9(N, H, W, 64, C, 1, 1, 0), "gc": d9(nc, hc, wc, 64, 64, 3, 1, 1), "gs": d9(ns, hs, ws_, cs, ks, 3, 2, 1),
             "gs1": d9(ns, hs, ws_, cs, ks, 1, 2, 0), "gsc": d9(nc, 4 * hc, 4 * wc, 4, 64, 7, 2, 3), "pair": ("pair", ns, hs, ws_, cs, ks, ks, 2), "gst": d9(*st_[:3], 4, *st_[3:])}
    if "stemb" in G:
        names["gsb"] = d9(*G["stemb"], 4, 64, 7, 2, 3)
    return [(names[t], d) for t, d in tags]


def _counting(lib, names):
    """wraps the C-ABI entries `names` of the library object: -> counts, undo"""
    counts, saved = {n: 0 for n in names}, {}
    for n in names:
        f = getattr(lib, n)
        saved[n] = f

        def g(*a, _f=f, _n=n, **kw):
            counts[_n] += 1
            return _f(*a, **kw)
        setattr(lib, n, g)
    return counts, lambda: [setattr(lib, n, f) for n, f in saved.items()]


def run_dispatch(lib, given, name, log, count=()):
    """One dispatch case with the conv_log the table expects of THIS process; -> (ratio, bracket names of its launches, entry counts)"""
    import test_gpu_conv as tg
    from hifihr_amd import ops
    G = dict(_dispatch_geoms(lib, given))
    behind_bn = dict(direct=True, tol=2e-4, wtol=2e-4)          # (the bound behind a batch-norm: the trunk tests', bn_wino_fused's)
    if name == "stem_block":
        if "stemb" not in _MEMO["geoms"]:
            _MEMO["geoms"]["stemb"] = _stem_block_geom(lib)
        G = dict(_MEMO["geoms"])
        setup, opts = (lambda: _stem_block_setup(*G["stemb"])), behind_bn
    elif name == "defer_chain":
        setup, opts = (lambda: _defer_chain_setup(lib, G["c64"], G["f4"])), behind_bn
    elif name == "bn_block":
        setup, opts = (lambda: _bn_block_setup(*G["f4"])), behind_bn
    elif name == "pair_block":
        setup, opts = (lambda: _pair_block_setup(*G["s2"])), dict(direct=True)
    else:
        _, setup, opts = tg._cases(lib)[name]
    counts, undo = _counting(lib, count)
    tg.DISPATCH_RATIO[0] = 0.0
    early = ops._DEFER_DW.n_early
    try:
        tg._run_dispatch_case(_resolve_log(G, log), setup, _Env(), **opts)
    finally:
        undo()
    events = sorted({e[0] for e in ops.PROFILE.events})
    _MEMO["early"] = ops._DEFER_DW.n_early > early
    return tg.DISPATCH_RATIO[0], events, counts


# ---- one instrumented training step (BASELINE configs[1] at batch 4, the third step: the step's re-laid-out weights are served; weight
#      gradients on the step's own stream, as in the captured step bench.py times: the deferred launches exist only there) --------------------
def model_probe():
    if "probe" in _MEMO:
        return _MEMO["probe"]
    import torch
    import test_gpu_e2e as te
    from collections import Counter
    from hifihr_amd import ops
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import _forward_backward, train_step
    tables, args, model, ref, ex, ex_cpu = te._setup(4, graded=True)
    flat = FlatParams(model); opt = FusedAdam(flat, lr=1e-6)
    lossf = LossFunction()
    for _ in range(2):
        train_step(model, lossf, opt, ex, args)
    torch.cuda.synchronize()
    n_early = ops._DEFER_DW.n_early
    counts, undo = _counting(ops.get_lib(), ["wino4_dw_transform_multi", "wino_dw_transform_parts", "conv_halo_wgrad_reduce_multi", "wino_bn_input_transform",
                                             "bn_relu_maxpool_fwd", "bn_relu_maxpool_bwd_y", "bn_relu_maxpool_bwd", "conv3x3_c64_wino", "wino4_bwd_gemm_pair",
                                             "conv3x3_c64_bwd_pair_slabs", "conv3x3_c64_bwd_pair", "conv2d_fwd_bnstats_pair", "conv2d_bwd_data_pre_plus1x1",
                                             "conv2d_bwd_weight_plus1x1", "mano_full_fwd", "mano_joints_fwd", "mano_lbs_fwd"])
    ops.PROFILE.enable(); ops.PROFILE.conv_log.clear()
    try:
        with ops.prepared_weights(async_wgrad=False):
            loss, dic = _forward_backward(model, lossf, opt, ex, args, "FreiHand")
        opt.step()
        torch.cuda.synchronize()
    finally:
        ops.PROFILE.disable()
        undo()
    log = list(ops.PROFILE.conv_log); ops.PROFILE.conv_log.clear()
    out = {"events": dict(Counter(e[0] for e in ops.PROFILE.events)), "directions": dict(Counter(d for _, d in log)),
           "tiles": sorted({g[-1] for g, _ in log if g[0] == "wino"}), "calls": counts,
           "branches": sorted({k[1] for k in ops.side_branch._streams}),
           "n_early": ops._DEFER_DW.n_early > n_early}
    _MEMO["probe"] = out
    return out


# ---- witness queries ------------------------------------------------------------------------------------------------------------------------
def tn_skip_behaviour(lib, device, N, H, W, C, K, route):
    """hifihr_wino_wgrad_gemm_parts on a mosaic layer with FINITE NON-ZERO values planted in the rows of V and Y' behind the last computed
    tile: "valid" -- the slabs sum to the product over the computed rows alone (those rows are skipped); "all" -- over every row."""
    import torch
    import kernel_cases as kc
    with _route(route):
        T, Tr = lib.wino_tiles(N, H, W, 4), lib.wino_tiles_computed(N, H, W, 4)
        parts = lib.wino_wgrad_parts(N, H, W, C, K, 4)
        assert 0 < Tr < T and parts > 0, (T, Tr, parts)
        gen = torch.Generator().manual_seed(5)
        V, Y = torch.randn(36, T, C, generator=gen), torch.randn(36, T, K, generator=gen)
        dU = torch.zeros(parts, 36, K, C, device=device)
        lib.wino_wgrad_gemm_parts(V.to(device), Y.to(device), dU, N, H, W, C, K, parts, 4)
    got = dU.double().sum(0).cpu()
    full = lambda rows: torch.matmul(Y[:, :rows].double().transpose(1, 2), V[:, :rows].double())
    # (the kernel skips the k-steps -- 4 rows each -- that lie WHOLLY behind the last computed row: csrc/gemm.hip bgemm_tn_rows_kernel)
    fits = [name for name, rows in (("valid", min(T, (Tr + 3) // 4 * 4)), ("all", T)) if kc.layer_passes("gemm_tn", got, full(rows), rows)]
    assert len(fits) == 1, f"the slabs' sum is the product over neither / both row ranges: {fits}"
    return fits[0]


def launched(lib, kind, args, route):
    """emulator: the kernels one call launches (tests/hostsim logs them as the launch site spells them)"""
    import torch
    import kernel_cases as kc
    kc.launch_log(lib)
    with _route(route):
        if kind == "dw_parts":
            K, C = args
            lib.wino_dw_transform_parts(torch.zeros(1, 36, K, C), 1, torch.zeros(K, 3, 3, C), K, C, 4)
        elif kind == "render":               # (the renderer cases drain the log themselves, into RENDER_LAUNCHED)
            kc.RENDER_LAUNCHED.clear()
            kc.render_contract_case(lib, "cpu", tuple(args))
            return sorted(k.replace(" ", "") for k in kc.RENDER_LAUNCHED)
        else:
            raise ValueError(kind)
    return sorted({k.replace(" ", "") for k in kc.launch_log(lib)})


def profiled(lib, kind, args):
    """GPU: the kernel names torch's profiler reports for one call (None: the tracer gave nothing)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    import kernel_cases as kc

    def call():
        if kind == "dw_parts":
            K, C = args
            lib.wino_dw_transform_parts(torch.zeros(1, 36, K, C, device="cuda"), 1, torch.zeros(K, 3, 3, C, device="cuda"), K, C, 4)
        elif kind == "render":
            kc.render_contract_case(lib, "cuda", tuple(args))
        torch.cuda.synchronize()
    call()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "hifihr::" in e.name}
    return sorted(n.split("hifihr::", 1)[1].split("(")[0].replace(" ", "") for n in names) or None


def answer(lib, device, given, q):
    k = _key(q)
    if k in _MEMO:
        return _MEMO[k]
    kind = q[0]
    if kind == "conv_describe":
        a = lib.conv2d_describe(*q[1], q[2])
    elif kind == "bgemm_describe":
        with _route(q[3] if len(q) > 3 else None):
            a = lib.bgemm_describe(bool(q[1]), *q[2])
    elif kind == "pred":
        with _route(q[3] if len(q) > 3 else None):
            a = getattr(lib, q[1])(*q[2])
        a = a if isinstance(a, (bool, int, str)) else int(a)
    elif kind == "tn_skip":
        a = tn_skip_behaviour(lib, device, *q[1], q[2] if len(q) > 2 else None)
    elif kind == "launched":
        a = any(q[3] in name for name in launched(lib, q[1], q[2], q[4] if len(q) > 4 else None))
    elif kind == "profiled":
        names = profiled(lib, q[1], q[2])
        a = None if names is None else any(q[3] in name for name in names)
    elif kind == "conv_log":              # the case passed with exactly this log (asserted in _run_dispatch_case): the log is the answer
        run_dispatch(lib, given, q[1], q[2])
        a = sorted(f"{t}:{d}" for t, d in q[2])
    elif kind == "events":                # bracket names of the launches of a dispatch case
        _, ev, _ = run_dispatch(lib, given, q[1], q[2])
        a = q[3] in ev
    elif kind == "calls":                 # a C-ABI entry called during a dispatch case
        _, _, counts = run_dispatch(lib, given, q[1], q[2], count=(q[3],))
        a = counts[q[3]] > 0
    elif kind == "early":                 # ops._DEFER_DW flushed early (beside the stem's backward) during a dispatch case
        run_dispatch(lib, given, q[1], q[2])
        a = _MEMO["early"]
    elif kind == "model":
        a = model_probe()
        for part in q[1:]:
            a = a.get(part, 0) if isinstance(a, dict) else (part in a)
        a = a if isinstance(a, bool) else bool(a)
    else:
        raise ValueError(f"unknown witness query {q}")
    _MEMO[k] = a
    return a


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def run_case(lib, device, given, case):
    """-> (accepted, ratio)"""
    import kernel_cases as kc
    for log in _ratio_logs():
        log.clear()
    kind = case[0]
    if kind == "conv":
        geo = tuple(case[1])
        acc = kc.conv_contract_case(lib, device, *geo, seed=sum(geo))
        if device == "cpu":                # hifihr_conv2d_describe against the launch log, under the arm
            import test_hostsim_conv_contract as tc
            tc.test_describe_names_the_kernel_that_runs(lib, geo)
        doc = kc.conv_contract_expect(*geo)          # what the header documents, whatever the switches say (reported for the parent to compare)
        return dict({e: bool(v) for e, v in acc.items()}, documented={"fwd": doc["fwd"], "fwd_bnstats": doc["fwd"], "bwd_data": doc["dgrad"],
                                                                      "bwd_weight": doc["wgrad"]}), _worst_ratio()
    if kind == "pair":
        g = tuple(case[1])
        with _route(case[2] if len(case) > 2 else None):
            want = bool(lib.conv2d_fwd_bnstats_pair_supported(*g))
            acc = kc.conv_pair_contract_case(lib, device, *g, seed=sum(g))
        assert acc == want
        return bool(acc), _worst_ratio()
    if kind == "nt":
        M, N, K, batch, route, ws = case[1]
        with _route(route):
            acc, _ = kc.bgemm_nt_contract_case(lib, device, M, N, K, batch, ws_mode=ws, seed=(M + N + K + batch) % 1000)
        assert acc == kc.bgemm_nt_expect(M, N, K, batch)
        return bool(acc), _worst_ratio()
    if kind == "tn":
        M, N, T, batch, route = case[1]
        with _route(route):
            parts = kc.bgemm_tn_contract_case(lib, device, M, N, T, batch, seed=(M + N + T + batch) % 1000)
        assert (parts > 0) == kc.bgemm_tn_expect(M, N, T, batch)
        return parts > 0, _worst_ratio()
    if kind == "wino":
        g = tuple(case[1])
        with _route(case[2] if len(case) > 2 else None):
            if hasattr(lib, "_pair_ok"):
                lib._pair_ok.clear()
            acc = kc.wino_chain_contract_case(lib, device, *g, seed=sum(g))
        assert acc == kc.wino_contract_expect(*g)
        return bool(acc), _worst_ratio()
    if kind == "wino_bn":
        g = tuple(case[1])
        acc = kc.wino_bn_contract_case(lib, device, *g, seed=sum(map(int, g)))
        assert acc == kc.wino_bn_contract_expect(g[3], g[4])
        return bool(acc), _worst_ratio()
    if kind == "render":
        return bool(kc.render_contract_case(lib, device, tuple(case[1]))), _worst_ratio()
    if kind == "dispatch":
        ratio, _, _ = run_dispatch(lib, given, case[1], case[2])
        return True, ratio
    if kind == "model":
        import test_gpu_e2e as te
        te.ORACLE_RATIO.clear()
        {"losses": te.test_train_step_losses_match_oracle, "chain": te.test_backward_chain_matches_oracle_from_features}[case[1]]()
        return True, max(te.ORACLE_RATIO.values())
    raise ValueError(f"unknown case {case}")


def main():
    name, device = sys.argv[1], sys.argv[2]
    _DEVICE[0] = device
    given = json.loads(sys.argv[3]) if len(sys.argv) > 3 else None
    arm = sa.ARMS[name]
    for k, v in arm["env"].items():
        assert os.environ.get(k) == v, f"{name}: the parent did not set {k}={v}"
    for k in sa.ALL_SWITCHES - set(arm["env"]):
        assert k not in os.environ, f"{name}: {k} is set in this process's environment"
    import torch
    if device == "cpu":
        import kernel_cases as kc
        torch.set_num_threads(min(torch.get_num_threads(), 8))
        lib = kc.build_hostsim()
    else:
        assert torch.cuda.is_available()
        from hifihr_amd._lib import get_lib
        lib = get_lib()
    started = time.time() - T0
    out = {"arm": name, "device": device, "cases": []}
    if name == "default":
        out["witness"] = {n: [answer(lib, device, given, q) for q, _, _ in sa.witness(a, device)] for n, a in sa.ARMS.items() if n != "default"}
    else:
        out["witness"] = [None if a is None else answer(lib, device, given, q) for q, _, a in sa.witness(arm, device)]
    for case in sa.cases(arm, device):
        t = time.time()
        acc, ratio = run_case(lib, device, given, case)
        out["cases"].append({"case": case, "accepted": acc, "ratio": round(float(ratio), 4), "seconds": round(time.time() - t, 2)})
    out["geoms"] = {k: list(v) for k, v in _MEMO.get("geoms", {}).items()}
    out["max_ratio"] = max([c["ratio"] for c in out["cases"]] + [0.0])
    out["startup_seconds"], out["seconds"] = round(started, 2), round(time.time() - T0, 2)
    if device == "cuda":
        torch.cuda.synchronize()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
