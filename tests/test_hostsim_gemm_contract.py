"""The C ABI contract of the batched GEMMs (csrc/gemm.hip), hifihr_weight_transpose and the fully-connected entries (csrc/mlp.hip) on the
hostsim emulator, in the form of tests/test_hostsim_layer_contract.py: fixed shape lists on both sides of every tile, share and dispatch
boundary; an entry either refuses (HIFIHR_EINVAL, outputs untouched) or matches a float64 reference inside NaN / canary guard bands, twice
on the same workspace with identical bits (tests/kernel_cases.py, "The GEMM contract").  The routing switches (HIFIHR_GEMM_*) are set per
case so that the lists reach every kernel of the family on the emulator's 4 compute units; the coverage test at the end fails when an edit
stops reaching one, or when hifihr_bgemm_describe names another kernel than the one that ran.  The GPU half runs the same lists, and
a few larger shapes, in tests/test_gpu_gemm.py and tests/test_gpu_tail.py."""
import pytest
import torch

import kernel_cases as kc
from kernel_cases import (GEMM_ROUTES as ROUTES, LINEAR_GROUPS, LINEAR_SHAPES, NT_SHAPES, TN_SHAPES, TRANSPOSE_SHAPES, WINO_BN_GEOMS, WINO_GEOMS,
                          WINO_LAYERS, gemm_route as _route, wino_route)

_ids = lambda g: "x".join(map(str, g))

EXPECT_LAUNCHED = {f"bgemm_{d}_kernel<{bm},{bn}>" for d in ("nt", "tn") for bm in (64, 128) for bn in (64, 128)}
EXPECT_LAUNCHED |= {f"bgemm_ws_kernel<128,128,{tn},{w}>" for tn in ("false", "true") for w in (1, 2, 4)}
EXPECT_LAUNCHED |= {"bgemm_nt_sk_kernel<2>", "bgemm_nt_sk_kernel<4>", "bgemm_nt_rows_kernel<0>", "bgemm_nt_rows_kernel<1>", "bgemm_tn_rows_kernel",
                    "weight_transpose_kernel"}
# (the forward kernels' row block RB = 32 / 64 is a template argument of their launch site: the log spells it symbolically, the coverage test
# asks for batches on both sides of 32 instead)
EXPECT_LAUNCHED_LINEAR = {"linear_fwd_kernel<RB>", "linear_bwd_w_kernel", "linear_bwd_x_kernel", "linear_fwd_group_kernel<RB>",
                          "linear_bwd_w_group_kernel", "linear_bwd_x_group_kernel"}

EXPECT_LAUNCHED_WINO = {"wino_weight_transform_kernel", "wino_input_transform_kernel<false>", "wino_input_transform_kernel<true>", "wino_output_transform_kernel",
                        "wino_dy_transform_kernel", "wino_dw_transform_kernel", "wino_dw_transform_parts_kernel", "weight_prep_kernel",
                        "wino4_weight_transform_kernel", "wino4_output_transform_kernel<false>", "wino4_output_transform_kernel<true>",
                        "wino4_dy_transform_kernel<false>", "wino4_dy_transform_kernel<true>", "wino4_dw_transform_multi_kernel",
                        "wino4_dw_transform_parts_kernel", "wino4_dw_transform_parts_wide_kernel"}
EXPECT_LAUNCHED_WINO |= {f"wino4_input_transform_kernel<{a},{b}>" for a in ("false", "true") for b in ("false", "true")}

LAUNCHED = {}           # (family, shape) -> set of kernels the case launched
_DONE = {}


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.fixture(scope="module")
def tally():
    yield None
    kc.layer_contract_report("GEMM and fully-connected entries on the emulator", ("bgemm", "weight_transpose", "weight_prep", "linear", "wino"))


def nt_kernel_expected(lib, g):
    """The kernel an accepted NT case must run on: what hifihr_bgemm_describe names -- except the stream-K plan without (enough of) its
    workspace, which include/hifihr.h sends to one workgroup per tile (the wave-specialised kernel with the same loader waves)."""
    M, N, K, batch, route, ws = g
    with _route(route):
        name = lib.bgemm_describe(False, M, N, K, batch).replace(" ", "")
    if name.startswith("bgemm_nt_sk_kernel") and ws != "full":
        return f"bgemm_ws_kernel<128,128,false,{ROUTES[route]['HIFIHR_GEMM_WS']}>"
    return name


def _case(lib, family, g):
    if family == "nt":
        return kc.bgemm_nt_contract_case(lib, "cpu", *g[:4], ws_mode=g[5], seed=sum(g[:4]) % 1000)
    if family == "tn":
        return kc.bgemm_tn_contract_case(lib, "cpu", *g[:4], seed=sum(g[:4]) % 1000)
    if family == "wino":
        return kc.wino_chain_contract_case(lib, "cpu", *g, seed=sum(g))
    if family == "wino_bn":
        return kc.wino_bn_contract_case(lib, "cpu", *g, seed=sum(map(int, g)))
    if family == "linear":
        return kc.linear_contract_case(lib, "cpu", *g, seed=sum(map(int, g)))
    if family == "group":
        return kc.linear_group_contract_case(lib, "cpu", list(g), seed=len(g))
    return kc.weight_transpose_contract_case(lib, "cpu", *g, seed=sum(g))


def _run(lib, family, g):
    """One shape, once per session, under its route; the kernels it launched go to LAUNCHED."""
    key = (family, g)
    if key not in _DONE:
        kc.launch_log(lib)
        with _route(g[4] if family in ("nt", "tn") else kc.wino_route(g) if family == "wino" else "default"):
            try:
                _DONE[key] = _case(lib, family, g)
            finally:
                LAUNCHED[key] = {k.replace(" ", "") for k in kc.launch_log(lib)}
    return _DONE[key]


@pytest.mark.parametrize("geo", NT_SHAPES, ids=_ids)
def test_bgemm_nt_on_every_shape(hostsim_lib, tally, geo):
    accepted, nb = _run(hostsim_lib, "nt", geo)
    assert accepted == kc.bgemm_nt_expect(*geo[:4])
    if accepted:
        assert LAUNCHED[("nt", geo)] == {nt_kernel_expected(hostsim_lib, geo)}, "hifihr_bgemm_describe names another kernel than the one that ran"
    else:
        assert not LAUNCHED[("nt", geo)], "a refused call launched a kernel"


@pytest.mark.parametrize("geo", TN_SHAPES, ids=_ids)
def test_bgemm_tn_on_every_shape(hostsim_lib, tally, geo):
    parts = _run(hostsim_lib, "tn", geo)
    assert (parts > 0) == kc.bgemm_tn_expect(*geo[:4])
    if parts:
        with _route(geo[4]):
            name = hostsim_lib.bgemm_describe(True, *geo[:4]).replace(" ", "")
        assert LAUNCHED[("tn", geo)] == {name}, "hifihr_bgemm_describe names another kernel than the one that ran"
    else:
        assert not LAUNCHED[("tn", geo)], "a refused call launched a kernel"


@pytest.mark.parametrize("geo", TRANSPOSE_SHAPES, ids=_ids)
def test_weight_transpose_on_every_shape(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "transpose", geo) == (min(geo) > 0)



@pytest.mark.parametrize("geo", LINEAR_SHAPES, ids=_ids)
def test_linear_on_every_shape(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "linear", geo) == kc.linear_contract_expect(*geo[:5])


@pytest.mark.parametrize("members", LINEAR_GROUPS, ids=lambda ms: f"{len(ms)}x" + "_".join(map(str, ms[0])))
def test_linear_groups(hostsim_lib, tally, members):
    assert _run(hostsim_lib, "group", tuple(members)) == (len(members) <= kc.LINEAR_MAX_GROUP and all(m[3] < 2 for m in members))


def test_linear_batch_norm_on_one_row(hostsim_lib):
    """B = 1 (nn.BatchNorm1d raises): variance 0, save_invstd = 1 / sqrt(eps), y = act(beta), the running variance takes the biased value 0."""
    lib, I, O, eps, mom = hostsim_lib, 36, 20, 1e-3, 0.25
    inp = kc.linear_contract_inputs(1, I, O, 3)
    y, z, sm, si = (torch.empty(1, O), torch.empty(1, O), torch.empty(O), torch.empty(O))
    rm, rv = torch.zeros(O), torch.ones(O)
    lib.linear_fwd(inp["x"], inp["w"], inp["b"], 0, y, (inp["gamma"], inp["beta"], eps, mom, rm, rv, z, sm, si))
    assert torch.equal(sm, z[0])
    assert float((si - eps ** -0.5).abs().max()) <= 4e-7 * eps ** -0.5
    # y = z sc + sh with sc = gamma / sqrt(eps), sh = beta - mean sc: the two terms cancel to the rounding of their size
    assert float((y[0] - inp["beta"]).abs().max()) <= 4 * 6e-8 * float((z.abs() * inp["gamma"].abs()).max()) * eps ** -0.5
    assert float((rm - mom * z[0]).abs().max()) <= 1e-6 and float((rv - (1 - mom)).abs().max()) <= 1e-6


@pytest.mark.parametrize("geo", WINO_GEOMS, ids=_ids)
def test_every_winograd_transform_on_every_geometry(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "wino", geo) == kc.wino_contract_expect(*geo)


@pytest.mark.parametrize("geo", WINO_BN_GEOMS, ids=_ids)
def test_every_winograd_batch_norm_fusion_on_every_geometry(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "wino_bn", geo) == kc.wino_bn_contract_expect(geo[3], geo[4])


def test_winograd_products_refuse_operands_beyond_32_bit_offsets(hostsim_lib):
    """T C = 2^31 elements per position: the predicate path alone (nothing large is allocated) -- HIFIHR_EINVAL, like hifihr_bgemm_nt."""
    lib, G = hostsim_lib, kc.Guards("cpu")
    V, U, M, dU = G.inp(torch.zeros(36, 1, 64)), G.inp(torch.zeros(36, 64, 64)), G.out(36, 1, 64), G.out(2, 36, 64, 64)
    for m, N in ((4, 2 ** 25), (2, 2 ** 23)):
        kc._refuses("wino_gemm", lambda: lib.wino_gemm(V, U, M, N, 4, 4, 64, 64, m=m), G, f"wino_gemm, m = {m}, N = {N}")
    parts = lib.wino_wgrad_parts(2 ** 25, 4, 4, 64, 64, 4)
    kc._refuses("wino4_bwd_gemm_pair", lambda: lib.wino4_bwd_gemm_pair(V, U, M, V, V, dU, 2 ** 25, 4, 4, 64, 64, max(parts, 1)), G, "pair launch")


def test_detection_the_winograd_comparator_notices_one_missing_tap():
    """No kernel involved: float64 conv2d without the filter's centre tap (y, dx) / without one output pixel's contribution (dw) must fail the
    comparator on every accepted geometry."""
    missed = []
    for g in WINO_GEOMS:
        if kc.wino_contract_expect(*g):
            inp = kc.wino_contract_inputs(*g[:5], sum(g))
            ref, bad = kc.wino_contract_ref(inp), kc.wino_contract_ref(inp, drop_tap=True)
            kinds = {"y": "wino4_fwd", "dx": "wino4_fwd", "dw": "wino4_wgrad"} if g[5] == 4 else {"y": "wino_fwd", "dx": "wino_fwd", "dw": "wino_wgrad"}
            missed += [(g, n) for n in ("y", "dx") if kc.layer_passes(kinds[n], bad[n][1], ref[n][1], ref[n][0])]
            bad = kc.wino_contract_ref(inp, drop_pixel=True)
            missed += [(g, "dw")] if kc.layer_passes(kinds["dw"], bad["dw"][1], ref["dw"][1], ref["dw"][0]) else []
    assert not missed, missed


def test_no_winograd_bound_is_looser_than_the_case_it_replaces():
    """wino_case: 3e-5 (F(2x2)) / 5e-5 (F(4x4)) of max|ref| for y and dx, 1e-4 for dw."""
    legacy = {"wino_fwd": 3e-5, "wino4_fwd": 5e-5, "wino_wgrad": 1e-4, "wino4_wgrad": 1e-4}
    assert set(legacy) == set(kc.WINO_CONTRACT_KINDS)
    for kind, tol in legacy.items():
        c, cap = kc.LAYER_CONTRACT_C[kind]
        assert 0 < c <= cap <= tol and kind not in kc.LAYER_CONTRACT_FLOOR
        assert kc.layer_bound(kind, torch.ones(3, dtype=torch.float64), 10 ** 12) <= tol


def test_the_integer_family_is_exact_in_fp32():
    """No kernel involved: |a| |b| L < 2^24 for every reduction length of the lists, and the operands do differ from row to row and k to k."""
    for L in {g[2] for g in NT_SHAPES + TN_SHAPES if g[2] > 0 and g[2] < 2 ** 20}:
        assert kc.gemm_ints_exact(L), L
    a, b = kc.gemm_operands("ints", 2, 65, 33, 96, 7, False)
    assert float(a.abs().max()) == kc.GEMM_INT_A and float(b.abs().max()) == kc.GEMM_INT_B
    assert len({tuple(r.tolist()) for r in a[0]}) == min(65, 2 * kc.GEMM_INT_A + 1) and len({tuple(c.tolist()) for c in a[0].t()}) == min(96, 2 * kc.GEMM_INT_A + 1)
    assert not torch.equal(a[0], a[1]) and not torch.equal(b[0], b[1])
    prods = a[0, 0] * b[0, 0]
    assert len({(float(x), float(y)) for x, y in zip(a[0, 0], b[0, 0])}) == 96, "a k-step's pair of operands repeats inside a row"
    assert prods.abs().sum() > 0


def test_detection_the_comparator_notices_one_missing_k_step():
    """No kernel involved: a float64 product with ONE k-step (NT) / one row t (TN) removed must fail the comparator on every accepted shape of
    the lists, or the bound would not notice a kernel that skips one."""
    missed = []
    for g in NT_SHAPES:
        M, N, K, batch = g[:4]
        if kc.bgemm_nt_expect(M, N, K, batch):
            a, b = kc.gemm_operands("randn", batch, M, N, K, sum(g[:4]) % 1000, False)
            ref = torch.matmul(a.double(), b.double().transpose(1, 2))
            bad = torch.matmul(a[:, :, :-1].double(), b[:, :, :-1].double().transpose(1, 2))
            missed += [("nt", g)] if kc.layer_passes("gemm_nt", bad, ref, K) else []
    for g in TN_SHAPES:
        M, N, T, batch = g[:4]
        if kc.bgemm_tn_expect(M, N, T, batch):
            a, b = kc.gemm_operands("randn", batch, M, N, T, sum(g[:4]) % 1000, True)
            ref = torch.matmul(a.double().transpose(1, 2), b.double())
            bad = torch.matmul(a[:, :-1].double().transpose(1, 2), b[:, :-1].double())
            missed += [("tn", g)] if kc.layer_passes("gemm_tn", bad, ref, T) else []
    # fully connected: one input feature removed from the reductions over I (y, z), one batch row from those over B (dW, db, dgamma, dbeta)
    fails = lambda ref, bad, n: not kc.layer_passes(ref[n][0], bad[n][2], ref[n][2], ref[n][1], ref[n][3] if len(ref[n]) > 3 else 0.0)
    for g in LINEAR_SHAPES:
        B, I, O, act, bn = g[:5]
        if kc.linear_contract_expect(B, I, O, act, bn):
            inp = kc.linear_contract_inputs(B, I, O, sum(map(int, g)))
            ref = kc.linear_contract_ref(inp, act, bn)
            mask = (ref["y"][2] > 0) if act == 1 else None
            worst = int(inp["x"].abs().amax(0).argmax())
            bad = kc.linear_contract_ref(inp, 0, False, drop_k=worst)
            missed += [("linear", g, "z")] if not fails(kc.linear_contract_ref(inp, 0, False), bad, "z") else []
            row = int(inp["gy"].abs().amax(1).argmax())
            bad = kc.linear_contract_ref(inp, act, bn, mask=mask, drop_row=row)
            names = ("dW", "db") if not bn else (("dW", "dbeta") if B > 2 else ())      # (B <= 2 under batch-norm: dz vanishes identically, rows cancel)
            if act == 1 and not bool(mask[row].any()):
                names = ()
            missed += [("linear", g, n) for n in names if not fails(ref, bad, n)]
            # dx without one output feature's term (the reduction over O)
            col = int((inp["gy"].abs().amax(0) * inp["w"].abs().amax(1)).argmax()) if not bn else 0
            if O > 1 and not bn and not (act == 1 and not bool(mask[:, col].any())):
                missed += [("linear", g, "dx")] if not fails(ref, kc.linear_contract_ref(inp, act, bn, mask=mask, drop_o=col), "dx") else []
            if bn:
                # y behind batch-norm without one input feature; dgamma without one batch row; the statistics of B - 1 rows (B = 1: none to drop)
                if B > 1:                                   # (B = 1: y = beta whatever the input)
                    missed += [("linear", g, "y")] if not fails(kc.linear_contract_ref(inp, 0, True), kc.linear_contract_ref(inp, 0, True, drop_k=worst), "y") else []
                if B > 2:
                    missed += [("linear", g, "dgamma")] if not fails(ref, bad, "dgamma") else []
                if B > 1:
                    less = kc.linear_contract_ref({k: (v[:-1] if k in ("x", "gy") else v) for k, v in inp.items()}, 0, True)
                    full = kc.linear_contract_ref(inp, 0, True)
                    missed += [("linear", g, n) for n in ("save_mean", "save_invstd", "running_mean", "running_var") if not fails(full, less, n)]
    assert not missed, f"the comparator accepts a product with one k-step removed: {missed}"


def test_no_gemm_bound_is_looser_than_the_case_it_replaces():
    """bgemm_case / bgemm_tn_case hold err <= 2e-6 sqrt(L) max|ref| + 1e-6: c <= 2e-6 keeps c sqrt(L) below that at every L, and no floor is added."""
    for kind in ("gemm_nt", "gemm_tn"):
        c, cap = kc.LAYER_CONTRACT_C[kind]
        assert 0 < c <= cap <= 2e-6 and kind not in kc.LAYER_CONTRACT_FLOOR
        ref = torch.ones(3, dtype=torch.float64)
        for L in (1, 32, 777, 10 ** 6):
            assert kc.layer_bound(kind, ref, L) <= 2e-6 * L ** 0.5


def test_no_linear_bound_is_looser_than_the_case_it_replaces():
    """linear_case: 3e-5 max(1, max|y|) forward, rtol 1e-5 on the running mean, 2e-4 on every gradient."""
    legacy = {"lin_y": 3e-5, "lin_bn_y": 3e-5, "lin_stat": 1e-5, "lin_dw": 2e-4, "lin_dx": 2e-4}
    assert set(legacy) | {"gemm_nt", "gemm_tn"} == set(kc.GEMM_CONTRACT_KINDS)
    for kind, tol in legacy.items():
        c, cap = kc.LAYER_CONTRACT_C[kind]
        assert 0 < c <= cap <= tol and kind not in kc.LAYER_CONTRACT_FLOOR
        assert kc.layer_bound(kind, torch.ones(3, dtype=torch.float64), 10 ** 12) <= tol


def test_the_gemm_lists_reach_every_kernel_and_both_answers(hostsim_lib):
    """A shape edit that stops reaching a kernel, a schedule or an accept / refuse rule fails here."""
    lib = hostsim_lib
    for family, shapes in (("nt", NT_SHAPES), ("tn", TN_SHAPES), ("transpose", TRANSPOSE_SHAPES), ("linear", LINEAR_SHAPES),
                           ("group", [tuple(ms) for ms in LINEAR_GROUPS]), ("wino", WINO_GEOMS), ("wino_bn", WINO_BN_GEOMS)):      # (whatever a -k selection left out runs now)
        for g in shapes:
            _run(lib, family, g)
    ran = set().union(*LAUNCHED.values())
    assert EXPECT_LAUNCHED <= ran, f"no shape reaches {sorted(EXPECT_LAUNCHED - ran)}"
    # every kernel is reached by a case that is the only ... at least one; and the schedules inside the row-share kernels
    tn_rows = [g for g in TN_SHAPES if LAUNCHED[("tn", g)] == {"bgemm_tn_rows_kernel"}]
    assert {_DONE[("tn", g)] for g in tn_rows} >= {1, 2}, "bgemm_tn_rows_kernel: single slab and T-split"
    assert any(g[4] == "cus16" for g in tn_rows), "the XCD-coherent schedule"
    per_tile_fallback = [g for g in NT_SHAPES if g[5] != "full" and _DONE[("nt", g)][1] > 0]
    assert {g[5] for g in per_tile_fallback} == {"short", "none"}, "a stream-K shape without (enough of) its workspace"
    assert all(LAUNCHED[("nt", g)] == {f"bgemm_ws_kernel<128,128,false,{ROUTES[g[4]]['HIFIHR_GEMM_WS']}>"} for g in per_tile_fallback)
    sk = [g for g in NT_SHAPES if g[5] == "full" and _DONE[("nt", g)][1] > 0]
    assert {next(iter(LAUNCHED[("nt", g)])) for g in sk} == {"bgemm_nt_sk_kernel<2>", "bgemm_nt_sk_kernel<4>"}
    # both outcomes of every rule
    assert {kc.bgemm_nt_expect(*g[:4]) for g in NT_SHAPES} == {True, False} and {kc.bgemm_tn_expect(*g[:4]) for g in TN_SHAPES} == {True, False}
    refused = [g[:4] for g in NT_SHAPES if not kc.bgemm_nt_expect(*g[:4])]
    assert {g[2] for g in refused} >= {0, 16, 48} and {g[1] for g in refused} >= {0, 32, 96, 2 ** 26} and {g[0] for g in refused} >= {0, 2 ** 26}
    assert any(g[3] == 0 for g in refused)
    assert EXPECT_LAUNCHED_LINEAR <= ran, f"no shape reaches {sorted(EXPECT_LAUNCHED_LINEAR - ran)}"
    lin = [g for g in LINEAR_SHAPES if kc.linear_contract_expect(*g[:5])]
    assert {g[0] for g in lin} == {1, 2, 31, 32, 33, 63, 64, 65, 70, 129} and {g[1] for g in lin} == {1, 3, 4, 31, 32, 33, 36, 72, 128, 1038, 1100}
    assert {g[2] for g in lin} == {1, 3, 20, 33, 48, 300} and {g[3] for g in lin} == {0, 1, 2, 3}
    assert {g[0] for g in lin if g[4]} == {1, 2, 32, 64} and {g[5] for g in lin if g[4]} == {True, False} and {g[6] for g in lin} == {True, False}
    assert {kc.linear_contract_expect(*g[:5]) for g in LINEAR_SHAPES} == {True, False} and {_DONE[("group", tuple(ms))] for ms in LINEAR_GROUPS} == {True, False}
    assert {len(ms) for ms in LINEAR_GROUPS} >= {1, 2, 3, 6, 7}
    assert {max(m[0] for m in ms) <= 32 for ms in LINEAR_GROUPS if _DONE[("group", tuple(ms))]} == {True, False}, "groups on 32- and on 64-row blocks"
    # Winograd: both tile edges on every layer, mosaic tile counts and their plain neighbours, images below one tile, every refused m
    acc = [g for g in WINO_GEOMS if kc.wino_contract_expect(*g)]
    assert {g[:5] for g in acc if g[5] == 2} == {g[:5] for g in acc if g[5] == 4} == set(WINO_LAYERS)
    assert {g[1] for g in acc} == {1, 2, 3, 4, 5, 6, 7, 9, 13, 14} == {g[2] for g in acc} and {g[0] for g in acc} == {1, 2, 3, 16, 17, 32}
    assert {g[3] for g in acc} >= {4, 8, 24, 32, 64, 100, 128} and {g[4] for g in acc} >= {4, 8, 24, 32, 64, 100, 128}
    mosaic = [g for g in acc if g[5] == 4 and lib.wino_tiles_computed(*g[:3], 4) < lib.wino_tiles(*g[:3], 4)]
    assert {g[1] % 4 for g in mosaic} == {1, 2} and {g[0] for g in mosaic} == {16, 32}, "mosaic tile counts with padding rows behind them"
    assert {g[5] for g in WINO_GEOMS if not kc.wino_contract_expect(*g)} >= {0, 3, 8, 2, 4}
    for e in ("wino_weight_transform", "wino_input_transform", "wino_output_transform", "wino_output_transform_act", "wino_dy_transform",
              "wino_input_dy_transform", "wino_dw_transform_parts", "wino_dw_transform", "wino4_dw_transform_multi", "wino_gemm",
              "wino_wgrad_gemm_parts", "wino4_bwd_gemm_pair", "weight_prep", "wino_bn_input_transform", "wino_output_transform_bnred",
              "wino_bn_bwd_dual_transform"):
        row = kc.LAYER_CONTRACT_LOG[e]
        assert row[1] > 0 and (row[0] > 0 or e in ("wino_weight_transform", "wino_input_transform", "wino_dy_transform")), \
            f"{e}: accepted {row[0]}, refused {row[1]} calls"      # (those three are accepted inside every chain: their results are what it compares)
    # every kernel of csrc/wino.hip, wino4.hip and wino4_bn.hip (the batch-norm fusions by name: their template arguments are logged symbolically)
    assert EXPECT_LAUNCHED_WINO <= ran, f"no geometry reaches {sorted(EXPECT_LAUNCHED_WINO - ran)}"
    for prefix in ("wino4_bn_input_transform_kernel<", "wino4_output_transform_bnred_kernel<", "wino4_bn_bwd_dual_transform_kernel<"):
        assert any(k.startswith(prefix) for k in ran), prefix
    # the pair launch really is one launch somewhere, and its predicate gives both answers
    assert any("bgemm_nt_tn_pair_kernel" in LAUNCHED[("wino", g)] for g in acc), "no geometry takes the two backward products as one launch"
    lib._pair_ok.clear()
    answers = set()
    for g in acc:
        if g[5] == 4:
            with _route(kc.wino_route(g)):
                lib._pair_ok.pop(g[:5], None)
                answers.add(lib.wino4_bwd_gemm_pair_supported(*g[:5]))
    assert answers == {True, False}
    lib._pair_ok.clear()
    # the batch-norm fusions: both limits of C, residual and addend in all four combinations, refused C and m
    bn_acc = [g for g in WINO_BN_GEOMS if kc.wino_bn_contract_expect(g[3], g[4])]
    assert {g[3] for g in bn_acc} >= {4, 512} and {(g[5], g[6]) for g in bn_acc} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {g[3] for g in WINO_BN_GEOMS if g not in bn_acc} >= {516, 6, 1024} and {g[4] for g in WINO_BN_GEOMS if g not in bn_acc} >= {0, 2, 4}
    for e in ("bgemm_nt", "bgemm_tn", "weight_transpose", "linear_fwd", "linear_bwd", "linear_fwd_group", "linear_bwd_group"):
        row = kc.LAYER_CONTRACT_LOG[e]
        assert row[0] > 0 and row[1] > 0, f"{e}: accepted {row[0]}, refused {row[1]} calls"
    # the classes the lists exist for
    acc = [g for g in NT_SHAPES if kc.bgemm_nt_expect(*g[:4])]
    assert {g[0] for g in acc} == {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300} and {g[1] for g in acc} == {64, 128, 192, 256, 576}
    assert {g[2] for g in acc} == {32, 64, 96, 128, 160, 512} and {g[3] for g in acc} == {1, 2, 5, 36}
    acc = [g for g in TN_SHAPES if kc.bgemm_tn_expect(*g[:4])]
    assert {g[0] for g in acc} == {64, 128, 192, 256, 320} == {g[1] for g in acc}
    assert {g[2] for g in acc} == {1, 4, 31, 32, 33, 63, 64, 65, 96, 256, 777} and {g[3] for g in acc} == {1, 2, 16, 36}
