"""The layer kernels' C ABI contract on the hostsim emulator: every batch-norm, pooling, depthwise, squeeze-excite and SSIM entry point on
fixed geometry lists -- channel counts on both sides of every dispatch threshold, row counts around the rows-per-workgroup of the grids,
images smaller than the filter / window, ragged tiles.  An entry either refuses a geometry (HIFIHR_EINVAL, outputs untouched) or matches a
float64 reference inside guard bands (tests/kernel_cases.py, "The layer contract").  The GPU half runs the same lists, and larger sizes, in
tests/test_gpu_conv.py (batch-norm, depthwise) and tests/test_gpu_tail.py (pooling, squeeze-excite, SSIM)."""
import pytest
import torch

import kernel_cases as kc

# ---- batch-norm: (M, C, act, residual, y_given, running) ---------------------------------------------------------------------------------
# rows per workgroup of bn_grid = 256 / (C / 4): 128 at C = 8, 16 at C = 64, 4 at C = 256; M % 4 in all four classes (kBnUnroll)
BN_GEOMS = [
    (1, 4, 0, False, True, True), (2, 8, 1, False, True, True), (3, 12, 1, True, True, True), (5, 64, 2, False, True, True),
    (15, 64, 1, False, False, True), (16, 64, 0, True, True, False), (17, 64, 1, True, True, True), (18, 64, 2, False, True, False),
    (127, 8, 1, False, False, True), (128, 8, 2, False, True, True), (129, 8, 0, False, True, True),
    (3, 256, 1, False, True, True), (4, 256, 2, False, True, True), (5, 256, 0, True, True, True), (6, 260, 1, True, True, True),
    (7, 512, 1, False, False, True), (300, 64, 1, False, False, False),
    (9, 516, 1, True, True, True), (300, 516, 2, False, True, True), (2, 516, 1, False, False, True),
    (5, 1024, 1, True, True, True), (1, 1024, 2, False, True, True),
    (2, 1028, 1, True, True, True), (9, 1028, 2, False, True, True), (3, 1028, 1, False, False, False),
    (3, 2304, 2, False, True, True), (5, 2304, 1, True, True, True), (2, 4096, 1, True, True, True), (1, 4096, 0, False, True, True),
    (5, 64, 2, True, True, True),                                  # swish with a residual: refused
    (5, 0, 0, False, True, True), (5, 2, 1, False, True, True), (5, 6, 0, False, True, True), (3, 4100, 1, False, True, True),      # refused C
]
# the fused stem: (N, H, W, C); channel 1 has |gamma| < 1e-3, channel 2 a negative gamma (kc.bn_stem_contract_inputs)
BN_STEM_GEOMS = [(1, 2, 2, 4), (1, 3, 2, 12), (2, 5, 7, 64), (1, 8, 6, 8), (3, 4, 9, 260), (1, 7, 7, 512),
                 (1, 6, 6, 516), (1, 1, 6, 64), (1, 6, 1, 64), (1, 6, 6, 6)]                                 # refused

# ---- pooling: (N, H, W, C, k, s, p, mode) ------------------------------------------------------------------------------------------------
_POOL_SIZES = [(1, 1), (1, 4), (4, 1), (2, 2), (2, 3), (3, 2), (3, 3), (4, 5), (5, 4), (7, 8), (8, 7), (5, 5), (7, 7), (8, 8)]
POOL_GEOMS = [(1 + (i + j) % 2, H, W, (4, 8, 260)[(i + j) % 3], *ksp, ("random", "ties", "special")[(i + 2 * j) % 3])
              for j, ksp in enumerate(kc.POOL_KSP + ((3, 2, 0),)) for i, (H, W) in enumerate(_POOL_SIZES)]
POOL_GEOMS += [(1, 5, 5, 8, 2, 1, 0, "random"), (1, 5, 5, 8, 5, 1, 2, "random"), (1, 5, 5, 8, 3, 3, 1, "random"),        # refused (k, s, p)
               (1, 4, 4, 6, 3, 2, 1, "random"), (1, 4, 4, 6, 3, 2, 0, "random")]                                      # refused C
# the flat forward accepted these and wrote OH = (1 - 2) / 2 + 1 = 1 rows where the output has none
POOL_FLAT_REGRESSIONS = [g for g in POOL_GEOMS if g[4:7] == (2, 2, 0) and 1 in (g[1], g[2])]
# mmpool: (B, HW, C, p, ties)
MMPOOL_GEOMS = [(2, 1, 4, 0.3, False), (1, 2, 132, -1.2, False), (3, 255, 4, -30.0, True), (2, 256, 132, 30.0, False),
                (1, 257, 1028, 0.3, True), (2, 49, 1028, -1.2, False), (2, 7, 6, 0.3, False)]

# ---- depthwise: (N, H, W, C, K, stride, pad_top, pad_left, OH, OW) -----------------------------------------------------------------------
_DW_SIZES = [(1, 1), (1, 9), (2, 3), (3, 2), (4, 5), (5, 4), (7, 9), (9, 7), (12, 12), (2, 12), (12, 1), (3, 3)]
_DW_C = [4, 8, 60, 64, 68, 132]
DW_GEOMS = []
for _ki, (_K, _S) in enumerate(((3, 1), (3, 2), (5, 1), (5, 2))):
    DW_GEOMS += [kc.dw_same_geom(1 + 2 * ((_i + _ki) % 2), _H, _W, _DW_C[(_i + _ki) % 6], _K, _S) for _i, (_H, _W) in enumerate(_DW_SIZES)]
    for _pi, _pad in enumerate((0, _K // 2, _K - 1)):                # explicit symmetric pads; pad 0 on an input below the filter has OH <= 0
        DW_GEOMS += [kc.dw_pad_geom(1, _H, _W, _DW_C[(_pi + _ki + _j) % 6], _K, _S, _pad) for _j, (_H, _W) in enumerate(((7, 9), (5, 4), (2, 3), (8, 8)))]
DW_GEOMS += [
    (1, 8, 8, 8, 3, 2, 0, 0, 3, 3),          # stride 2, H + pads - K odd: the implied bottom pad is -1, the row a floor division leaves unread
    (1, 7, 7, 8, 3, 1, 1, 1, 5, 7),          # a crop (bottom pad -3 at stride 1): refused
    (1, 7, 7, 8, 3, 1, 1, 1, 7, 9),          # windows in the padding alone (right pad 3 > K - 1): refused
    (1, 7, 7, 8, 3, 1, 3, 1, 9, 7),          # pad_top = K: refused
    (1, 7, 7, 8, 3, 1, -1, 1, 5, 7),         # negative pad: refused
    (1, 7, 7, 8, 3, 1, 1, 1, 0, 7), (1, 7, 7, 8, 3, 1, 1, 1, 7, -1),      # OH / OW <= 0: refused
    (1, 7, 7, 8, 1, 1, 0, 0, 7, 7), (1, 7, 7, 8, 4, 1, 1, 1, 6, 6), (1, 9, 9, 8, 7, 1, 3, 3, 9, 9),      # K 1, 4, 7: refused
    (1, 7, 7, 8, 3, 3, 1, 1, 3, 3),          # stride 3: refused
    (1, 7, 7, 6, 3, 1, 1, 1, 7, 7),          # C = 6: refused
]

# ---- squeeze-excite: (B, HW, C, SQ) ------------------------------------------------------------------------------------------------------
SE_GEOMS = [(1, 1, 4, 1), (2, 2, 40, 6), (48, 49, 132, 34), (49, 2, 2304, 96), (49, 1, 4096, 256), (96, 2, 40, 6), (97, 196, 40, 6),
            (2, 196, 132, 96),
            (3, 49, 4100, 6),                # the plain entries take it, the fused MLP pair (C <= 4096) refuses
            (2, 2, 40, 257), (2, 2, 6, 4)]   # SQ = 257: the MLP pair refuses; C = 6: all refuse
# drop-connect: (B, per_sample, keep, with_skip)
DROP_GEOMS = [(3, 8, 1.0, True), (4, 260, 0.8, True), (2, 64, 0.8, False), (1, 4, 0.8, True),
              (2, 8, 0.0, True), (2, 8, -0.5, False), (2, 6, 0.8, True)]                  # refused

# ---- SSIM: (planes, H, W, inputs) ----------------------------------------------------------------------------------------------------------
SSIM_GEOMS = [(1, 1, 1, "random"), (6, 3, 4, "identical"), (1, 11, 36, "random"), (6, 10, 36, "constants"), (1, 33, 32, "masked"),
              (6, 32, 32, "random"), (1, 64, 100, "random"), (1, 70, 65, "masked"), (1, 9, 1, "random"), (1, 1, 12, "constants"),
              (1, 37, 21, "identical"), (1, 32, 64, "identical")]
SSIM_FINISH_COUNTS = [1, 255, 256, 257, 1023, 1024, 1025, 4704]

_ids = lambda g: "x".join(map(str, g))

# Every instantiation the launchers can select.  (bn_act_fwd_kernel<false, kMaxNG> and bn_bwd_apply_kernel<false, kMaxNG> no longer exist:
# the fused forms run at C <= 512 only, where one channel group per thread always suffices.)
EXPECT_LAUNCHED = {
    "bn_stats_kernel", "bn_act_fwd_kernel<false,1>", "bn_act_fwd_kernel<true,1>", "bn_act_fwd_kernel<true,kMaxNG>", "bn_bwd_reduce_kernel<1>",
    "bn_bwd_reduce_kernel<kMaxNG>", "bn_bwd_apply_kernel<false,1>", "bn_bwd_apply_kernel<true,1>", "bn_bwd_apply_kernel<true,kMaxNG>",
    "bn_finalize_fwd_kernel", "bn_finalize_bwd_kernel", "bn_relu_pool_fwd_kernel", "bn_pool_bwd_reduce_kernel", "bn_pool_bwd_reduce_y_kernel",
    "bn_pool_bwd_apply_kernel", "mmpool_fwd_kernel", "mmpool_bwd_kernel", "ssim_fwd_kernel<true>", "ssim_fwd_kernel<false>",
    "ssim_bwd_kernel<true>", "ssim_bwd_kernel<false>", "ssim_finish_kernel", "se_reduce_kernel<0>", "se_reduce_kernel<1>", "se_scale_kernel",
    "se_mlp_fwd_kernel", "se_mlp_bwd_x_kernel", "se_mlp_bwd_w_kernel", "drop_connect_add_kernel"}
EXPECT_LAUNCHED |= {f"maxpool_{d}_kernel<{k},{s},{p}{flat}>" for d in ("fwd", "bwd") for k, s, p in kc.POOL_KSP for flat in ("", ",true")}
EXPECT_LAUNCHED |= {f"dwconv_{d}_kernel<{K},{S},{pre}>" for d in ("fwd", "bwd_weight") for K in (3, 5) for S in (1, 2) for pre in ("true", "false")}
EXPECT_LAUNCHED |= {f"dwconv_bwd_data_kernel<{K},{S}>" for K in (3, 5) for S in (1, 2)}

LAUNCHED = set()
_DONE = {}


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.fixture(scope="module")
def tally():
    yield None
    kc.layer_contract_report("every entry on the emulator")


_RUNNERS = {
    "bn": lambda lib, g: kc.bn_contract_case(lib, "cpu", *g, seed=sum(map(int, g))),
    "bn_stem": lambda lib, g: kc.bn_stem_contract_case(lib, "cpu", *g, seed=sum(g)),
    "pool": lambda lib, g: kc.pool_contract_case(lib, "cpu", *g, seed=sum(g[:7])),
    "mmpool": lambda lib, g: kc.mmpool_contract_case(lib, "cpu", *g, seed=g[0] + g[1] + g[2]),
    "dw": lambda lib, g: kc.dw_contract_case(lib, "cpu", *g, seed=sum(g)),
    "se": lambda lib, g: kc.se_contract_case(lib, "cpu", *g, seed=sum(g)),
    "drop": lambda lib, g: kc.drop_connect_contract_case(lib, "cpu", *g, seed=g[0] + g[1]),
    "ssim": lambda lib, g: kc.ssim_contract_case(lib, "cpu", *g, seed=sum(g[:3])),
    "ssim_finish": lambda lib, g: kc.ssim_finish_contract_case(lib, "cpu", g, seed=g),
}
_LISTS = {"bn": BN_GEOMS, "bn_stem": BN_STEM_GEOMS, "pool": POOL_GEOMS, "mmpool": MMPOOL_GEOMS, "dw": DW_GEOMS, "se": SE_GEOMS,
          "drop": DROP_GEOMS, "ssim": SSIM_GEOMS, "ssim_finish": SSIM_FINISH_COUNTS}


def _run(lib, family, geo):
    """One geometry, once per session; the kernels it launched go to LAUNCHED."""
    key = (family, geo)
    if key not in _DONE:
        kc.launch_log(lib)
        try:
            _DONE[key] = _RUNNERS[family](lib, geo)
        finally:
            LAUNCHED.update(k.replace(" ", "") for k in kc.launch_log(lib))
    return _DONE[key]


@pytest.mark.parametrize("geo", BN_GEOMS, ids=_ids)
def test_every_bn_entry_on_every_geometry(hostsim_lib, tally, geo):
    _run(hostsim_lib, "bn", geo)


@pytest.mark.parametrize("geo", BN_STEM_GEOMS, ids=_ids)
def test_fused_stem_on_every_geometry(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "bn_stem", geo) == kc.bn_stem_contract_expect(*geo)


@pytest.mark.parametrize("geo", POOL_GEOMS, ids=_ids)
def test_every_maxpool_entry_on_every_geometry(hostsim_lib, tally, geo):
    _run(hostsim_lib, "pool", geo)


@pytest.mark.parametrize("geo", POOL_FLAT_REGRESSIONS, ids=_ids)
def test_flat_maxpool_refuses_an_image_below_the_window(hostsim_lib, geo):
    """(2, 2, 0) on a one-pixel-high or -wide image has no output row: the flat forms must refuse it like the plain forms do."""
    assert geo in POOL_GEOMS and not kc.pool_contract_expect(*geo[:7])["maxpool2d_fwd_flat"]
    N, H, W, C, k, s, p, _ = geo
    G = kc.Guards("cpu")
    x, y, tap = G.inp(torch.zeros(N, H, W, C)), G.out(N, C * 2 * max(H, W)), G.out(N * C * 2 * max(H, W), dtype=torch.uint8)
    kc._contract_rejects(lambda: hostsim_lib.maxpool2d_fwd_flat(x, N, H, W, C, k, s, p, y, tap), G.wholes(), f"maxpool2d_fwd_flat {geo}")
    kc._contract_rejects(lambda: hostsim_lib.maxpool2d_bwd_flat(y, tap, N, H, W, C, k, s, p, G.out(N, H, W, C)), G.wholes(), f"maxpool2d_bwd_flat {geo}")


@pytest.mark.parametrize("geo", MMPOOL_GEOMS, ids=_ids)
def test_mmpool_on_every_geometry(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "mmpool", geo) == kc.mmpool_contract_expect(*geo[:3])


@pytest.mark.parametrize("geo", DW_GEOMS, ids=_ids)
def test_every_depthwise_entry_on_every_geometry(hostsim_lib, tally, geo):
    assert _run(hostsim_lib, "dw", geo) == kc.dw_contract_expect(*geo)


@pytest.mark.parametrize("geo", SE_GEOMS, ids=_ids)
def test_every_se_entry_on_every_geometry(hostsim_lib, tally, geo):
    _run(hostsim_lib, "se", geo)


@pytest.mark.parametrize("geo", DROP_GEOMS, ids=_ids)
def test_drop_connect_on_every_geometry(hostsim_lib, tally, geo):
    _run(hostsim_lib, "drop", geo)


@pytest.mark.parametrize("geo", SSIM_GEOMS, ids=_ids)
def test_every_ssim_entry_on_every_geometry(hostsim_lib, tally, geo):
    _run(hostsim_lib, "ssim", geo)


@pytest.mark.parametrize("count", SSIM_FINISH_COUNTS)
def test_ssim_finish_on_every_count(hostsim_lib, tally, count):
    _run(hostsim_lib, "ssim_finish", count)


def test_bn_m1_rule(hostsim_lib):
    """M = 1 (nn.BatchNorm2d raises): variance 0, save_invstd = 1 / sqrt(eps), y = act(beta), the running variance takes the biased value."""
    lib, C, eps, mom = hostsim_lib, 8, 1e-3, 0.25
    x = torch.arange(C, dtype=torch.float32).view(1, C) - 3
    gamma, beta = torch.full((C,), 1.5), torch.linspace(-1, 1, C)
    stats = torch.zeros(lib.bn_stats_floats(C))
    lib.bn_stats(x, 1, C, stats)
    y, sm, si, rm, rv = torch.empty(1, C), torch.empty(C), torch.empty(C), torch.zeros(C), torch.ones(C)
    lib.bn_act_fwd(x, stats, gamma, beta, None, 0, 1, C, eps, mom, y, sm, si, rm, rv)
    assert torch.equal(sm, x[0])
    # y = x sc + sh with sc = gamma / sqrt(eps), sh = beta - mean sc: the two terms cancel to the rounding of their size
    assert float((y[0] - beta).abs().max()) <= 4 * 6e-8 * float(x.abs().max()) * 1.5 * eps ** -0.5
    assert float((si - eps ** -0.5).abs().max()) <= 4e-7 * eps ** -0.5
    assert float((rm - mom * x[0]).abs().max()) <= 1e-6 and float((rv - (1 - mom)).abs().max()) <= 1e-6


def test_detection_the_comparator_notices_one_missing_contribution():
    """No kernel involved: a float64 reference with ONE contribution removed -- a row of M, a filter tap, a pixel of HW, a sample of B, a tile
    of the SSIM partials -- must fail the comparator on every emulator geometry, or the bounds would not notice a kernel that skips one."""
    missed = []
    fails = lambda ref, bad, name: not kc.layer_passes(ref[name][0], bad[name][2], ref[name][2], ref[name][1], ref[name][3] if len(ref[name]) > 3 else 0.0)
    for g in BN_GEOMS:
        M, C, act, residual = g[:4]
        if not kc.bn_contract_expect(M, C)["bn_stats"] or (act == 2 and residual):
            continue
        inp = kc.bn_contract_inputs(M, C, residual, sum(map(int, g)))
        ref, _ = kc.bn_contract_ref(inp, act, 1e-5, 0.1)
        bad, _ = kc.bn_contract_ref(inp, act, 1e-5, 0.1, drop_row=M - 1)
        names = ("sum", "sumsq", "dgamma", "dbeta") if M > 1 else ("sum", "sumsq", "dbeta")      # (M = 1: xhat = 0, the row adds nothing to dgamma)
        missed += [("bn", g, n) for n in names if not fails(ref, bad, n)]
    for g in MMPOOL_GEOMS:
        if kc.mmpool_contract_expect(*g[:3]):
            x, gy = kc.mmpool_contract_inputs(g[0], g[1], g[2], g[4], g[0] + g[1] + g[2])
            worst = int(x.abs().amax((0, 2)).argmax())                       # (post-ReLU inputs are mostly zeros: a pixel that holds something)
            ref, bad = kc.mmpool_contract_ref(x, g[3], gy), kc.mmpool_contract_ref(x, g[3], gy, drop_pixel=worst)
            names = ("y", "xavg") if g[3] < 10 else ("xavg",)             # (p = 30: 1 - sigmoid(p) = 1e-13, the mean does not reach y)
            missed += [("mmpool", g, n) for n in names if not fails(ref, bad, n)]
    for g in DW_GEOMS:
        if kc.dw_contract_expect(*g):
            inp = kc.dw_contract_inputs(g[0], g[1], g[2], g[3], g[4], g[8], g[9], sum(g))
            for pre in (False, True):
                ref, bad = kc.dw_contract_ref(inp, g, pre), kc.dw_contract_ref(inp, g, pre, drop_tap=True)
                missed += [("dw", g, pre, n) for n in ("y", "dx") if not fails(ref, bad, n)]
            N, OH, OW = g[0], g[8], g[9]                                   # the weight gradient without one output pixel's contribution
            ref = kc.dw_contract_ref(inp, g, False)
            inp2 = dict(inp, gy=inp["gy"].clone())
            inp2["gy"][0, 0, 0] = 0
            missed += [("dw", g, "dw")] if not fails(ref, kc.dw_contract_ref(inp2, g, False), "dw") else []
    for g in SE_GEOMS:
        B, HW, C, SQ = g
        exp = kc.se_contract_expect(*g)
        inp = kc.se_contract_inputs(B, HW, C, max(SQ, 1), sum(g))
        if exp["se_pool"]:
            ref, bad = kc.se_plain_ref(inp), kc.se_plain_ref(inp, drop_pixel=HW - 1)
            missed += [("se", g, n) for n in ("pool", "bwd_gate") if not fails(ref, bad, n)]
        if exp["se_mlp_fwd"]:
            f = kc.se_mlp_fwd_ref(inp)
            saved = [f[k][2] for k in ("gate", "z1", "h1", "mean")]
            ref, bad = kc.se_mlp_bwd_ref(inp, *saved), kc.se_mlp_bwd_ref(inp, *saved, drop_sample=B - 1)
            missed += [("se", g, n) for n in ("dw1", "db1", "dw2", "db2") if not fails(ref, bad, n)]
    for g in SSIM_GEOMS:
        a, b = kc.ssim_contract_inputs(g[0], g[1], g[2], g[3], sum(g[:3]))
        ref, bad = kc.ssim_contract_ref(a, b, 2.0), kc.ssim_contract_ref(a, b, 2.0, drop_tile=True)
        missed += [("ssim", g, "value")] if not fails(ref, bad, "value") else []
    assert not missed, f"the comparator accepts a reference with one contribution removed: {missed}"


def test_no_bound_is_looser_than_the_family_case_it_replaces():
    """c sqrt(L) is capped by the relative tolerance of the family's older case (the second column of LAYER_CONTRACT_C)."""
    legacy = {"bn_sum": 1e-4, "bn_stat": 1e-5, "bn_y": 2e-5, "bn_dx": 2e-4, "bn_dparam": 2e-4, "pool_dx": 2e-6, "mm_y": 1e-5, "mm_dx": 1e-5,
              "mm_dp": 1e-4, "dw_fwd": 2e-5, "dw_pre": 3e-5, "dw_dgrad": 2e-5, "dw_wgrad": 1e-4, "dw_wgrad_pre": 2e-4, "se_pool": 1e-5,
              "se_y": 3e-5, "se_mlp": 2e-5, "se_grad": 3e-4, "ssim_val": 2e-6, "ssim_part": 2e-6, "ssim_map": 2.1e-3, "ssim_grad": 2e-4}      # (no older case asserts on the SSIM maps)
    # (the kinds of the GEMM contract live in the same table: tests/test_hostsim_gemm_contract.py holds them to their own older cases)
    # (so do the kinds of the tail contract: tests/test_hostsim_tail_contract.py holds them to kc.TAIL_LEGACY)
    # (and those of the renderer contract: tests/test_hostsim_render_contract.py holds them to render_case / render_uv_case)
    assert set(legacy) == (set(kc.LAYER_CONTRACT_C) - set(kc.GEMM_CONTRACT_KINDS) - set(kc.WINO_CONTRACT_KINDS) - set(kc.TAIL_CONTRACT_KINDS) -
                           set(kc.RENDER_CONTRACT_KINDS))
    for kind in legacy:
        c, cap = kc.LAYER_CONTRACT_C[kind]
        assert 0 < c <= cap <= legacy[kind], kind
        ref = torch.ones(3, dtype=torch.float64)
        assert kc.layer_bound(kind, ref, 10 ** 12) <= legacy[kind] + kc.LAYER_CONTRACT_FLOOR.get(kind, 0.0)


def test_the_lists_reach_every_instantiation_and_both_answers(hostsim_lib):
    """A geometry edit that stops reaching a kernel, a predicate answer or an accept / refuse rule fails here."""
    lib = hostsim_lib
    for family, geoms in _LISTS.items():                                     # (whatever a -k selection left out runs now)
        for g in geoms:
            _run(lib, family, g)
    assert EXPECT_LAUNCHED <= LAUNCHED, f"no geometry reaches {sorted(EXPECT_LAUNCHED - LAUNCHED)}"
    assert "maxpool3s2_notap_kernel" in LAUNCHED
    # both answers of every predicate, both outcomes of every accept / refuse rule
    assert {lib.bn_relu_maxpool_supported(*g) for g in BN_STEM_GEOMS} == {True, False}
    assert {lib.se_mlp_supported(g[2], g[3]) for g in SE_GEOMS} == {True, False}
    for e in ("bn_stats", "bn_bwd_apply"):
        assert {kc.bn_contract_expect(g[0], g[1])[e] for g in BN_GEOMS} == {True, False}, e
    for e in ("maxpool2d_fwd", "maxpool2d_fwd_notap"):
        assert {kc.pool_contract_expect(*g[:7])[e] for g in POOL_GEOMS} == {True, False}, e
    assert {kc.mmpool_contract_expect(*g[:3]) for g in MMPOOL_GEOMS} == {True, False}
    assert {kc.dw_contract_expect(*g) for g in DW_GEOMS} == {True, False}
    for e in ("se_pool", "se_mlp_fwd"):
        assert {kc.se_contract_expect(*g)[e] for g in SE_GEOMS} == {True, False}, e
    assert {bool(_DONE[("drop", g)]) for g in DROP_GEOMS} == {True, False}
    for e, row in kc.LAYER_CONTRACT_LOG.items():
        if e.startswith(kc.GEMM_CONTRACT_ENTRIES) or e in kc.TAIL_CONTRACT_ENTRIES:          # (the GEMM and tail contracts log into the same table and ask this of their own entries)
            continue
        assert row[0] > 0 and (row[1] > 0 or e in ("ssim_bwd", "ssim_bwd_scaled")), f"{e}: accepted {row[0]}, refused {row[1]} calls"
    # the classes the lists exist for
    assert {g[1] for g in BN_GEOMS} >= {4, 8, 12, 64, 256, 260, 512, 516, 1024, 1028, 2304, 4096, 0, 2, 6, 4100}
    assert {g[0] for g in BN_GEOMS} >= {1, 2, 3, 5, 15, 16, 17, 127, 128, 129} and {g[0] % 4 for g in BN_GEOMS} == {0, 1, 2, 3}
    assert {(g[2], g[3], g[4]) for g in BN_GEOMS} >= {(a, r, True) for a in (0, 1) for r in (False, True)} | {(1, False, False), (2, False, True)}
    assert {g[5] for g in BN_GEOMS} == {True, False}
    acc = [g for g in DW_GEOMS if kc.dw_contract_expect(*g)]
    assert {g[9] % 4 for g in acc} == {0, 1, 2, 3} and {g[3] for g in acc} >= set(_DW_C) and {g[0] for g in acc} == {1, 3}
    assert {(g[4], g[5]) for g in acc} == {(3, 1), (3, 2), (5, 1), (5, 2)} and any(g[1] < g[4] for g in acc)
    for K in (3, 5):
        assert {(g[6], g[7]) for g in acc if g[4] == K} >= {(0, 0), (K // 2, K // 2), (K - 1, K - 1)}
    assert any(g[0] > 48 and kc.se_contract_expect(*g)["se_mlp_bwd"] for g in SE_GEOMS), "the SE weight gradient never takes a second pass"
    assert {g[0] for g in SE_GEOMS} >= {1, 2, 48, 49, 96, 97} and {g[3] for g in SE_GEOMS} >= {1, 6, 34, 96, 256, 257}
    assert {g[1] for g in SE_GEOMS} >= {1, 2, 49, 196} and {g[2] for g in SE_GEOMS} >= {4, 40, 132, 2304, 4096, 4100}
    assert {g[0] for g in SSIM_GEOMS} == {1, 6} and {g[3] for g in SSIM_GEOMS} == {"random", "identical", "constants", "masked"}
    ws = {g[2] for g in SSIM_GEOMS}
    assert any(w % 4 for w in ws) and any(w % 4 == 0 and w % 32 for w in ws) and any(w % 32 == 0 for w in ws)
