"""The convolution C ABI's contract on the hostsim emulator: every entry point (forward with and without bias / ReLU / statistics / the balanced
schedule, the three backward-data forms, backward-weight with its slab form, the fused plus1x1 backward launches, the forward pair and the
3-channel stem gradient) on a fixed list of geometries -- square and non-square filters, strides 1-4, every pad below the filter and some at
or above it, channel counts that are and are not multiples of 16.  An entry either refuses a geometry (HIFIHR_EINVAL, output untouched) or
matches float64 autograd (tests/kernel_cases.py conv_contract_case).  The GPU half runs the same list in tests/test_gpu_conv.py."""
import re

import pytest

import kernel_cases as kc

# (N, H, W, C, K, R, S, stride, pad)
CONTRACT_GEOMS = [
    # 1x1: stride 1 on the GEMM kernels (plain, ragged, the weight gradient's TN slabs), strided, pads at and above the filter
    (1, 4, 4, 256, 128, 1, 1, 1, 0),
    (1, 4, 6, 136, 232, 1, 1, 1, 0),
    (2, 3, 5, 64, 128, 1, 1, 1, 0),
    (2, 7, 5, 32, 48, 1, 1, 2, 0),
    (1, 9, 7, 12, 20, 1, 1, 3, 1),
    (1, 6, 5, 32, 16, 1, 1, 4, 2),
    # 2x2
    (2, 7, 9, 32, 64, 2, 2, 1, 0),
    (1, 8, 7, 12, 16, 2, 2, 2, 1),
    (1, 9, 6, 64, 48, 2, 2, 3, 2),
    # 3x3: the named kernels, channel counts off 16 / 32, every stride, every pad, pad >= filter
    (1, 3, 14, 64, 64, 3, 3, 1, 1),      # conv_halo_kernel, conv_halo_wgrad_kernel (OW % 14 == 0)
    (1, 5, 15, 64, 64, 3, 3, 1, 1),      # conv_halo_kernel, ragged column tile; weight gradient on conv_wgrad_kernel
    (1, 7, 7, 32, 128, 3, 3, 2, 1),      # bgemm_nt_rows_kernel<2>: the strided forward as the gathering row-share GEMM
    (1, 6, 5, 32, 4, 3, 3, 1, 1),        # conv3x3_oc4_kernel forward (K = 4)
    (1, 6, 7, 4, 64, 3, 3, 1, 1),        # conv3x3_oc4_kernel backward-data (C = 4 from K = 64)
    (2, 9, 7, 128, 192, 3, 3, 1, 1),     # fwd and dgrad balanced schedules on the emulator's 16 persistent workgroups
    (2, 5, 7, 136, 48, 3, 3, 1, 0),
    (1, 9, 8, 12, 20, 3, 3, 1, 1),       # C, K off 16: the generic gather forward and stride-1 backward-data
    (2, 9, 8, 12, 20, 3, 3, 2, 1),       # K = 20 at stride 2: backward-data refused
    (1, 10, 9, 32, 64, 3, 3, 2, 1),
    (3, 7, 6, 4, 16, 3, 3, 2, 0),
    (1, 11, 10, 32, 48, 3, 3, 3, 1),
    (1, 9, 11, 64, 16, 3, 3, 4, 2),
    (1, 5, 6, 32, 16, 3, 3, 1, 3),       # pad == filter
    (1, 4, 5, 12, 16, 3, 3, 2, 4),       # pad > filter
    (1, 12, 12, 32, 64, 3, 3, 2, 1),     # ResNet layer2.0 class: both plus1x1 launches
    (1, 9, 13, 16, 32, 3, 3, 2, 1),
    # 5x5
    (1, 9, 9, 32, 16, 5, 5, 1, 2),
    (2, 7, 8, 12, 48, 5, 5, 1, 0),
    (1, 11, 9, 64, 16, 5, 5, 2, 1),
    (1, 10, 12, 32, 64, 5, 5, 2, 2),
    (1, 9, 10, 4, 16, 5, 5, 3, 3),
    (1, 9, 7, 32, 16, 5, 5, 4, 4),
    (1, 5, 5, 16, 16, 5, 5, 1, 5),
    # 7x7: the stem (conv_stem_kernel, conv_stem_wgrad_kernel, the 3-channel parameter), every pad
    (1, 4, 56, 4, 64, 7, 7, 2, 3),
    (1, 9, 9, 4, 64, 7, 7, 2, 3),
    (1, 9, 8, 16, 16, 7, 7, 1, 0),
    (1, 7, 9, 12, 16, 7, 7, 2, 1),
    (1, 8, 7, 16, 48, 7, 7, 2, 2),
    (1, 9, 9, 16, 16, 7, 7, 3, 4),
    (1, 7, 6, 4, 20, 7, 7, 1, 5),
    (1, 5, 5, 16, 16, 7, 7, 4, 6),
    (1, 3, 4, 16, 16, 7, 7, 2, 7),
    # 1x3 / 3x1
    (2, 7, 9, 32, 16, 1, 3, 1, 0),
    (1, 8, 7, 16, 48, 1, 3, 2, 1),
    (1, 9, 10, 12, 16, 1, 3, 3, 2),
    (1, 6, 9, 16, 16, 1, 3, 4, 3),
    (2, 9, 7, 32, 16, 3, 1, 1, 0),
    (1, 7, 8, 16, 48, 3, 1, 2, 1),
    (1, 10, 9, 12, 16, 3, 1, 3, 2),
    (1, 9, 6, 16, 16, 3, 1, 4, 3),
    # the regression geometries of bwd_data_pre_plus1x1: parity class (0, 0) with row taps and no column taps
    (1, 9, 7, 16, 32, 3, 1, 3, 1),
    (2, 8, 10, 32, 16, 3, 1, 3, 1),
    (2, 8, 10, 32, 16, 3, 1, 4, 1),
    # 3x5 / 5x3 / 3x2
    (1, 7, 9, 32, 16, 3, 5, 1, 0),
    (1, 9, 8, 16, 48, 3, 5, 2, 1),
    (1, 8, 11, 12, 16, 3, 5, 3, 2),
    (1, 9, 9, 16, 16, 3, 5, 4, 3),
    (1, 6, 7, 16, 16, 3, 5, 2, 4),
    (1, 5, 6, 16, 16, 3, 5, 1, 5),
    (1, 9, 7, 32, 16, 5, 3, 1, 0),
    (1, 8, 9, 16, 48, 5, 3, 2, 1),
    (1, 11, 8, 12, 16, 5, 3, 3, 2),
    (1, 9, 9, 16, 16, 5, 3, 4, 3),
    (1, 7, 6, 16, 16, 5, 3, 2, 4),
    (1, 6, 5, 16, 16, 5, 3, 1, 5),
    (2, 7, 8, 32, 16, 3, 2, 1, 0),
    (1, 9, 8, 16, 48, 3, 2, 2, 1),
    (1, 8, 10, 12, 16, 3, 2, 3, 2),
    (1, 6, 7, 16, 16, 3, 2, 4, 3),
]

# bwd_data_pre_plus1x1_supported accepted these while class (0, 0) had row taps and no column taps (the fused tap ran as an ordinary one)
PLUS1X1_REGRESSIONS = [(1, 9, 7, 16, 32, 3, 1, 3, 1), (2, 8, 10, 32, 16, 3, 1, 3, 1), (2, 8, 10, 32, 16, 3, 1, 4, 1)]

# (N, H, W, C, stride, K1, R1, pad1, K2, R2, pad2) for conv2d_fwd_bnstats_pair
PAIR_GEOMS = [
    (2, 12, 12, 32, 2, 128, 3, 1, 128, 1, 0),     # the ResNet stage's first block: equal output grids
    (1, 9, 11, 64, 2, 128, 3, 0, 256, 1, 0),      # different output sizes (4 x 5 and 5 x 6)
    (1, 10, 9, 32, 2, 128, 1, 1, 128, 3, 2),      # (R, pad) swapped round, pads at the filter and above it
    (1, 7, 7, 32, 2, 128, 3, 2, 128, 3, 0),       # two 3x3 convolutions
    (1, 8, 8, 32, 1, 128, 3, 1, 128, 1, 0),       # stride 1: refused
    (1, 8, 8, 32, 2, 128, 5, 2, 128, 1, 0),       # 5x5: refused
    (1, 8, 8, 32, 2, 64, 3, 1, 128, 1, 0),        # K1 % 128: refused
    (1, 8, 8, 12, 2, 128, 3, 1, 128, 1, 0),       # C % 32: refused
]

# the kernels hifihr_conv2d_describe can name (directions 0, 1, 2) that the list must keep reaching
DESCRIBED = {"conv_halo_kernel", "conv_stem_kernel", "bgemm_nt_rows_kernel<2>", "conv_igemm_kernel", "conv_halo_wgrad_kernel",
             "conv_stem_wgrad_kernel", "conv_wgrad_kernel", "bgemm_nt_rows_kernel<0>", "bgemm_nt_rows_kernel<1>", "conv3x3_oc4_kernel",
             "conv3x3_oc4_tile_kernel"}

# kernels that run beside the one hifihr_conv2d_describe names: the filter transpose of the plain backward-data entry, the sums over the
# slabs of a weight gradient
HELPER_KERNELS = {"weight_transpose_kernel", "slab_sum_acc_kernel", "conv_halo_wgrad_reduce_kernel", "conv_stem_wgrad_reduce_kernel"}


def dispatch_coverage(lib, geoms):
    names = set()
    for g in geoms:
        for direction in (0, 1, 2):
            names.add(lib.conv2d_describe(*g, direction))
    return names


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.fixture(scope="module")
def tally():
    t = {}
    yield t
    print("\nconvolution contract on the emulator (entry: accepted / refused geometries):")
    for e, (a, r) in sorted(t.items()):
        print(f"  {e:24s} {a:3d} / {r:3d}")
    print("largest err / bound per entry:", {e: round(v[2], 3) for e, v in sorted(kc.CONV_CONTRACT_LOG.items()) if v[0]})


@pytest.mark.parametrize("geo", CONTRACT_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_every_conv_entry_on_every_geometry(hostsim_lib, tally, geo):
    got = kc.conv_contract_case(hostsim_lib, "cpu", *geo, seed=sum(geo))
    for e, ok in got.items():
        tally.setdefault(e, [0, 0])[0 if ok else 1] += 1


@pytest.mark.parametrize("geo", PLUS1X1_REGRESSIONS, ids=lambda g: "x".join(map(str, g)))
def test_plus1x1_dgrad_refuses_a_class_without_column_taps(hostsim_lib, geo):
    """Parity class (0, 0) of these has row taps and no column taps: the second convolution's tap cannot ride on it."""
    assert geo in CONTRACT_GEOMS
    assert not hostsim_lib.conv2d_bwd_data_pre_plus1x1_supported(*geo)


@pytest.mark.parametrize("N,H,C,K", [(32, 56, 64, 128), (32, 28, 128, 256), (3, 31, 32, 48)])
def test_network_shapes_keep_the_fused_launches(hostsim_lib, monkeypatch, N, H, C, K):
    """ResNet-18 layer2.0 / layer3.0 (3x3 / stride 2 / pad 1 and the 1x1 / stride 2 downsample): both plus1x1 backward launches, and the
    forward pair where K is a multiple of 128."""
    monkeypatch.setenv("HIFIHR_GEMM_CUS", "16")
    assert hostsim_lib.conv2d_bwd_data_pre_plus1x1_supported(N, H, H, C, K, 3, 3, 2, 1)
    assert hostsim_lib.conv2d_bwd_weight_plus1x1_supported(N, H, H, C, K, 3, 3, 2, 1)
    assert hostsim_lib.conv2d_fwd_bnstats_pair_supported(N, H, H, C, 2, K, 3, 1, K, 1, 0) == (K % 128 == 0)


@pytest.mark.parametrize("pair", PAIR_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_fwd_bnstats_pair_on_every_pair(hostsim_lib, monkeypatch, pair):
    monkeypatch.setenv("HIFIHR_GEMM_CUS", "16")     # the pair wants at least 8 workgroups per side; the emulator reports 4 CUs
    accepted = kc.conv_pair_contract_case(hostsim_lib, "cpu", *pair, seed=sum(pair))
    assert accepted == (pair[4] == 2 and pair[3] % 32 == 0 and pair[5] % 128 == 0 and pair[8] % 128 == 0 and {pair[6], pair[9]} <= {1, 3})


@pytest.mark.parametrize("geo", CONTRACT_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_describe_names_the_kernel_that_runs(hostsim_lib, geo):
    """hifihr_conv2d_describe against the emulator's launch log: every plain entry that accepts the geometry (forward without bias,
    backward-data, backward-weight, each with the workspace its query asks for) launches exactly the kernel describe names, helper kernels
    aside.  Names are compared up to the template arguments (the log spells those as the launch site does)."""
    import torch
    lib = hostsim_lib
    N, H, W, C, K, R, S, stride, pad = geo
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    x, w, gy = torch.ones(N, H, W, C), torch.ones(K, R, S, C), torch.ones(N, OH, OW, K)
    ws_of = lambda nbytes: torch.zeros((nbytes + 3) // 4) if nbytes else None
    # (a logged template argument list without an identifier is literal: bgemm_nt_rows_kernel<0> / <1> / <2> are then told apart)
    literal = lambda name: "<" not in name or not re.search(r"[A-Za-z_]", name.split("<", 1)[1].replace("true", "").replace("false", ""))
    base = lambda name: name.split("<")[0]
    expect = kc.conv_contract_expect(*geo)
    calls = (("fwd", 0, lambda: lib.conv2d_fwd(x, w, None, torch.empty(N, OH, OW, K), *geo, ws=ws_of(lib.conv2d_workspace_bytes(*geo, False)))),
             ("dgrad", 1, lambda: lib.conv2d_bwd_data(gy, w, torch.empty(N, H, W, C), torch.empty(K * R * S * C), *geo,
                                                      ws=ws_of(lib.conv2d_workspace_bytes(*geo, True)))),
             ("wgrad", 2, lambda: lib.conv2d_bwd_weight(x, gy, torch.zeros(K, R, S, C), *geo, ws=ws_of(lib.conv2d_wgrad_workspace_bytes(*geo)))))
    for entry, direction, call in calls:
        if not expect[entry]:
            continue
        kc.launch_log(lib)
        call()
        ran = [k for k in kc.launch_log(lib) if base(k) not in HELPER_KERNELS]
        named = lib.conv2d_describe(*geo, direction)
        assert [base(k) for k in ran] == [base(named)], f"{entry} {geo}: describe names {named}, the launch log shows {ran}"
        if literal(ran[0]) and "<" in named:
            assert ran[0].replace(" ", "") == named.replace(" ", ""), f"{entry} {geo}: describe names {named}, the launch log shows {ran}"


def test_the_list_reaches_every_dispatch_path(hostsim_lib):
    """A geometry edit that stops reaching a kernel fails here instead of shrinking the coverage quietly."""
    names = dispatch_coverage(hostsim_lib, CONTRACT_GEOMS)
    assert DESCRIBED <= names, f"no geometry reaches {sorted(DESCRIBED - names)}"
    assert any(n.startswith("bgemm_tn") for n in names), "no 1x1 weight gradient on the TN GEMM slabs"
    # and what the entries are asked about: both answers of every predicate occur in the list
    lib = hostsim_lib
    for pred in (lib.conv2d_bwd_data_pre_plus1x1_supported, lib.conv2d_bwd_weight_plus1x1_supported):
        answers = {pred(*g) for g in CONTRACT_GEOMS}
        assert answers == {True, False}, pred
    assert {lib.conv2d_bwd_weight_c3_supported(N, H, W, K, R, S, st, p) for N, H, W, C, K, R, S, st, p in CONTRACT_GEOMS if C == 4} == {True, False}
    assert {bool(lib.conv2d_wgrad_workspace_bytes(*g)) for g in CONTRACT_GEOMS} == {True, False}
    assert any(lib.conv2d_workspace_bytes(*g, False) for g in CONTRACT_GEOMS) and any(lib.conv2d_workspace_bytes(*g, True) for g in CONTRACT_GEOMS)
    expect = [kc.conv_contract_expect(*g) for g in CONTRACT_GEOMS]
    assert {e["dgrad"] for e in expect} == {True, False}
    geoms = set(CONTRACT_GEOMS)
    assert {(R, S) for _, _, _, _, _, R, S, _, _ in geoms} >= {(1, 1), (2, 2), (3, 3), (5, 5), (7, 7), (1, 3), (3, 1), (3, 5), (5, 3), (3, 2)}
    assert {st for *_, st, _ in geoms} == {1, 2, 3, 4}
    for R, S in {(g[5], g[6]) for g in geoms}:
        pads = {g[8] for g in geoms if (g[5], g[6]) == (R, S)}
        assert set(range(max(R, S))) <= pads and max(pads) >= max(R, S), (R, S, pads)
