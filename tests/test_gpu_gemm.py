"""csrc/gemm.hip through the C ABI on the GPU: the Winograd GEMM shapes of the ResNet-18 step at B = 32 and ragged / small ones."""
import pytest
import torch

import kernel_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    return get_lib()


@pytest.mark.parametrize("M,N,K,batch", [(6272, 128, 128, 16), (1568, 256, 256, 16), (1568, 512, 256, 16), (1568, 256, 512, 16),
                                         (1568, 512, 512, 16), (98, 128, 64, 2), (130, 192, 32, 3), (40, 64, 96, 1)])
def test_bgemm_nt(lib, M, N, K, batch):
    kc.bgemm_case(lib, "cuda", M, N, K, batch, seed=M + N + K)


@pytest.mark.parametrize("M,N,T,batch", [(128, 128, 6272, 16), (256, 256, 1568, 16), (512, 256, 1568, 16), (512, 512, 1568, 16),
                                         (64, 128, 98, 2), (128, 64, 40, 1), (64, 64, 777, 1)])
def test_bgemm_tn(lib, M, N, T, batch):
    kc.bgemm_tn_case(lib, "cuda", M, N, T, batch, seed=M + T)


def test_bgemm_tn_is_bit_reproducible(lib):
    """No atomics: two launches give identical slabs."""
    gen = torch.Generator().manual_seed(5)
    M, N, T, batch = 256, 256, 1568, 16
    a = torch.randn(batch, T, M, generator=gen).cuda(); b = torch.randn(batch, T, N, generator=gen).cuda()
    parts = lib.bgemm_tn_parts(M, N, T, batch)
    c1 = torch.empty(parts, batch, M, N, device="cuda"); c2 = torch.empty_like(c1)
    lib.bgemm_tn(a, b, c1, M, N, T, batch, parts); lib.bgemm_tn(a, b, c2, M, N, T, batch, parts)
    assert torch.equal(c1, c2)


@pytest.mark.parametrize("M,N,K,batch", [(300, 256, 96, 3), (50, 128, 32, 5), (129, 384, 64, 2), (17, 128, 160, 9), (100000, 128, 32, 1),
                                         (6272, 128, 128, 7), (2352, 256, 256, 16)])
def test_bgemm_nt_row_shares(lib, M, N, K, batch):
    """bgemm_nt_rows_kernel on 256 workgroups: shares ending inside tiles (1..8 row blocks), crossing column-tile and problem boundaries,
    a B = 48-sized product and a very tall one."""
    assert lib.bgemm_describe(False, M, N, K) .startswith("bgemm_nt_rows_kernel<")
    assert kc.bgemm_case(lib, "cuda", M, N, K, batch, seed=M + K) == 0


def test_bgemm_nt_rows_is_bit_reproducible(lib):
    gen = torch.Generator().manual_seed(9)
    a = torch.randn(16, 1568, 512, generator=gen).cuda(); b = torch.randn(16, 512, 512, generator=gen).cuda()
    c1 = torch.empty(16, 1568, 512, device="cuda"); c2 = torch.empty_like(c1)
    lib.bgemm_nt(a, b, c1, 1568, 512, 512, 16); lib.bgemm_nt(a, b, c2, 1568, 512, 512, 16)
    assert torch.equal(c1, c2)


@pytest.mark.parametrize("M,N,T,batch", [(512, 512, 512, 36), (512, 256, 512, 36), (256, 512, 768, 36), (320, 384, 96, 40), (128, 128, 64, 300)])
def test_bgemm_tn_row_shares(lib, M, N, T, batch):
    """bgemm_tn_rows_kernel on 256 workgroups (the F(4x4, 3x3) backward-weight shapes of layer 4 and shapes whose shares end inside tiles:
    64 / 32 / 16-row tail tiles, column-tile and problem boundaries): complete products in one slab, bit-reproducible."""
    assert lib.bgemm_describe(True, M, N, T, batch) == "bgemm_tn_rows_kernel"
    assert kc.bgemm_tn_case(lib, "cuda", M, N, T, batch, seed=M + T) == 1
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(batch, T, M, generator=gen).cuda(); b = torch.randn(batch, T, N, generator=gen).cuda()
    c1 = torch.empty(1, batch, M, N, device="cuda"); c2 = torch.full_like(c1, 7.0)
    lib.bgemm_tn(a, b, c1, M, N, T, batch, 1); lib.bgemm_tn(a, b, c2, M, N, T, batch, 1)
    assert torch.equal(c1, c2)


# ---- the GEMM contract (tests/kernel_cases.py "The GEMM contract"): the emulator's lists (tests/test_hostsim_gemm_contract.py) plus the few
# larger shapes whose 256-workgroup plan reaches what the small shapes reach on the emulator's 4 -- chosen with hifihr_bgemm_describe
# at 256 compute units: no small shape takes the stream-K kernel, the single-slab or T-split TN row-share kernel or shares above the minimum there.
from kernel_cases import (GEMM_ROUTES as ROUTES, NT_SHAPES, TN_SHAPES, TRANSPOSE_SHAPES, WINO_BN_GEOMS, WINO_GEOMS,  # noqa: E402
                          gemm_route as _route)

# (M, N, K, batch, route, workspace), the kernel it must name at 256 compute units
NT_SHAPES_GPU = [
    ((2048, 256, 64, 24, "ws4", "full"), "bgemm_nt_sk_kernel<4>"),           # 768 tiles x 2 chunks: 6 chunks per workgroup, every tile split
    ((2000, 128, 96, 52, "ws2", "full"), "bgemm_nt_sk_kernel<2>"),           # 832 tiles x 3 chunks, ragged M
    ((2000, 128, 96, 52, "ws2", "short"), "bgemm_ws_kernel<128, 128, false, 2>"),
    ((1000, 256, 64, 5, "default", "full"), "bgemm_nt_rows_kernel<0>"),      # 10 000 rows / 256: shares of 40 rows that end inside tiles
    ((1000, 576, 128, 3, "default", "full"), "bgemm_nt_rows_kernel<1>"),     # ragged N, shares of 59 rows
]
# (M, N, T, batch, route), the kernel and the slab count
TN_SHAPES_GPU = [
    ((320, 384, 96, 40, "default"), "bgemm_tn_rows_kernel", 1),             # shares ending inside 128-row tiles, 64-row tails
    ((512, 512, 64, 16, "default"), "bgemm_tn_rows_kernel", 1),             # 256 workgroups, 128 blocks per problem: the XCD-coherent schedule
    ((128, 256, 512, 36, "default"), "bgemm_tn_rows_kernel", 4),            # T-split
    ((256, 256, 256, 36, "default"), "bgemm_tn_rows_kernel", 2),
]


@pytest.fixture(scope="module")
def gemm_tally():
    yield None
    kc.layer_contract_report("GEMM and Winograd entries on the GPU", ("bgemm", "weight_transpose", "weight_prep", "wino"))


@pytest.mark.parametrize("geo", NT_SHAPES + [g for g, _ in NT_SHAPES_GPU], ids=lambda g: "x".join(map(str, g)))
def test_bgemm_nt_contract_on_every_shape(lib, gemm_tally, geo):
    with _route(geo[4]):
        accepted, _ = kc.bgemm_nt_contract_case(lib, "cuda", *geo[:4], ws_mode=geo[5], seed=sum(geo[:4]) % 1000)
    assert accepted == kc.bgemm_nt_expect(*geo[:4])


@pytest.mark.parametrize("geo", TN_SHAPES + [g for g, _, _ in TN_SHAPES_GPU], ids=lambda g: "x".join(map(str, g)))
def test_bgemm_tn_contract_on_every_shape(lib, gemm_tally, geo):
    with _route(geo[4]):
        parts = kc.bgemm_tn_contract_case(lib, "cuda", *geo[:4], seed=sum(geo[:4]) % 1000)
    assert (parts > 0) == kc.bgemm_tn_expect(*geo[:4])


@pytest.mark.parametrize("geo", TRANSPOSE_SHAPES + [(512, 9, 512)], ids=lambda g: "x".join(map(str, g)))
def test_weight_transpose_contract_on_every_shape(lib, gemm_tally, geo):
    assert kc.weight_transpose_contract_case(lib, "cuda", *geo, seed=sum(geo)) == (min(geo) > 0)


def test_the_gemm_contract_shapes_reach_every_kernel_on_this_device(lib):
    """What hifihr_bgemm_describe / _tn_parts / _nt_workspace_bytes name for the lists on THIS device's compute units: the larger
    shapes name what they were chosen for, and the lists together name every kernel of the family."""
    named = set()
    for g, kernel in NT_SHAPES_GPU:
        with _route(g[4]):
            assert lib.bgemm_describe(False, *g[:4]) == ("bgemm_nt_sk_kernel<2>" if g[5] == "short" else kernel), g
            assert (lib.bgemm_nt_workspace_bytes(*g[:4]) > 0) == (g[4] != "default"), g
        named.add(kernel)
    slabs = set()
    for g, kernel, parts in TN_SHAPES_GPU:
        with _route(g[4]):
            assert lib.bgemm_describe(True, *g[:4]) == kernel and lib.bgemm_tn_parts(*g[:4]) == parts, g
        named.add(kernel)
        slabs.add(parts)
    assert slabs >= {1, 2, 4}
    for tn, shapes in ((False, NT_SHAPES), (True, TN_SHAPES)):
        for g in shapes:
            if (kc.bgemm_tn_expect if tn else kc.bgemm_nt_expect)(*g[:4]):
                with _route(g[4]):
                    named.add(lib.bgemm_describe(tn, *g[:4]))
    expect = {f"bgemm_{d}_kernel<{bm}, {bn}>" for d in ("nt", "tn") for bm in (64, 128) for bn in (64, 128)}
    expect |= {f"bgemm_ws_kernel<128, 128, {t}, {w}>" for t in ("false", "true") for w in (1, 2, 4)}
    expect |= {"bgemm_nt_sk_kernel<2>", "bgemm_nt_sk_kernel<4>", "bgemm_nt_rows_kernel<0>", "bgemm_nt_rows_kernel<1>", "bgemm_tn_rows_kernel"}
    assert expect <= named, sorted(expect - named)
    assert set(ROUTES) >= {g[4] for g in NT_SHAPES + TN_SHAPES}


# (N, H, W, C, K, m): mosaics of 14 x 14 images and a 28 x 28 layer with the library's products on 256 compute units
WINO_GEOMS_GPU = [(16, 14, 14, 128, 64, 4), (32, 13, 13, 64, 128, 4), (4, 28, 28, 64, 128, 4), (4, 28, 28, 128, 64, 2)]


@pytest.mark.parametrize("geo", WINO_GEOMS + WINO_GEOMS_GPU, ids=lambda g: "x".join(map(str, g)))
def test_winograd_contract_every_transform_on_every_geometry(lib, gemm_tally, geo):
    with _route(kc.wino_route(geo)):
        assert kc.wino_chain_contract_case(lib, "cuda", *geo, seed=sum(geo)) == kc.wino_contract_expect(*geo)


@pytest.mark.parametrize("geo", WINO_BN_GEOMS + [(16, 14, 14, 256, 4, True, True), (8, 28, 28, 128, 4, False, False)], ids=lambda g: "x".join(map(str, g)))
def test_winograd_batch_norm_fusion_contract_on_every_geometry(lib, gemm_tally, geo):
    assert kc.wino_bn_contract_case(lib, "cuda", *geo, seed=sum(map(int, geo))) == kc.wino_bn_contract_expect(geo[3], geo[4])
