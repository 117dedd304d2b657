#!/usr/bin/env python3
"""Every answer the library gives about the dispatch of a shape, one line per shape, through the C ABI and without a launch:
hifihr_conv2d_describe (forward, backward-data, backward-weight), the workspace queries, the *_supported predicates of the fused
convolution entries, the GEMM describe / workspace / slab-count queries and the Winograd choices built on them.

Two libraries that print the same table send every one of these shapes to the same kernels with the same scratch: diff the table of a
dispatch change against profiles/dispatch_table.txt (the MI355X table of the committed code).

usage: python tools/dispatch_dump.py [--lib PATH] [--out FILE]
       --lib: another build of the library, e.g. tests/hostsim/libhifihr_hostsim.so (the emulator reports 4 compute units)
The switches of csrc/gemm.hip and csrc/conv.hip are read from the environment as usual (HIFIHR_GEMM_CUS=16 python tools/dispatch_dump.py ...).

Shapes: the contract geometries and pairs of tests/test_hostsim_conv_contract.py; ResNet-18's convolutions (tests/test_gpu_conv.py) at
N = 32; the convolutions of the VGG19 feature stack and of EfficientNet-b3 at N = 48 / 224 x 224 and of the light estimator, recorded
from a forward of the modules themselves on meta tensors; a grid of GEMM shapes."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def module_convs(N):
    """[(tag, (N, H, W, C, K, R, S, stride, pad))] of the networks' convolutions: each network's own forward runs on meta tensors with the
    entries of hifihr_amd.ops it calls replaced by shape-only stand-ins, and every call of a convolution entry is recorded with the shape
    that reaches it (the 3-channel stems arrive as NHWC4, the static same padding as part of the image)."""
    import torch
    from hifihr_amd import ops
    from hifihr_amd.effnet import EfficientNetB3
    from hifihr_amd.network import LightEstimator
    from hifihr_amd.perceptual import PerceptualLoss
    out, cur = [], [""]
    meta = lambda *shape: torch.empty(*shape, device="meta")

    def conv(x, w, stride, pad):
        (n, C, H, W), (K, _, R, S) = x.shape, w.shape
        out.append((cur[0], (n, H, W, C, K, R, S, stride, pad)))
        return meta(n, K, (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1)

    def conv2d(x, w, stride=1, pad=0, want_stats=False, fork=False):
        res = (conv(x, w, stride, pad),) + ((None,) if want_stats else ()) + ((x,) if fork else ())
        return res if len(res) > 1 else res[0]

    def dwconv2d(x, w, stride, pad4, want_stats=False):
        (n, C, H, W), k, (l, r, t, b) = x.shape, w.shape[-1], pad4
        y = meta(n, C, (H + t + b - k) // stride + 1, (W + l + r - k) // stride + 1)
        return (y, None) if want_stats else y

    def image_to_nhwc4(images, pad4=None, normalize=True):
        l, r, t, b = pad4 or (0, 0, 0, 0)
        return meta(images.shape[0], 4, images.shape[2] + t + b, images.shape[3] + l + r)

    stand_ins = dict(conv2d=conv2d, conv2d_bias_act=lambda x, w, bias, stride=1, pad=0, relu=True, **kw: conv(x, w, stride, pad),
                     dwconv2d=dwconv2d, image_to_nhwc4=image_to_nhwc4, bn_act=lambda x, *a, **kw: x, squeeze_excite=lambda x, *a: x,
                     maxpool2d=lambda x, k, s, p, relu_input=False: meta(x.shape[0], x.shape[1], (x.shape[2] + 2 * p - k) // s + 1, (x.shape[3] + 2 * p - k) // s + 1),
                     linear=lambda x, lin, act=None, bn=None: meta(x.shape[0], lin.out_features))
    kept = {name: getattr(ops, name) for name in stand_ins}
    try:
        for name, f in stand_ins.items():
            setattr(ops, name, f)
        runs = (("vgg19", PerceptualLoss(), lambda m: m.features(meta(N, 3, 224, 224))),
                ("light128", LightEstimator(128), lambda m: m(meta(N, 128, 28, 28))),
                ("light32", LightEstimator(32), lambda m: m(meta(N, 32, 56, 56))),
                ("effb3", EfficientNetB3(), lambda m: m.extract_features(meta(N, 3, 224, 224))))
        for tag, net, run in runs:
            net.eval()
            for name, m in net.named_modules():          # the tag of a recorded call: the module whose forward made it
                full = tag + "." + name.replace("model.", "").replace("base_layers.", "")
                m.register_forward_pre_hook(lambda mod, args, full=full: cur.__setitem__(0, full))
            with torch.no_grad():
                run(net)
    finally:
        for name, f in kept.items():
            setattr(ops, name, f)
    return out


def conv_line(lib, tag, g):
    N, H, W, C, K, R, S, stride, pad = g
    c = lib.c
    d = [lib.conv2d_describe(*g, direction) for direction in (0, 1, 2)]
    return (f"conv {tag} {g}: fwd={d[0]} dgrad={d[1]} wgrad={d[2]} ws_fwd={lib.conv2d_workspace_bytes(*g)} "
            f"ws_dgrad={lib.conv2d_workspace_bytes(*g, bwd_data=True)} ws_wgrad={lib.conv2d_wgrad_workspace_bytes(*g)} "
            f"dgrad_plus1x1={int(lib.conv2d_bwd_data_pre_plus1x1_supported(*g))} wgrad_plus1x1={int(lib.conv2d_bwd_weight_plus1x1_supported(*g))} "
            f"wgrad_c3={int(lib.conv2d_bwd_weight_c3_supported(N, H, W, K, R, S, stride, pad))} "
            f"c64_wino={int(lib.conv3x3_c64_wino_supported(N, H, W, C, K))} c64_bwd_pair={int(lib.conv3x3_c64_bwd_pair_supported(N, H, W))} "
            f"wino_tile={lib.wino_tile(N, H, W, C, K)} wino_parts={[lib.wino_wgrad_parts(N, H, W, C, K, m) for m in (2, 4)]} "
            f"wino_ws={[lib.wino_gemm_workspace_bytes(N, H, W, C, K, m) for m in (2, 4)]} "
            f"wino4_bwd_pair={int(c.hifihr_wino4_bwd_gemm_pair_supported(N, H, W, C, K))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hifihr_amd._lib import LIB_PATH, HifihrLib
    import test_gpu_conv
    import test_hostsim_conv_contract as contract
    lib = HifihrLib(args.lib or LIB_PATH)
    lines = []
    for g in contract.CONTRACT_GEOMS:
        lines.append(conv_line(lib, "contract", g))
    for g in contract.PAIR_GEOMS:
        lines.append(f"pair {g}: fwd_bnstats_pair={int(lib.conv2d_fwd_bnstats_pair_supported(*g))}")
    for (H, C, K, R, stride, pad) in test_gpu_conv.RESNET18_SHAPES:
        lines.append(conv_line(lib, "res18", (32, H, H, C, K, R, R, stride, pad)))
    for tag, g in module_convs(48):
        lines.append(conv_line(lib, tag, g))
    dims = (64, 128, 136, 192, 256, 512, 1392)
    for M in (50, 98, 1568, 6272, 25088):
        for N in dims:
            for K in dims:
                for batch in (1, 16, 36):
                    lines.append(f"gemm M={M} N={N} K={K} batch={batch}: nt={lib.bgemm_describe(False, M, N, K, batch)} "
                                 f"nt_ws={lib.bgemm_nt_workspace_bytes(M, N, K, batch)} tn={lib.bgemm_describe(True, N, K, M, batch)} "
                                 f"tn_parts={lib.bgemm_tn_parts(N, K, M, batch)}")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
