"""Torch restatement of LPIPS(net="alex"), version 0.1, written from the published definition (the tests' reference for
hifihr_amd/lpips.py and csrc/lpips.hip; runs on the CPU in any floating dtype).  Not a copy of the `lpips` package, which is not
available here: parity with the package itself is unpinned.

    scaling   (x - shift) / scale
    trunk     torchvision AlexNet features[0:12]
    tap       n = f / (sqrt(sum_c f^2) + 1e-10);  d = sum_c w_c (n0_c - n1_c)^2;  mean over pixels
    value     sum over the five taps, [N,1,1,1]
"""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (cin, cout, kernel, stride, pad, MaxPool2d(3, 2) in front)
ALEX = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))


def tap_ref(f0, f1, w):
    """One tap on channels-last maps f0, f1 [B, HW, C] and lin weights w [C] -> [B], in the dtype of the inputs."""
    n0 = f0 / (f0.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    return ((n0 - n1).pow(2) * w).sum(-1).mean(-1)


def module_weights(m):
    """(convs [(w [K,C,R,S], b [K])], lins [w [C]]) of a hifihr_amd.lpips.LPIPS as float64 CPU tensors."""
    convs = [(c.weight.detach().cpu().double().contiguous(), c.bias.detach().cpu().double()) for c in m.convs]
    return convs, [p.detach().cpu().double() for p in m.lins]


def lpips_alex_ref(in0, in1, convs, lins, dtype=torch.float64, shift=SHIFT, scale=SCALE):
    """-> [N,1,1,1] in `dtype` on the CPU."""
    sh = torch.tensor(shift, dtype=dtype).view(1, 3, 1, 1)
    sc = torch.tensor(scale, dtype=dtype).view(1, 3, 1, 1)
    N = in0.shape[0]
    x = torch.cat([(in0.detach().cpu().to(dtype) - sh) / sc, (in1.detach().cpu().to(dtype) - sh) / sc])
    val = torch.zeros(N, dtype=dtype)
    for (w, b), lin, (_, _, _, stride, pad, pool) in zip(convs, lins, ALEX):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), stride=stride, padding=pad))
        f = x.permute(0, 2, 3, 1).reshape(2 * N, -1, x.shape[1])
        val = val + tap_ref(f[:N], f[N:], lin.to(dtype))
    return val.view(N, 1, 1, 1)


def make_tap_inputs(B, HW, C, seed=0, identical_sample=None):
    """Non-negative maps [B, HW, C] (float32) with about 10 % all-zero pixels in f0 only, in both, or in f1 only, and
    (identical_sample = b) one sample whose two maps are the same tensor values; + non-negative w [C]."""
    gen = torch.Generator().manual_seed(seed)
    f0 = torch.rand(B, HW, C, generator=gen)
    f1 = torch.rand(B, HW, C, generator=gen)
    f0 = torch.where(torch.rand(B, HW, C, generator=gen) < 0.3, torch.zeros(()), f0)        # post-ReLU maps: many exact zeros
    f1 = torch.where(torch.rand(B, HW, C, generator=gen) < 0.3, torch.zeros(()), f1)
    r = torch.rand(B, HW, generator=gen)
    f0[r < 0.07] = 0.0                                    # zero in f0 (r < .035: f0 alone; .035 <= r < .07: both)
    f1[(r >= 0.035) & (r < 0.105)] = 0.0                  # zero in both, or (.07 <= r < .105) in f1 alone
    if identical_sample is not None:
        f1[identical_sample] = f0[identical_sample]
    w = torch.rand(C, generator=gen) / C
    return f0.contiguous(), f1.contiguous(), w
