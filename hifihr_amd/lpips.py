"""LPIPS(net="alex"), version 0.1: the perceptual texture metric of the reference's evaluation pass
(`lpips.LPIPS(net="alex")` built at reference train_hrnet.py:563, called at :158 and averaged at :259-264).

Restated from the published definition (Zhang et al. 2018, the `lpips` package's v0.1 linear calibration):

    x            in0, in1 [N,3,H,W] in [-1, 1]
    scaling      (x - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
    trunk        torchvision AlexNet features[0:12]: conv(3->64, 11, s4, p2) ReLU | MaxPool(3, 2) conv(64->192, 5, p2) ReLU |
                 MaxPool(3, 2) conv(192->384, 3, p1) ReLU | conv(384->256, 3, p1) ReLU | conv(256->256, 3, p1) ReLU
    taps         the five ReLU outputs (C = 64, 192, 384, 256, 256); per tap and pixel n = f / (sqrt(sum_c f^2) + 1e-10),
                 d = sum_c w_c (n0_c - n1_c)^2 with the tap's 1x1 `lin` weights (no bias), then the mean of d over pixels
    value        the sum over the five taps, [N,1,1,1]

ONE path, on the GPU: both images go through the trunk as one batch of 2N -- the ScalingLayer inside the NCHW -> NHWC4 repack
(csrc/lpips.hip), the five convolutions on the f32-MFMA kernels with the bias + ReLU epilogue, the two pools on the tapless
inference pool, and one fused launch (+ a fixed-order finish) per tap that normalises both maps, takes the weighted squared
difference and the pixel mean.  No ATen kernel runs between the input and the result, nothing synchronises with the host.
The convolutions run inside ops.conv_precision(self.conv_precision): "reference" (default, the direct kernels: this is a
metric) or "fast" (Winograd for the three 3x3 layers).

Forward-only by default: an input that requires grad under enabled grad raises NotImplementedError (no silent fallback); a CPU
tensor raises; net != "alex" raises NotImplementedError.

LPIPS(differentiable=True) is the same module with a backward for the FIRST image (the opt-in loss term `lpips` of losses.py): in0 may
require grad, in1 is the target and may not (NotImplementedError).  The value is the forward-only module's bit for bit -- ONE custom
autograd.Function (ops._LPIPSAlex) runs the identical launches on the batch of 2N and keeps the maps; its backward slices in0's half out
of them, so the target's half passes through no backward kernel: per layer lpips_tap_bwd (with the layer's ReLU mask in its store),
backward-data with the frozen weights, and the tapless gather backward of the pools (csrc/lpips.hip).  Parameters stay frozen, the module stays in eval mode.

Weights: `load_state_dict_lpips` takes torchvision's `alexnet().state_dict()` plus the package's `alex.pth`, or the package's
full `LPIPS(net="alex").state_dict()`.  Neither can be downloaded here: without them the convolutions carry nn.Conv2d's default
initialisation and the lin layers non-negative `rand / C`, all drawn from a seeded generator (as PerceptualLoss does).
Parity with the `lpips` package itself and with the real weights is NOT pinned by any test of this repository -- the tests
compare against a float64 torch restatement of the definition above (tests/lpips_ref.py) with the same seeded weights.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (torchvision features index, slice of the package's `net`, cin, cout, kernel, stride, pad, MaxPool(3, 2) in front)
ALEX_LAYERS = ((0, 1, 3, 64, 11, 4, 2, False), (3, 2, 64, 192, 5, 1, 2, True), (6, 3, 192, 384, 3, 1, 1, True),
               (8, 4, 384, 256, 3, 1, 1, False), (10, 5, 256, 256, 3, 1, 1, False))
MIN_SIZE = 31          # 31 -> 7 (stem) -> 3 (pool) -> 1 (pool): every tap keeps at least one pixel


class LPIPS(nn.Module):
    def __init__(self, net="alex", conv_precision="reference", seed=0, differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)
        if net != "alex":
            raise NotImplementedError(f"LPIPS(net={net!r}): only 'alex' is built")
        if conv_precision not in ("reference", "fast"):
            raise ValueError(f"conv_precision: 'reference' or 'fast', not {conv_precision!r}")
        self.net, self.version, self.conv_precision = net, "0.1", conv_precision
        self.shift, self.scale = tuple(SHIFT), tuple(SCALE)
        gen = torch.Generator().manual_seed(seed)
        self.convs, self.lins = nn.ModuleList(), nn.ParameterList()
        from .network import Conv2dMFMA
        for (_, _, cin, cout, k, stride, pad, _) in ALEX_LAYERS:
            m = Conv2dMFMA(cin, cout, k, stride, pad, bias=True, relu=True)
            with torch.no_grad():              # nn.Conv2d's default initialisation, drawn in the standard NCHW order
                w = torch.empty(cout, cin, k, k)
                nn.init.kaiming_uniform_(w, a=math.sqrt(5), generator=gen)
                bound = 1.0 / math.sqrt(cin * k * k)
                m.weight.copy_(w)
                m.bias.copy_(torch.empty(cout).uniform_(-bound, bound, generator=gen))
            self.convs.append(m)
        for (_, _, _, cout, *_rest) in ALEX_LAYERS:
            self.lins.append(nn.Parameter(torch.rand(cout, generator=gen) / cout))          # non-negative, like the calibrated ones
        # the 3-channel stem filter zero-padded to the NHWC4 input the kernels read (rebuilt by load_state_dict_lpips)
        self.register_buffer("stem_w4", torch.zeros(64, 4, 11, 11).contiguous(memory_format=torch.channels_last), persistent=False)
        self._refresh()
        self.eval()
        for p in self.parameters():
            p.requires_grad_(False)

    def _refresh(self):
        with torch.no_grad():
            self.stem_w4.zero_()
            self.stem_w4[:, :3].copy_(self.convs[0].weight)

    def train(self, mode=True):                # a metric: always in evaluation mode
        return super().train(False)

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        """-> [N,1,1,1].  normalize=True: the inputs are in [0, 1] (the package rescales them to [-1, 1] first; here that is folded
        into the scaling constants)."""
        from . import ops
        from ._lib import require_cuda
        if self.differentiable and torch.is_grad_enabled() and in1.requires_grad:
            raise NotImplementedError("LPIPS(differentiable=True): the second image is the target, a constant -- detach it")
        require_cuda(in0, in1)
        if retPerLayer:
            raise NotImplementedError("LPIPS: retPerLayer is not built")
        wants_grad = torch.is_grad_enabled() and (in0.requires_grad or in1.requires_grad)
        if wants_grad and not self.differentiable:
            raise NotImplementedError("LPIPS is forward-only here (a metric): call it under torch.no_grad() or on detached inputs, "
                                      "or build LPIPS(differentiable=True)")
        if in0.dim() != 4 or in0.shape != in1.shape or in0.shape[1] != 3:
            raise ValueError(f"LPIPS: two [N,3,H,W] batches of one shape, not {tuple(in0.shape)} and {tuple(in1.shape)}")
        N, _, H, W = in0.shape
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS(alex): H, W >= {MIN_SIZE} (smaller inputs leave a tap without pixels), got {H} x {W}")
        shift, scale = self.shift, self.scale
        if normalize:                          # (2x - 1 - shift) / scale
            shift, scale = tuple((1.0 + s) / 2.0 for s in shift), tuple(s / 2.0 for s in scale)
        if wants_grad:                         # one autograd.Function: the same launches forward, the backward on in0's half alone
            with ops.conv_precision(self.conv_precision):
                return ops.lpips_alex(self, in0, in1, shift, scale).view(N, 1, 1, 1)
        with torch.no_grad(), ops.conv_precision(self.conv_precision):
            x = torch.empty((2 * N, 4, H, W), device=in0.device, dtype=torch.float32, memory_format=torch.channels_last)
            ops.image_scale_to_nhwc4(in0.detach().float(), shift, scale, out=x[:N])
            ops.image_scale_to_nhwc4(in1.detach().float(), shift, scale, out=x[N:])
            val = torch.empty(N, device=in0.device, dtype=torch.float32)
            for i, (m, lin, cfg) in enumerate(zip(self.convs, self.lins, ALEX_LAYERS)):
                if cfg[7]:
                    x = ops.maxpool2d_notap(x, 3, 2, 0)
                x = ops.conv2d_bias_act(x, self.stem_w4 if i == 0 else m.weight, m.bias, m.stride, m.pad, True)
                ops.lpips_tap(x[:N], x[N:], lin, val, accumulate=i > 0)
        return val.view(N, 1, 1, 1)


def _pick(merged, names):
    for n in names:
        if n in merged:
            return merged[n]
    raise KeyError(f"LPIPS state dict lacks {names[0]!r}" + (f" (or {', '.join(repr(n) for n in names[1:])})" if len(names) > 1 else ""))


def load_state_dict_lpips(module: LPIPS, *state_dicts):
    """Loads the AlexNet trunk and the five `lin` layers into `module` from one or more state dicts, merged in order:
      * torchvision's `alexnet().state_dict()` (`features.<i>.weight/bias`; classifier keys are ignored) together with the
        package's `alex.pth` (`lin<i>.model.1.weight`, [1,C,1,1]);
      * or the package's full `LPIPS(net="alex").state_dict()` (`net.slice<j>.<i>.weight/bias`, `lin<i>.model.1.weight`,
        `scaling_layer.shift/scale`; the scaling constants are taken from it when present).
    A missing tensor raises KeyError naming it; nothing is changed in that case."""
    merged = {}
    for sd in state_dicts:
        merged.update(sd)
    picked = []
    for li, (fi, sj, cin, cout, k, *_rest) in enumerate(ALEX_LAYERS):
        w = _pick(merged, (f"features.{fi}.weight", f"net.slice{sj}.{fi}.weight"))
        b = _pick(merged, (f"features.{fi}.bias", f"net.slice{sj}.{fi}.bias"))
        lin = _pick(merged, (f"lin{li}.model.1.weight", f"lins.{li}.model.1.weight"))
        if tuple(w.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,) or lin.numel() != cout:
            raise ValueError(f"LPIPS layer {li}: shapes {tuple(w.shape)}, {tuple(b.shape)}, {tuple(lin.shape)} do not fit AlexNet")
        picked.append((w, b, lin))
    with torch.no_grad():
        for m, p, (w, b, lin) in zip(module.convs, module.lins, picked):
            m.weight.copy_(w)
            m.bias.copy_(b)
            p.copy_(lin.reshape(-1))
        module._refresh()
    if "scaling_layer.shift" in merged and "scaling_layer.scale" in merged:
        module.shift = tuple(float(v) for v in merged["scaling_layer.shift"].reshape(-1))
        module.scale = tuple(float(v) for v in merged["scaling_layer.scale"].reshape(-1))
    return module


def load_lpips_weights(module: LPIPS, *paths):
    """`load_state_dict_lpips` from files (torch.load, map_location="cpu"): the value of --lpips_weights."""
    return load_state_dict_lpips(module, *[torch.load(p, map_location="cpu") for p in paths])
