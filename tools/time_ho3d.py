"""Times hifihr_ho3d_batch (csrc/augment.hip) at the largest production crop: B samples of a 640 x 480 frame, every window 800 pixels
(640 / 0.8, the most hifihr_amd.data.ho3d_crop_windows makes) resized to out_size 224.
usage: python tools/time_ho3d.py [--lib other.so] [B]   -> average us over 200 calls (three launches each) and a checksum of the pixels,
so that two builds can be compared output for output."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hifihr_amd._lib import LIB_PATH, HifihrLib   # noqa: E402

args = sys.argv[1:]
path = LIB_PATH
if args and args[0] == "--lib":
    path, args = args[1], args[2:]
B = int(args[0]) if args else 32
S, n, FH, FW = 224, 8, 480, 640
lib = HifihrLib(path)
dev = "cuda"
rng = np.random.default_rng(0)
frames = torch.from_numpy(rng.integers(0, 256, (n, FH, FW, 4), dtype=np.uint8)).to(dev).view(torch.int32).reshape(n, FH, FW)
masks = torch.from_numpy((rng.random((n, FH, FW)) > 0.5).astype(np.uint8) * 255).to(dev)
Ks = torch.eye(3).repeat(n, 1, 1).to(dev)
uv, xyz = torch.rand(n, 21, 2, device=dev) * 640, torch.randn(n, 21, 3, device=dev)
x0, y0 = rng.integers(-160, 1, B), rng.integers(-320, 1, B)
boxes = np.stack([x0, y0, x0 + 800, y0 + 800], 1).astype(np.int32)
win = np.concatenate([rng.uniform(100, 500, (B, 2)), np.full((B, 1), 0.28)], 1).astype(np.float32)
packed = torch.from_numpy(np.concatenate([rng.integers(0, n, B).astype(np.int32), boxes.reshape(-1), win.reshape(-1).view(np.int32)])).to(dev)
ws = torch.empty(lib.ho3d_workspace_bytes(B, S) // 4 + 1, dtype=torch.int32, device=dev)
out = {"img_crop": torch.empty(B, 3, S, S, device=dev), "hand_mask_crop": torch.empty(B, 1, S, S, device=dev), "K_crop": torch.empty(B, 3, 3, device=dev),
       "uv21_crop": torch.empty(B, 21, 2, device=dev), "xyz21": torch.empty(B, 21, 3, device=dev)}
call = lambda: lib.ho3d_batch(frames, masks, Ks, uv, xyz, packed, B, S, ws, out)
for _ in range(20):
    call()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
runs = []
for _ in range(5):
    e0.record()
    for _ in range(200):
        call()
    e1.record(); torch.cuda.synchronize()
    runs.append(e0.elapsed_time(e1) * 1e3 / 200)
check = float(out["img_crop"].double().sum()), float(out["hand_mask_crop"].double().sum())
print(f"ho3d_batch B={B} 800 -> {S} [{os.path.basename(path)}]: " + " ".join(f"{r:7.1f}" for r in runs) + f" us per call (5 x 200 calls); pixel sums {check[0]:.6f} {check[1]:.1f}")
