#!/usr/bin/env python3
"""Headline benchmark: training-step images/sec on FreiHAND-shaped 224x224 batches (BASELINE.json configs[1]:
batch 32 per GPU, ResNet-18 encoder + MANO LBS + render + silhouette/texture losses), one process per GPU.

  python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: bench.py starts the N ranks itself, `launch_ranks`)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

One step = the whole training iteration on a NEW batch: the batch is assembled on the device from the uint8 sample cache resident
in HBM (hifihr_amd/data.py:batch_examples -> hifihr_freihand_batch: gather + affine warp + the K / joint / vertex / projection terms
of `data_dic`) straight into the captured step's static inputs, then forward + losses + backward + fused Adam (one hipGraph replay at N = 1).

Rank 0 prints ONE JSON line: `metric`, `value` (images/sec), `unit`, `higher_is_better`, `dtype` and `ms_per_step` (milliseconds of
one timed step; `--steps` of them are timed).  A plain run does only what that line needs: set-up, `--warmup` steps, the timed steps.

  --dump-outputs DIR   after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32): the loss, every
                       term of the loss dictionary and the parameters after the optimizer step (a fixed, seeded sample of them when
                       the model has more than 2^23).  The inputs depend on the arguments only, so two builds can be compared output
                       for output.
  --full               everything else, behind the timed steps as before: the same step on one resident batch (`resident_batch`),
                       `roofline` for the dominant hand-written kernel of the step (by time per step, measured here),
                       `roofline_kernels` for every MFMA kernel of the convolution path, `roofline_render_fwd`, `roofline_render_bwd`,
                       `roofline_mano_lbs` (the north star's HBM-bound kernels), the per-bucket all-reduce times at N > 1 and, at
                       N = 1, `cpu_baseline` (the oracle step timed on the host cores on a bounded sample).  `--no-rooflines` and
                       `--no-cpu-baseline` leave parts of it out.
"""
import argparse
import hashlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import torch
import torch.distributed as dist

MFMA_PEAK_TF = 157.3       # dense f32 matrix peak (MI355X_MICROARCH.md); the pipe sustains 155 in a register-only loop (tools/mfma_peak.hip)
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch (BASELINE configs[1]: 32)")
    ap.add_argument("--encoder", default="res18", choices=["res18", "res50", "res101", "effb3"], help="res18 = BASELINE configs[1] (headline)")
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 5],
                    help="2 = BASELINE configs[1] (headline); 3 = configs[2] full_rhd_freihand.json: effb3, batch 48, texture + "
                         "perceptual losses; 5 = configs[4] HO-3D weak supervision, 512^2 render, batch 16 per GPU (MANO + texture "
                         "stand-in for the unavailable NIMBLE layer in both; not headline lines)")
    ap.add_argument("--hand", default="mano", choices=["mano", "nimble-synthetic", "nimble-synthetic-uv"],
                    help="configs 3 / 5 only: the hand layer.  mano = MANO + vertex-colour texture stand-in; nimble-synthetic = the NIMBLE-SHAPED layer "
                         "(5 990 skin vertices / 11 976 faces, 25 joints, 20 / 30 / 10 PCA) on seeded synthetic tables; -uv = its texture as an "
                         "image sampled through per-face uvs (TexturesUV).  The real NIMBLE tables are absent: parity unpinned, declared")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: resident-batch replay, rooflines, per-bucket all-reduce "
                         "times, CPU baseline (see the module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (loss, loss terms, parameters) to DIR/<name>.npy as float32")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-rooflines", action="store_true",
                    help="with --full: skip the roofline block behind the timed region (the rocprofv3 trace then ends with the timed replays)")
    ap.add_argument("--graph", type=int, default=-1, help="0: eager; -1 or 1: hipGraph replay (N = 1: whole step; N > 1: the fastest of the data-parallel forms in a "
                    "short trial); 2: force the N > 1 form (one graph, then all-reduce + Adam); 3: force the segmented form (backward as one graph "
                    "launch per trunk segment, each bucket exchanged beside the next segment)")
    ap.add_argument("--cpu-batch", type=int, default=32, help="sample size of the CPU baseline (images; SURVEY 8d: the batch of 32)")
    ap.add_argument("--cpu-steps", default="1,3", help="warm-up,timed oracle steps of the CPU baseline.  SURVEY 8d names 3,10: at ~21 s per B = 32 "
                    "step on the GPU box's host that is ~4.5 minutes, against the contract's bounded sample (10-30 s of CPU work) and a default "
                    "run that ends within minutes; the default times 3 steps after 1 and reports their spread")
    ap.add_argument("--cache", type=int, default=256, help="synthetic samples in the device-resident uint8 cache")
    ap.add_argument("--aa", type=int, default=3, help="renderer anti-aliasing factor (config 5 also reports aa = 1)")
    return ap.parse_args()


def hip_us(fn, n=10, warm=3, groups=3):
    """Average duration of `fn`'s launches: HIP events around n BACK-TO-BACK calls on torch's current stream (the stream the
    C-ABI launches on).  Inside a replayed graph a single kernel cannot be bracketed; a bracket around one eager launch also counts
    the host's launch latency.  `groups` such brackets, the smallest average reported: one disturbed bracket (a clock dip after host
    work, an unrelated event on the box) once quadrupled a 22 us entry and moved the dominant kernel's fraction from 0.60 to 0.56."""
    for _ in range(warm):
        fn()
    best = None
    for _ in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / n
        best = us if best is None else min(best, us)
    return best


def _norm_kernel(name):
    """'void hifihr::bgemm_tn_kernel<64, 64>(hifihr::BgemmArgs)' -> 'bgemm_tn_kernel<64,64>' (the form csrc's *_describe entry points use)."""
    n = name.strip()
    if n.startswith("void "):
        n = n[5:]
    depth, cut = 0, len(n)
    for i, ch in enumerate(n):                      # cut at the argument list: the first '(' outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    return n[:cut].replace("hifihr::", "").replace(" ", "")


def instep_kernel_times(step_fn, nsteps=3):
    """Per-kernel device time INSIDE the training step: roctracer (torch.profiler) over `nsteps` eager steps -- every kernel of the step
    in its real order, with the caches in the state the step leaves them in (a bracket around back-to-back launches of one entry point
    times warm tables and, for entries that launch helper kernels, more than the kernel).  -> {normalised kernel name: (launches per
    step, us per step)} or None when the profiler is unavailable."""
    done = [0]

    def counted():
        done[0] += 1                                 # (before the call: a step that raised has issued some of its collectives)
        return step_fn()
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(nsteps):
                counted()
            torch.cuda.synchronize()
        acc = {}
        for e in prof.events():
            if e.device_type != torch.autograd.DeviceType.CUDA:
                continue
            nm = _norm_kernel(e.name)
            if not nm or nm.lower().startswith(("memcpy", "memset")) or "Memcpy" in nm or "Memset" in nm:
                continue
            dur = getattr(e, "device_time", None)
            if dur is None:
                dur = e.cuda_time
            c, t = acc.get(nm, (0, 0.0))
            acc[nm] = (c + 1, t + float(dur))
        return {k: (c / nsteps, t / nsteps) for k, (c, t) in acc.items()} or None
    except Exception as ex:                          # measurement aid only
        print(f"[bench] in-step kernel profile unavailable: {type(ex).__name__}: {ex}", file=sys.stderr)
        while done[0] < nsteps:                      # data parallel: the other ranks run exactly `nsteps` steps beside this one
            counted()
        return None


def instep_lookup(prof, name):
    """(launches per step, us per step) of every profiled kernel whose normalised name starts with `name` (template arguments included
    when `name` carries them), or None."""
    if not prof:
        return None
    key = name.replace(" ", "")
    hits = [(c, t) for k, (c, t) in prof.items() if k == key or k.startswith(key + "<") or k.startswith(key)]
    if not hits:
        return None
    return sum(c for c, _ in hits), sum(t for _, t in hits)


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(args_ns, examples, tables, nimg, render_frames=8, steps=(1, 3)):
    """The oracle training step (oracle/model_oracle.py) on the host cores, on `nimg` images of the same batch: `steps[0]` untimed
    warm-up steps, then `steps[1]` timed ones, each timed on its own so the line carries their spread (B = 32, all host
    cores, 3 + 10 iterations = `--cpu-steps 3,10`; the default 1 + 3 keeps the default run within minutes) -- and the renderer
    alone (oracle/render_oracle.render: the C rasteriser of oracle/raster_oracle.c + torch shading / resolve), forward and
    forward + backward, on `render_frames` meshes of the batch, as milliseconds per frame."""
    from oracle import render_oracle as ro
    from oracle.model_oracle import OracleModel, oracle_step
    torch.manual_seed(0)
    model = OracleModel(tables).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-6)
    ex = {k: (v[:nimg].detach().cpu() if torch.is_tensor(v) else v) for k, v in examples.items()}
    nwarm, ntimed = max(1, int(steps[0])), max(1, int(steps[1]))
    for _ in range(nwarm):
        oracle_step(model, ex, args_ns, opt)               # warm-up (allocator, OpenMP pools, oneDNN primitives)
    per = []
    for _ in range(ntimed):
        t0 = time.time()
        oracle_step(model, ex, args_ns, opt)
        per.append(time.time() - t0)
    dt, nstep = sum(per), len(per)
    out = {"value": nimg * nstep / dt, "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port", "cpu": cpu_model_name(),
           "step_s": [round(t, 3) for t in per], "spread": round((max(per) - min(per)) / (dt / nstep), 4),
           "sample": f"{nwarm} warm-up + {nstep} timed oracle training steps (torch-CPU encoder and heads, oracle MANO LBS, the C rasteriser of "
                     f"oracle/raster_oracle.c (OpenMP over sample rows, all host threads) + torch shading / losses, torch Adam) on {nimg} images "
                     f"of the same synthetic batch, {dt:.1f} s timed, per-step times in `step_s` ((max - min) / mean = `spread`)"
                     + ("; SURVEY 8d's 3 + 10 would be ~4.5 min of CPU work in the default run: `--cpu-steps 3,10` runs it" if (nwarm, nstep) != (3, 10) else "")}
    # the renderer alone, on the ground-truth meshes of the first frames of the batch (camera space, the size the hands have on screen)
    verts = ex["verts"][:render_frames].float()
    nf = verts.shape[0]
    cam = ro.ndc_camera_from_K(ex["Ps"][:nf], 224.0)
    faces = torch.as_tensor(tables.faces.astype("int64"))
    col = torch.full_like(verts, 0.7); lc = torch.full((nf, 3), 0.6); ld = torch.tensor([[0.0, 0.0, -1.0]]).repeat(nf, 1)

    def fwd(need_grad):
        v = verts.clone().requires_grad_(need_grad)
        return v, ro.render(v, col, cam, lc, ld, faces, image_size=224, aa=3)[0]
    fwd(False)
    t0 = time.time()
    for _ in range(2):
        fwd(False)
    t_f = (time.time() - t0) / 2
    v, img = fwd(True); img.sum().backward()
    t0 = time.time()
    for _ in range(2):
        v, img = fwd(True); img.sum().backward()
    t_fb = (time.time() - t0) / 2
    out["render_ms_per_frame"] = {"fwd": t_f / nf * 1e3, "fwd+bwd": t_fb / nf * 1e3, "frames": nf, "image_size": 224, "aa": 3,
                                  "note": "oracle/render_oracle.render (C rasteriser with OpenMP + torch shading, autograd backward), 1 warm-up + 2 timed calls"}
    return out


def build_cache(model, n, first_index, dev):
    """A synthetic FreiHAND-shaped sample set resident in HBM as uint8 (hifihr_amd/data.py), made of seeded synthetic samples."""
    import numpy as np
    from hifihr_amd import synth
    from hifihr_amd.data import FreiHandDeviceCache
    imgs, masks, Ks, joints, verts = [], [], [], [], []
    for lo in range(0, n, 64):
        s = synth.make_batch(getattr(model, "data_mano", None) or model.hand_layer.handle, getattr(model, "data_renderer", None) or model.renderer_p3d,
                             min(64, n - lo), first_index=first_index + lo, device=dev)
        imgs.append((s["trans_images"].permute(0, 2, 3, 1) * 255.0).round().clamp(0, 255).to(torch.uint8))
        masks.append((s["trans_masks"][:, 0] * 255.0).to(torch.uint8))
        Ks.append(s["trans_Ks"]); joints.append(s["trans_joints"]); verts.append(s["trans_verts"])
    cat = lambda xs: torch.cat(xs, 0)
    return FreiHandDeviceCache(cat(imgs), cat(masks), cat(Ks), cat(joints), cat(verts), device=dev)


def csrc_digest():
    """Digest of the kernel sources: a PMC traffic file is only used when it was measured on THIS tree's kernels."""
    h = hashlib.sha256()
    d = os.path.join(REPO, "hifihr_amd", "csrc")
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".h")):
            h.update(open(os.path.join(d, fn), "rb").read())
    return h.hexdigest()[:16]


_TRAFFIC_OK = True        # main() clears it when the workload is not the one the counter file was measured on (B = 32, res18, config 2)


def measured_traffic(kernel_key):
    """HBM bytes per launch from the PMC counters (separate FETCH_SIZE / WRITE_SIZE rocprofv3 passes over this command,
    tools/kernel_traffic.sh -> profiles/r<NN>_kernel_traffic.json), or None when no measurement of this tree's kernels exists."""
    if not _TRAFFIC_OK:
        return None
    import glob
    dig = csrc_digest()
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "r*_kernel_traffic.json")), reverse=True):      # newest round first
        j = json.load(open(f))
        if j.get("csrc_digest") == dig:
            return j.get("traffic_bytes_per_launch", {}).get(kernel_key)
    return None


def conv_path_rooflines(ops, lib, dev, nprof, prof=None, prof_how="roctracer (torch.profiler) over 3 eager steps"):
    """Every MFMA kernel of the convolution path: each distinct (shape, direction) the profiled steps launched is timed with HIP
    events over 10 back-to-back launches on tensors of that shape and weighted by launches per step.  FLOPs are the ones the kernel
    EXECUTES (Winograd GEMMs: 2 M N K per product).  Returns {kernel name as rocprof lists it: entry}."""
    from collections import Counter
    table = {}

    def add(name, per_step, us, flop, nbytes, what="", useful=None):
        """flop: what the kernel EXECUTES; useful: the part of it that lands in rows carrying data (the TN products of the mosaic layers
        walk the 480 allocated rows of which 450 hold tiles: the padding rows are zeros) -- defaults to flop."""
        e = table.setdefault(name, {"launches_per_step": 0.0, "us_per_step": 0.0, "flop_per_step": 0.0, "useful_flop_per_step": 0.0,
                                    "compulsory_bytes_per_step": 0.0, "shapes": []})
        e["launches_per_step"] += per_step; e["us_per_step"] += us * per_step
        e["flop_per_step"] += flop * per_step; e["compulsory_bytes_per_step"] += nbytes * per_step
        e["useful_flop_per_step"] += (flop if useful is None else useful) * per_step
        e["shapes"].append({"shape": what, "launches_per_step": per_step, "us": round(us, 1), "TFLOPs": round(flop / us / 1e6, 1)})
    for (geom, direction), cnt in Counter(ops.PROFILE.conv_log).items():
        per_step = cnt / nprof
        if direction == "gemm-pair":
            # backward-data + backward-weight products of one F(4x4) layer (C_ -> K_ channels) in ONE launch (bgemm_nt_tn_pair_kernel); a
            # product the library declines to pair (too long) falls back to the two launches inside the same entry point: priced the same way
            _, N_, H_, W_, C_, K_, m_ = geom
            P_ = (m_ + 2) ** 2
            T_ = lib.wino_tiles(N_, H_, W_, m_); Tc = lib.wino_tiles_computed(N_, H_, W_, m_)
            parts = lib.wino_wgrad_parts(N_, H_, W_, C_, K_, m_)
            V2 = torch.randn(P_ * T_ * K_, device=dev); U2 = torch.randn(P_ * C_ * K_, device=dev) * 0.05; M2 = torch.empty(P_ * T_ * C_, device=dev)
            Vx = torch.randn(P_ * T_ * C_, device=dev); Yt = torch.randn(P_ * T_ * K_, device=dev); dU = torch.empty(parts * P_ * K_ * C_, device=dev)
            us = hip_us(lambda: lib.wino4_bwd_gemm_pair(V2, U2, M2, Vx, Yt, dU, N_, H_, W_, C_, K_, parts))
            # the TN half skips the k-steps (4 rows each) of the zero rows behind the last tile mosaic (round 6): it EXECUTES ceil(Tc / 4) * 4
            # of the T_ allocated rows (HIFIHR_GEMM_TN_SKIP=0: all of them)
            Tx = T_ if os.environ.get("HIFIHR_GEMM_TN_SKIP", "1") == "0" else min(T_, (Tc + 3) // 4 * 4)
            add("bgemm_nt_tn_pair_kernel", per_step, us, 2.0 * P_ * (Tc + Tx) * C_ * K_,
                4.0 * P_ * ((Tc * K_ + C_ * K_ + Tc * C_) + (T_ * C_ + T_ * K_ + parts * K_ * C_)),
                f"{P_} x ([{Tc} x {K_}] . [{C_} x {K_}]^T  +  [{Tx} of {T_} x {K_}]^T . [{Tx} of {T_} x {C_}], {parts} slab(s))",
                useful=2.0 * P_ * (Tc + Tc) * C_ * K_)
            continue
        if direction in ("gemm", "gemm-tn"):
            _, N_, H_, W_, C_, K_, m_ = geom                    # m_: Winograd output-tile edge (2: 16 positions, 4: 36)
            P_ = (m_ + 2) ** 2
            T_ = lib.wino_tiles(N_, H_, W_, m_)                 # (mosaic tiles on the 14 x 14 layers: 480 rows allocated, 450 computed)
            V = torch.randn(P_ * T_ * C_, device=dev)
            if direction == "gemm":
                U = torch.randn(P_ * K_ * C_, device=dev) * 0.05; M = torch.empty(P_ * T_ * K_, device=dev)
                name = lib.bgemm_describe(False, T_, K_, C_, P_)
                if not name:                       # shape outside csrc/gemm.hip: runs on the gather kernel
                    name = "conv_igemm_kernel"
                nb = lib.wino_gemm_workspace_bytes(N_, H_, W_, C_, K_, m_)
                ws = torch.zeros(nb // 4 + 64, device=dev) if nb else None
                us = hip_us(lambda: lib.wino_gemm(V, U, M, N_, H_, W_, C_, K_, ws=ws, m=m_))
                Tc = lib.wino_tiles_computed(N_, H_, W_, m_)    # rows the product walks (the mosaic count before its rounding)
                add(name, per_step, us, 2.0 * P_ * Tc * C_ * K_, 4.0 * P_ * (Tc * C_ + K_ * C_ + Tc * K_), f"{P_} x [{Tc} x {C_}] . [{K_} x {C_}]^T")
            else:
                Y = torch.randn(P_ * T_ * K_, device=dev)
                parts = lib.wino_wgrad_parts(N_, H_, W_, C_, K_, m_)
                if parts > 0:
                    name = lib.bgemm_describe(True, K_, C_, T_, P_)
                    dU = torch.empty(parts * P_ * K_ * C_, device=dev)
                    us = hip_us(lambda: lib.wino_wgrad_gemm_parts(V, Y, dU, N_, H_, W_, C_, K_, parts, m_))
                else:
                    name = "conv_wgrad_kernel"
                    dU = torch.zeros(16 * K_ * C_, device=dev)
                    us = hip_us(lambda: lib.wino_wgrad_gemm(V, Y, dU, N_, H_, W_, C_, K_))
                Tc = lib.wino_tiles_computed(N_, H_, W_, m_)
                Tx = min(T_, (Tc + 3) // 4 * 4) if (name == "bgemm_tn_rows_kernel" and m_ == 4 and os.environ.get("HIFIHR_GEMM_TN_SKIP", "1") != "0") else T_
                add(name, per_step, us, 2.0 * P_ * Tx * C_ * K_, 4.0 * P_ * (T_ * C_ + T_ * K_ + max(parts, 1) * K_ * C_),
                    f"{P_} x [{Tx} of {T_} x {K_}]^T . [{Tx} of {T_} x {C_}], {max(parts, 1)} slab(s)",
                    useful=2.0 * P_ * Tc * C_ * K_)
            continue
        if direction == "fwd-pair":            # bgemm_nt_rows_pair2_kernel: conv1 (3x3, pad 1) + downsample[0] (1x1) of a stage's first block, one launch
            _, N_, H_, W_, C_, K1_, K2_, st_ = geom
            OH_, OW_ = (H_ + 2 - 3) // st_ + 1, (W_ + 2 - 3) // st_ + 1
            x = torch.randn(N_, H_, W_, C_, device=dev); w1 = torch.randn(K1_, 3, 3, C_, device=dev) * 0.05; w2 = torch.randn(K2_, 1, 1, C_, device=dev) * 0.05
            y1 = torch.empty(N_, OH_, OW_, K1_, device=dev); y2 = torch.empty(N_, OH_, OW_, K2_, device=dev)
            s1 = torch.zeros(lib.bn_stats_floats(K1_), device=dev); s2 = torch.zeros(lib.bn_stats_floats(K2_), device=dev)
            us = hip_us(lambda: lib.conv2d_fwd_bnstats_pair(x, w1, y1, s1, K1_, 3, 1, w2, y2, s2, K2_, 1, 0, N_, H_, W_, C_, st_))
            add("bgemm_nt_rows_pair2_kernel", per_step, us, 2.0 * N_ * OH_ * OW_ * C_ * (9 * K1_ + K2_),
                4.0 * (N_ * H_ * W_ * C_ + (9 * K1_ + K2_) * C_ + N_ * OH_ * OW_ * (K1_ + K2_)),
                f"fwd N{N_} {H_}x{W_} C{C_}: 3x3 s{st_} ->K{K1_}  +  1x1 s{st_} ->K{K2_}, one launch")
            continue
        N_, H_, W_, C_, K_, R_, S_, st_, pd_ = geom
        if direction in ("fwd-wino2", "dgrad-wino2"):          # conv_wino2_kernel: one launch, 2 x 16 x (tiles x 64 x 64) executed products
            x = torch.randn(N_, H_, W_, 64, device=dev); U = torch.randn(16 * 64 * 64, device=dev) * 0.05; y = torch.empty(N_, H_, W_, 64, device=dev)
            us = hip_us(lambda: lib.conv3x3_c64_wino(x, U, None, False, y, None, N_, H_, W_))
            add("conv_wino2_kernel", per_step, us, 2.0 * 16 * (N_ * H_ * W_ / 4) * 64 * 64, 4.0 * (2 * N_ * H_ * W_ * 64 + 16 * 64 * 64),
                f"{direction} N{N_} {H_}x{W_} 64->64 3x3 as F(2x2, 3x3), transforms in registers")
            continue
        if direction == "c64-pair":            # conv_c64_bwd_pair_kernel: F(2x2) data gradient + direct (9-tap) weight gradient in one launch
            x = torch.randn(N_, H_, W_, 64, device=dev); U = torch.randn(16 * 64 * 64, device=dev) * 0.05; gy = torch.randn(N_, H_, W_, 64, device=dev)
            dx = torch.empty(N_, H_, W_, 64, device=dev); dw = torch.zeros(64, 3, 3, 64, device=dev)
            us = hip_us(lambda: lib.conv3x3_c64_bwd_pair(gy, U, None, dx, x, dw, N_, H_, W_))
            add("conv_c64_bwd_pair_kernel", per_step, us, 2.0 * 16 * (N_ * H_ * W_ / 4) * 64 * 64 + 2.0 * N_ * H_ * W_ * 64 * 9 * 64,
                4.0 * (3 * N_ * H_ * W_ * 64 + 16 * 64 * 64 + 9 * 64 * 64),
                f"N{N_} {H_}x{W_} 64->64 3x3: data gradient as F(2x2, 3x3) + weight gradient (9 taps, pixel reduction), one launch")
            continue
        OH_, OW_ = (H_ + 2 * pd_ - R_) // st_ + 1, (W_ + 2 * pd_ - S_) // st_ + 1
        x = torch.randn(N_, H_, W_, C_, device=dev); w = torch.randn(K_, R_, S_, C_, device=dev) * 0.05
        y = torch.randn(N_, OH_, OW_, K_, device=dev)
        flop = 2.0 * N_ * OH_ * OW_ * K_ * R_ * S_ * (3 if C_ == 4 else C_)          # the NHWC4 stem has 3 real channels
        nbytes = 4.0 * (N_ * H_ * W_ * C_ + K_ * R_ * S_ * C_ + N_ * OH_ * OW_ * K_)     # input, weights, output once each
        if direction == "wgrad+1x1":           # conv_wgrad_kernel: the strided 3x3 weight gradient with the downsample 1x1's column tiles in the same launch
            dw = torch.zeros(K_, R_, S_, C_, device=dev); dw2 = torch.zeros(K_, C_, device=dev); y2 = torch.randn(N_, OH_, OW_, K_, device=dev)
            us = hip_us(lambda: lib.conv2d_bwd_weight_plus1x1(x, y, dw, y2, dw2, N_, H_, W_, C_, K_, R_, S_, st_, pd_))
            add(lib.conv2d_describe(N_, H_, W_, C_, K_, R_, S_, st_, pd_, 2), per_step, us, flop + 2.0 * N_ * OH_ * OW_ * K_ * C_,
                nbytes + 4.0 * (N_ * OH_ * OW_ * K_ + K_ * C_), f"wgrad N{N_} {H_}x{W_} C{C_}->K{K_} {R_}x{S_} s{st_}  +  1x1 s{st_} of the same input, one launch")
            continue
        if direction == "wgrad":
            dw = torch.zeros(K_, R_, S_, C_, device=dev)
            us = hip_us(lambda: lib.conv2d_bwd_weight(x, y, dw, N_, H_, W_, C_, K_, R_, S_, st_, pd_))
            add(lib.conv2d_describe(N_, H_, W_, C_, K_, R_, S_, st_, pd_, 2), per_step, us, flop, nbytes, f"wgrad N{N_} {H_}x{W_} C{C_}->K{K_} {R_}x{S_} s{st_}")
            continue
        if direction == "dgrad+1x1":           # conv_igemm_kernel: the strided 3x3 backward-data with the downsample 1x1's as a tap of class (0, 0)
            wt = torch.empty(w.numel(), device=dev); lib.weight_transpose(w, wt, K_, R_ * S_, C_)
            y2 = torch.randn(N_, OH_, OW_, K_, device=dev); wt2 = torch.randn(C_, K_, device=dev) * 0.05
            us = hip_us(lambda: lib.conv2d_bwd_data_pre_plus1x1(y, wt, y2, wt2, x, N_, H_, W_, C_, K_, R_, S_, st_, pd_))
            add(lib.conv2d_describe(N_, H_, W_, C_, K_, R_, S_, st_, pd_, True), per_step, us, flop + 2.0 * N_ * OH_ * OW_ * K_ * C_,
                nbytes + 4.0 * (N_ * OH_ * OW_ * K_ + K_ * C_), f"dgrad N{N_} {H_}x{W_} C{C_}->K{K_} {R_}x{S_} s{st_}  +  1x1 s{st_} of the same input, one launch")
            continue
        ws = ops._conv_ws(lib, dev, geom, direction == "dgrad")
        if direction == "fwd":
            fn = lambda: lib.conv2d_fwd(x, w, None, y, N_, H_, W_, C_, K_, R_, S_, st_, pd_, ws=ws)
        else:
            wt = torch.empty(w.numel(), device=dev)            # the step gets this transpose from its one weight_prep launch
            lib.weight_transpose(w, wt, K_, R_ * S_, C_)
            fn = lambda: lib.conv2d_bwd_data_pre(y, wt, x, N_, H_, W_, C_, K_, R_, S_, st_, pd_, ws=ws)
        add(lib.conv2d_describe(N_, H_, W_, C_, K_, R_, S_, st_, pd_, direction == "dgrad"), per_step, hip_us(fn), flop, nbytes,
            f"{direction} N{N_} {H_}x{W_} C{C_}->K{K_} {R_}x{S_} s{st_}")
    out = {}
    for name, e in table.items():
        n = max(e["launches_per_step"], 1e-9)
        entry_us = e["us_per_step"]
        # KERNEL time inside the step (roctracer over eager steps) where the profile has this kernel; the back-to-back bracket around the
        # C-ABI entry point (which may launch helper kernels: transposes, slab reductions, statistics) is kept beside it as `entry_*`
        hit = instep_lookup(prof, name)
        us_step, timing = entry_us, "entry point: HIP events over 10 back-to-back launches per shape (helper kernels of the entry included)"
        if hit is not None and hit[0] > 0 and abs(hit[0] - e["launches_per_step"]) <= 0.01:
            us_step, timing = hit[1], "kernel time inside the step: " + prof_how + ", this kernel's launches only"
        elif hit is not None and hit[0] > 0:
            # the tracer returned fewer (or more) launches of this kernel than the step holds -- roctracer drops records now and then, and a
            # per-launch average over the survivors is biased towards whichever shapes survived (seen: 23 of 30, the short ones missing,
            # 99.7 us against rocprofv3's 89.9): keep the entry-point bracket, which times every shape
            timing = (f"entry point: HIP events over 10 back-to-back launches per shape (the in-step trace held {hit[0]:.2f} launches of this kernel "
                      f"per step instead of {e['launches_per_step']:.2f}: not used)")
        ach = e["flop_per_step"] / (us_step * 1e-6) / 1e12
        tr = measured_traffic(name)
        out[name] = {"bound": "mfma", "achieved": ach, "peak": MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": ach / MFMA_PEAK_TF,
                     "traffic": tr, "traffic_ratio": (tr / (e["compulsory_bytes_per_step"] / n)) if tr else None,       # counter bytes / compulsory bytes
                     "kernel": name, "launches_per_step": e["launches_per_step"],
                     "avg_us": us_step / n, "us_per_step": us_step, "timing": timing,
                     "entry_avg_us": entry_us / n, "entry_us_per_step": entry_us,
                     "instep_launches_per_step": hit[0] if hit else None,
                     "executed_flop_per_launch": e["flop_per_step"] / n,
                     # rows of zero padding are executed, not useful: frac_useful = frac x useful_flop_frac
                     "useful_flop_frac": e["useful_flop_per_step"] / max(e["flop_per_step"], 1e-9),
                     "frac_useful": ach / MFMA_PEAK_TF * e["useful_flop_per_step"] / max(e["flop_per_step"], 1e-9),
                     "compulsory_bytes_per_launch": e["compulsory_bytes_per_step"] / n, "shapes": e["shapes"]}
    return out


DUMP_MAX_PARAMS = 1 << 23        # 32 MB of float32: the dump stays far below 64 MB whatever the encoder


def dump_outputs(out_dir, loss, loss_dic, flat):
    """--dump-outputs: what the last timed step handed its caller, as float32 .npy files -- `loss`, `loss_<term>` for every floating
    tensor of the loss dictionary, and `params`: the flat parameter vector after the optimizer step, or DUMP_MAX_PARAMS of its entries
    at fixed seeded positions (ascending) when it is longer."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())
    save("loss", loss)
    for k, v in sorted(loss_dic.items()):
        if k != "loss" and torch.is_tensor(v) and v.is_floating_point():
            save("loss_" + "".join(c if c.isalnum() or c in "_-" else "_" for c in k), v)
    p = flat.flat.detach()
    if p.numel() > DUMP_MAX_PARAMS:
        idx = torch.randperm(p.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_MAX_PARAMS].sort().values
        p = p[idx.to(p.device)]
    save("params", p)


def launch_ranks(a):
    """`python bench.py --gpus N` (N > 1) outside a launcher: start N rank processes of this script, one per GPU, and hand back rank 0's
    JSON line.  The parent never touches the GPU (no HIP call is made before this point: `import torch` alone does not initialise the
    runtime) and nothing is re-exec'd: the ranks are fresh children with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, exactly what
    `python -m torch.distributed.run --nproc-per-node N` would give them (replaces the reference's in-process nn.DataParallel,
    reference train_hrnet.py:560).  Returns the exit code: non-zero when any rank failed."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    base = dict(os.environ, WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"), HIFIHR_BENCH_CHILD="1")
    import tempfile
    procs = []
    with tempfile.TemporaryFile("w+") as out0:
        for r in range(a.gpus):
            env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
            # rank 0's stdout is the JSON line; the other ranks print nothing there, every rank's stderr passes through
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL))
        # a rank that dies leaves the others waiting in a collective: stop them all as soon as one fails
        codes = [None] * a.gpus
        while any(c is None for c in codes):
            for r, p in enumerate(procs):
                if codes[r] is None:
                    codes[r] = p.poll()
            if any(c not in (None, 0) for c in codes):
                time.sleep(2.0)
                for r, p in enumerate(procs):
                    if codes[r] is None:
                        p.kill()                      # exactly the children started above
                        codes[r] = p.wait()
                break
            time.sleep(0.2)
        out0.seek(0)
        sys.stdout.write(out0.read())
        sys.stdout.flush()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print(f"[bench] rank(s) failed (rank, exit code): {bad}", file=sys.stderr, flush=True)
        return 1
    return 0


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a))
    from hifihr_amd import dist as hdist, ops, options, synth
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.mano_tables import synthetic_mano_tables
    from hifihr_amd.models import Model
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep, data_dic, train_step

    rank, local_rank, world = hdist.init_process_group_from_env()
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}: the line would report the wrong n_gpus"
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP hot path has no CPU fallback)"
    dev = torch.device("cuda", local_rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    # Work on a non-default stream from the start: autograd pins each parameter's gradient accumulation to the stream
    # of its first use, and a step that ever ran on the legacy default stream cannot be captured into a hipGraph later.
    torch.cuda.set_stream(torch.cuda.Stream(device=dev))

    image_size, dat_name = 224, "FreiHand"
    nimble = a.hand != "mano"
    assert not nimble or a.config in (3, 5), "--hand nimble-* belongs to configs 3 / 5 (BASELINE configs[2] / [4])"
    hm = "nimble" if nimble else "mano"
    if a.config == 3:
        a.encoder, a.no_cpu_baseline = "effb3", True
        a.batch = 48 if a.batch == 32 else a.batch
        args_ns = options.baseline_config3_args(train_batch=a.batch, hand_model=hm)
    elif a.config == 5:
        a.encoder, a.no_cpu_baseline, image_size, dat_name = "effb3", True, 512, "HO3D"
        a.batch = 16 if a.batch == 32 else a.batch
        args_ns = options.baseline_config5_args(train_batch=a.batch, hand_model=hm)
    else:
        args_ns = options.baseline_config2_args(train_batch=a.batch)
    global _TRAFFIC_OK
    _TRAFFIC_OK = (a.config == 2 and a.encoder == "res18" and a.batch == 32 and a.aa == 3)
    tables = synthetic_mano_tables(0)
    torch.manual_seed(0)
    if nimble:
        from hifihr_amd.nimble_tables import add_synthetic_uv, synthetic_nimble_tables
        ntab = synthetic_nimble_tables(0)
        if a.hand.endswith("-uv"):
            ntab = add_synthetic_uv(ntab)
        model = Model(ifRender=True, device=dev, if_4c=False, hand_model="nimble", use_mean_shape=False, pretrain=a.encoder,
                      mano_tables=tables, nimble_tables=ntab, image_size=image_size, aa_factor=a.aa).to(dev).train()
        model.data_mano = ops.ManoLayerHandle(tables)       # the DATA side stays MANO (FreiHAND / HO-3D ground truth is MANO)
        model.data_renderer = ops.RendererHandle(tables.faces, 778, image_size=224, aa=3)
    else:
        model = Model(ifRender=True, device=dev, if_4c=False, hand_model="mano", use_mean_shape=False, pretrain=a.encoder,
                      texture_stand_in=10 if a.config in (3, 5) else 0, mano_tables=tables, image_size=image_size, aa_factor=a.aa).to(dev).train()
    flat = FlatParams(model)
    hdist.broadcast_params(flat)
    reducer = hdist.GradReducer(flat, num_buckets=4)
    lr = args_ns.force_init_lr if args_ns.force_init_lr > 0 else args_ns.init_lr
    opt = FusedAdam(flat, lr=lr, betas=(0.9, 0.999), grad_scale=reducer.grad_scale)
    loss_func = LossFunction()

    # rank r owns samples [r*B, (r+1)*B) of every global batch
    if dat_name == "FreiHand":
        cache = build_cache(model, a.cache, first_index=rank * a.cache, dev=dev)
        perm_gen = torch.Generator().manual_seed(100 + rank)
        rot_gen = torch.Generator().manual_seed(200 + rank)

        def next_batch(out=None):
            idx = torch.randint(0, cache.n, (a.batch,), generator=perm_gen)
            return cache.batch_examples(idx, generator=rot_gen, out=out, root_id=args_ns.ROOT)
        data_note = ("every step assembles a NEW batch on the device from the uint8 sample cache resident in HBM (one staged H2D copy of "
                     "100 B per sample + hifihr_freihand_batch: gather + affine warp, K / joint / vertex / projection terms of data_dic), "
                     "written straight into the captured step's static inputs")
    else:
        from hifihr_amd.data import HO3DDeviceCache
        # the renderer that draws the synthetic 224 x 224 hands is the bench model's only when that renders at 224
        from hifihr_amd import ops as _ops
        draw = model.renderer_p3d if (image_size == 224 and not nimble) else _ops.RendererHandle(tables.faces, int(tables.v_template.shape[0]), image_size=224, aa=3,
                                                                                 ambient=(0.5,) * 3, mat_diffuse=(0.8,) * 3, specular=(0.04,) * 3,
                                                                                 shininess=30.0, background=(1.0,) * 3)
        ho_cache = HO3DDeviceCache(**synth.make_ho3d_frames(getattr(model, "data_mano", None) or model.hand_layer.handle, draw, a.cache, first_index=rank * a.cache, device=dev), device=dev)
        perm_gen = torch.Generator().manual_seed(100 + rank)
        noise_gen = torch.Generator().manual_seed(300 + rank)

        def next_batch(out=None):
            idx = torch.randint(0, ho_cache.n, (a.batch,), generator=perm_gen)
            return data_dic(ho_cache.batch(idx, generator=noise_gen), "HO3D", "training", args_ns, device=dev, image_size=image_size)
        data_note = ("every step assembles a NEW HO-3D batch on the device from 480 x 640 uint8 frames resident in HBM (hifihr_ho3d_batch: the "
                     "reference's hand crop window per sample, Pillow-exact crop + bilinear / bicubic resize to 224, K_crop / uv21_crop), data_dic, "
                     "copy into the step's static inputs")
    examples = next_batch()
    torch.cuda.synchronize()

    def eager_resident():
        return train_step(model, loss_func, opt, examples, args_ns, dat_name=dat_name, backward_hook=reducer.finish)

    for _ in range(a.warmup):
        eager_resident()
    # --full: a few profiled eager steps: which (shape, direction) every convolution-path kernel ran, the renderer's inputs
    nprof = 3
    if a.full:
        ops.PROFILE.enable()
        for _ in range(nprof):
            eager_resident()
        ops.PROFILE.disable()
        ops.PROFILE.summary()
    lib = ops.get_lib()
    B = a.batch
    extra = {}
    # ---- the step forms
    use_graph = a.graph != 0
    split = world > 1 or a.graph in (2, 3)   # data parallel: graph = forward + backward, then all-reduce + Adam eagerly
    graph_note, gstep = "eager", None
    seg_step = None
    if use_graph:
        try:
            if a.graph == 3:
                from hifihr_amd.traineval import SegmentedGraphedTrainStep
                gstep = SegmentedGraphedTrainStep(model, loss_func, opt, examples, args_ns, reducer, dat_name=dat_name)
                graph_note = "hipGraph replays: forward, then one backward graph per trunk segment with that segment's bucket all-reduced beside the next, fused Adam"
            else:
                gstep = GraphedTrainStep(model, loss_func, opt, examples, args_ns, dat_name=dat_name, reducer=reducer if split else None)
                graph_note = ("hipGraph replay of forward + backward, then bucketed all-reduce + fused Adam" if split
                              else "hipGraph replay (whole step captured)")
        except Exception as e:                          # capture is an optimisation; never fail the bench on it (state is restored)
            graph_note = f"eager (hipGraph capture failed: {type(e).__name__}: {str(e)[:200]})"
            print(f"[bench] rank {rank}: {graph_note}", file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            gstep = None
        if world > 1:
            # every rank must take the same form of the step (the forms issue their bucket all-reduces in different orders).  This is the
            # FIRST collective after the constructors above, whose warm-up and capture are collective-free: a one-sided failure meets
            # the other ranks here
            ok = torch.tensor([1.0 if gstep is not None else 0.0], device=dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if float(ok.item()) == 0.0 and gstep is not None:
                graph_note = "eager (hipGraph capture failed on another rank)"
                gstep.release()
                gstep = None

    def step_streamed():
        if gstep is not None:
            ex = next_batch(out=gstep.static)
            if ex["imgs"].data_ptr() != gstep.static["imgs"].data_ptr():
                gstep.load_batch(ex)
            return gstep()
        ex = next_batch()
        return train_step(model, loss_func, opt, ex, args_ns, dat_name=dat_name, backward_hook=reducer.finish)

    def eager_streamed():
        return train_step(model, loss_func, opt, next_batch(), args_ns, dat_name=dat_name, backward_hook=reducer.finish)

    step = step_streamed
    if world > 1 and gstep is not None and a.graph == -1:
        # Data parallel has two forms of the step: the hipGraph replay followed by the (not overlapped) bucketed all-reduce, and
        # the eager step whose all-reduce buckets overlap the rest of backward.  Which one wins at N > 1 depends on the exchange time
        # and on the host: measure both for a few steps (max over ranks) and keep the faster -- every rank takes the same decision.
        def timed(fn, n=3):
            fn()
            torch.cuda.synchronize(); dist.barrier()
            t_start = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize(); dist.barrier()
            t = torch.tensor([time.perf_counter() - t_start], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item()) / n
        t_graph = timed(step_streamed)
        # third candidate: the segmented form (ResNet trunks), whose exchange overlaps backward under graph replays
        t_seg = None
        gstep.release()
        try:
            from hifihr_amd.traineval import SegmentedGraphedTrainStep
            if os.environ.get("HIFIHR_DP_SEGMENTED", "1") == "0":
                raise NotImplementedError("HIFIHR_DP_SEGMENTED=0")
            seg_step = SegmentedGraphedTrainStep(model, loss_func, opt, examples, args_ns, reducer, dat_name=dat_name)
        except Exception as e:                       # noqa: BLE001 -- other encoders, capture failures: the single-graph form stays
            print(f"[bench] rank {rank}: segmented step not available ({type(e).__name__}: {str(e)[:200]})", file=sys.stderr, flush=True)
            seg_step = None
        ok = torch.tensor([1.0 if seg_step is not None else 0.0], device=dev)      # (collective-free constructor: the ranks meet here)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        if float(ok.item()) == 0.0 and seg_step is not None:
            seg_step.release()
            seg_step = None
        if seg_step is not None:
            whole_step, gstep = gstep, seg_step
            t_seg = timed(step_streamed)
            if t_seg < t_graph:
                graph_note = (f"hipGraph replays, backward in one graph launch per trunk segment with its bucket all-reduced beside the next (chosen over the "
                              f"single-graph form: {t_seg * 1e3:.2f} vs {t_graph * 1e3:.2f} ms/step in a 3-step trial)")
                t_graph = t_seg
            else:
                seg_step.release()
                gstep = whole_step
        reducer.pause_hooks(False)
        t_eager = timed(eager_streamed)
        if t_eager < t_graph:
            step = eager_streamed
            graph_note = (f"eager step, bucketed all-reduce overlapped with backward (chosen over the hipGraph form: "
                          f"{t_eager * 1e3:.2f} vs {t_graph * 1e3:.2f} ms/step in a 3-step trial)")
        else:
            reducer.pause_hooks(True)
            graph_note += f" (chosen over the eager overlapped form: {t_graph * 1e3:.2f} vs {t_eager * 1e3:.2f} ms/step in a 3-step trial)"

    def timed_region(fn, steps):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, out

    resident_ms = None
    if a.full and gstep is not None and step is step_streamed:
        dt_r, _ = timed_region(gstep, a.steps)            # the same captured step replayed on ONE resident batch (round 1's figure)
        resident_ms = dt_r / a.steps * 1e3
    dt, (loss, loss_dic) = timed_region(step, a.steps)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, loss, loss_dic, flat)

    bucket_us = reducer.time_buckets() if (world > 1 and a.full) else None        # a collective: every rank takes part
    # ---- rooflines (--full).  Kernel times come from the form of the step the timed region ran: three REPLAYS of the captured graph under
    # roctracer (single process), where every kernel runs alone on the stream in the graph's order -- the eager profile steps launch weight
    # gradients on a side stream beside other kernels, which inflated them (round-3 review).  Data parallel / eager runs: three eager steps, on every rank.
    rooflines = a.full and not a.no_rooflines
    if world > 1 and rooflines:
        reducer.pause_hooks(False)                   # (the eager profile steps below exchange gradients through the hooks)
    if rank != 0 and rooflines:
        for _ in range(3):                           # the steps rank 0 profiles hold the gradient exchange: every rank runs them
            eager_resident()
    if rank == 0 and rooflines:
        kprof, kprof_how = None, "roctracer (torch.profiler) over 3 eager steps"
        if world == 1 and gstep is not None and step is step_streamed:
            kprof = instep_kernel_times(gstep, nsteps=3)
            if kprof and instep_lookup(kprof, "adam_kernel"):
                kprof_how = "roctracer (torch.profiler) over 3 replays of the captured step (the graph the timed region replays)"
            else:
                kprof = None
        if kprof is None:
            kprof = instep_kernel_times(eager_resident, nsteps=3)
        roofs = conv_path_rooflines(ops, lib, dev, nprof, kprof, kprof_how)
        # ---- the north star's HBM-bound kernels: rasteriser (forward / backward) and MANO LBS, 20 back-to-back launches each
        if ops.PROFILE.last_render is not None:
            h_r, v_r, c_r, cam_r, lc_r, ld_r = ops.PROFILE.last_render
            Br, Hr, Sr, Vn, Fn = v_r.shape[0], h_r.H, h_r.H * h_r.aa, v_r.shape[1], int(h_r.F)
            rgba_r = torch.empty(Br, 4, Hr, Hr, device=dev); fid_r = torch.empty(Br, Sr, Sr, dtype=torch.int32, device=dev)
            ws_r = h_r.workspace(Br, dev)
            us_f = hip_us(lambda: h_r.lib.render_fwd(h_r.h, v_r, c_r, cam_r, lc_r, ld_r, rgba_r, fid_r, ws_r), n=20)
            g_r = torch.randn(Br, 4, Hr, Hr, device=dev); gv = torch.empty_like(v_r); gc = torch.empty_like(v_r)
            glc = torch.empty(Br, 3, device=dev); gld = torch.empty(Br, 3, device=dev)
            us_b = hip_us(lambda: h_r.lib.render_bwd(h_r.h, v_r, cam_r, lc_r, ld_r, fid_r, g_r, gv, gc, glc, gld, ws_r), n=20)
            # algorithmic bytes per image (SURVEY.md 8d / DESIGN.md section 4): fwd = verts V*12 + faces F*12 + per-vertex attributes V*24
            # + RGBA out H^2*16 + face-id side buffer S^2*4;  bwd = side buffer + grad RGBA in + grad verts / colours out
            alg_f = Vn * 12 + Fn * 12 + Vn * 24 + Hr * Hr * 16 + Sr * Sr * 4
            alg_b = Sr * Sr * 4 + Hr * Hr * 16 + Vn * 24
            for key, us, alg, kname, kk in (("roofline_render_fwd", us_f, alg_f, f"render_fwd3_kernel<{h_r.aa}> (+ render_vertex_kernel, render_bin_kernel)",
                                             "render_fwd3_kernel" if instep_lookup(kprof, "render_fwd3_kernel") else "render_fwd2_kernel"),
                                            ("roofline_render_bwd", us_b, alg_b, f"render_bwd_kernel<{h_r.aa}> (+ render_vertex_bwd_kernel)", "render_bwd_kernel")):
                ach = alg * Br / (us * 1e-6) / 1e9
                hit = instep_lookup(kprof, kk)
                tr_r = measured_traffic(key.replace("roofline_", ""))
                extra[key] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                              "traffic": tr_r, "traffic_ratio": (tr_r / (alg * Br)) if tr_r else None, "kernel": kname, "avg_us": us,
                              "algorithmic_bytes_per_launch": alg * Br,
                              "timing": "HIP events over 20 back-to-back launches of the C-ABI entry on this batch's meshes (the launch's helper kernels and "
                                        "memsets included)"}
                if hit is not None and hit[0] > 0:
                    k_us = hit[1] / hit[0]
                    extra[key]["tile_kernel_in_step"] = {"avg_us": k_us, "achieved": alg * Br / (k_us * 1e-6) / 1e9,
                                                         "frac": alg * Br / (k_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                                         "timing": "the tile kernel alone inside the step: " + kprof_how}
            extra["render_ms_per_frame"] = {"fwd": us_f / Br / 1e3, "fwd+bwd": (us_f + us_b) / Br / 1e3, "image_size": Hr, "aa": h_r.aa}
        mh = getattr(model, "data_mano", None) or model.hand_layer.handle
        pose = torch.randn(B, 48, device=dev) * 0.5; beta = torch.randn(B, 10, device=dev) * 0.5
        verts = torch.empty(B, 778, 3, device=dev); jtr = torch.empty(B, 21, 3, device=dev); saved = torch.empty(B, 778, 3, device=dev)
        us_mf = hip_us(lambda: lib.mano_lbs_fwd(mh.h, pose, beta, verts, jtr, saved), n=20)
        gvv = torch.randn(B, 778, 3, device=dev); gj = torch.randn(B, 21, 3, device=dev)
        gp = torch.empty(B, 48, device=dev); gb = torch.empty(B, 10, device=dev)
        us_mb = hip_us(lambda: lib.mano_lbs_bwd(mh.h, pose, beta, saved, gvv, gj, gp, gb), n=20)
        tbl = 4 * (3 * 800 + 10 * 3 * 800 + 135 * 3 * 800 + 16 * 800 * 2 + 45 * 45 + 45)        # the padded SoA tables one launch reads
        alg_mf = tbl + B * (232 + 778 * 12 + 21 * 12)
        alg_mb = tbl + B * (232 + 778 * 12 * 2 + 21 * 12 + 232)
        extra["roofline_mano_lbs"] = {
            "bound": "hbm", "achieved": alg_mf / (us_mf * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": alg_mf / (us_mf * 1e-6) / 1e9 / HBM_PEAK_GBS, "traffic": measured_traffic("mano_fwd_kernel"), "kernel": "mano_fwd_kernel",
            "avg_us": us_mf, "algorithmic_bytes_per_launch": alg_mf,
            "backward": {"kernel": "mano_bwd_kernel", "avg_us": us_mb, "algorithmic_bytes_per_launch": alg_mb,
                         "achieved": alg_mb / (us_mb * 1e-6) / 1e9, "frac": alg_mb / (us_mb * 1e-6) / 1e9 / HBM_PEAK_GBS},
            "in_step": (lambda hf, hb: {"fwd_avg_us": hf[1] / hf[0] if hf and hf[0] else None, "bwd_avg_us": hb[1] / hb[0] if hb and hb[0] else None,
                                        "fwd_frac": (alg_mf / (hf[1] / hf[0] * 1e-6) / 1e9 / HBM_PEAK_GBS) if hf and hf[0] else None,
                                        "timing": "kernel time inside the step (" + kprof_how + "): tables cold in L2, unlike the "
                                                  "back-to-back figure above"})(instep_lookup(kprof, "mano_fwd_kernel"), instep_lookup(kprof, "mano_bwd_kernel")),
            "note": f"B = {B} hands: 1.43 MB of tables + 9.8 KB per hand; a launch this small is latency-bound (one dependent chain per hand: "
                    "PCA -> 16 Rodrigues -> kinematic chain -> blend), the HBM fraction says how little memory it touches, not how slow it moves bytes"}
        if roofs:
            dom = max(roofs.values(), key=lambda e: e["us_per_step"])
            extra["roofline"] = dict({k: v for k, v in dom.items() if k != "shapes"},
                                     flops="the products the kernel executes (2 M N K per Winograd GEMM), per shape x launches per step")
            extra["roofline_kernels"] = {k: {kk: v[kk] for kk in ("achieved", "frac", "launches_per_step", "avg_us", "us_per_step", "timing", "entry_avg_us",
                                                                   "entry_us_per_step", "traffic", "traffic_ratio", "compulsory_bytes_per_launch", "useful_flop_frac", "frac_useful", "shapes")}
                                         for k, v in roofs.items()}
            tot_f = sum(v["executed_flop_per_launch"] * v["launches_per_step"] for v in roofs.values())
            tot_us = sum(v["us_per_step"] for v in roofs.values())
            tot_u = sum(v["executed_flop_per_launch"] * v["useful_flop_frac"] * v["launches_per_step"] for v in roofs.values())
            extra["conv_path"] = {"executed_flop_per_step": tot_f, "useful_flop_per_step": tot_u, "frac_useful": tot_u / (tot_us * 1e-6) / 1e12 / MFMA_PEAK_TF,
                                  "mfma_kernel_us_per_step": tot_us,
                                  "achieved": tot_f / (tot_us * 1e-6) / 1e12, "frac": tot_f / (tot_us * 1e-6) / 1e12 / MFMA_PEAK_TF,
                                  "note": "all MFMA kernels of the convolution path together (direct, Winograd GEMMs, weight gradients)"}

    if rank == 0:
        ms = dt / a.steps * 1e3
        wl = {2: "BASELINE configs[1]: FreiHAND batch=32/GPU, ResNet-18 encoder + MANO LBS + silhouette/texture render losses, 224x224, aa=3 (672^2 samples)",
              3: "BASELINE configs[2] composition: full_rhd_freihand.json (EfficientNet-b3, batch 48, losses incl. VGG19 perceptual with seeded random "
                 "weights), MANO + vertex-colour texture stand-in for the unavailable NIMBLE layer [NOT the headline config]",
              5: f"BASELINE configs[4] composition: HO-3D weak supervision (weak_rhd_ho3d.json losses), {image_size}^2 render at aa={a.aa}, batch 16/GPU, "
                 "EfficientNet-b3 on a 224^2 resize of the crop, MANO + texture stand-in for NIMBLE [NOT the headline config]"}[a.config]
        if nimble:
            wl = wl.replace("MANO + vertex-colour texture stand-in for the unavailable NIMBLE layer", "the NIMBLE-SHAPED layer on seeded synthetic tables").replace(
                "MANO + texture stand-in for NIMBLE", "the NIMBLE-SHAPED layer on seeded synthetic tables")
            wl += (f" [hand layer: {a.hand}: 5 990 skin vertices / 11 976 faces rendered, 25 joints, 20 / 30 / 10 PCA"
                   + (", TexturesUV sampling of a 64 x 64 texture image" if a.hand.endswith("-uv") else ", per-vertex texture") +
                   "; synthetic tables -- the real NIMBLE assets are absent, parity unpinned]")
        if a.config == 2 and a.encoder != "res18":
            wl += f" [encoder swapped to {a.encoder}: NOT the headline config]"
        out = {
            "metric": "train images/sec, FreiHAND 224x224 (ResNet-18 + MANO LBS + render + losses + Adam)",
            "value": world * B * a.steps / dt, "unit": "images/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic (FreiHAND-shaped, seeded; synthetic MANO-shaped tables; random-init weights)",
            "config": {"workload": wl, "per_gpu_batch": B, "global_batch": world * B, "losses": args_ns.losses, "parallelism": f"dp{world}"},
            "loss": float(loss.detach()), "launch_mode": graph_note, "input_delivery": data_note,
        }
        if resident_ms is not None:
            out["resident_batch"] = {"ms_per_step": resident_ms, "images_per_sec": world * B / (resident_ms * 1e-3),
                                     "note": "the same captured step replayed on one resident batch (no batch assembly, no copies): round 1's timed region"}
        if world > 1:
            out["rccl"] = {"world_size": dist.get_world_size(), "launched_by": "bench.py itself (one child process per GPU)" if os.environ.get("HIFIHR_BENCH_CHILD") else "external launcher (torch.distributed.run)", "backend": dist.get_backend(), "buckets": len(reducer.buckets),
                           "bucket_bytes": [int(4 * (e_hi - e_lo)) for (_, _, e_lo, e_hi) in reducer.buckets],
                           "allreduce_us_per_bucket": bucket_us}
        out.update(extra)
        if world == 1 and a.full and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args_ns, examples, tables, a.cpu_batch, steps=tuple(int(x) for x in a.cpu_steps.split(",")))
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
