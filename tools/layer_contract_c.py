#!/usr/bin/env python3
"""Where the constants of tests/kernel_cases.py LAYER_CONTRACT_C / LAYER_CONTRACT_FLOOR come from: the layer contract's float64 references run
in float32 -- plain fp32 PyTorch on the CPU -- over the emulator geometry lists of tests/test_hostsim_layer_contract.py (and, for the kinds of the GEMM and tail
contracts, of tests/test_hostsim_gemm_contract.py / tests/test_hostsim_tail_contract.py), compared with the same
references in float64.  Per kind it prints the worst  err / (sqrt(L) max|ref| + cond)  (c is 4 times that) and, over the comparisons whose
reference is zero to rounding, the worst absolute error (the floor is 4 times that).  No kernel runs.

    python tools/layer_contract_c.py
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import kernel_cases as kc                      # noqa: E402
import test_hostsim_layer_contract as lists    # noqa: E402
gemm_lists = kc                               # (the GEMM contract's lists live next to its case bodies)

RATIO, FLOOR = {}, {}
F32, F64 = torch.float32, torch.float64


def note(kind, got, ref, L, cond=0.0, where=""):
    err = kc.layer_err(got, ref)
    scale = max(L, 1) ** 0.5 * (float(ref.abs().max()) if ref.numel() else 0.0) + cond
    if scale < 1e-9:                            # a reference that is zero to rounding: its error is a floor, not a ratio
        if err > FLOOR.get(kind, (0.0, ""))[0]:
            FLOOR[kind] = (err, where)
    elif err / scale > RATIO.get(kind, (0.0, ""))[0]:
        RATIO[kind] = (err / scale, where)


def both(ref64, ref32, names, where):
    for n in names:
        q = ref64[n]
        note(q[0], ref32[n][2], q[2], q[1], q[3] if len(q) > 3 else 0.0, f"{where} {n}")


def tail():
    """The kinds of the tail contract (tests/test_hostsim_tail_contract.py): every float64 reference of kernel_cases' "The tail contract" run
    in float32 on the same lists; and the Procrustes floor, the largest difference between two float64 routes to the same err_sum."""
    import numpy as np
    import test_hostsim_tail_contract as tl
    q = lambda kind, a, b, L, cond=0.0, where="": note(kind, a, b, L, cond, where)
    for n, wd, gs in tl.ADAM_CASES:
        inp = kc.adam_contract_inputs(n, n)
        zero = torch.zeros(n)
        for step, m, v in ((1, zero, zero), (2, inp["m"], inp["v"]), (3, inp["m"], inp["v"]), (1000, inp["m"], inp["v"])):
            r64, r32 = (kc.adam_contract_ref(inp["p"], inp["g"][0], m, v, step, wd, gs, dt=dt) for dt in (F64, F32))
            for kind, a, b in zip(("adam_p", "adam_m", "adam_v"), r32, r64):
                q(kind, a, b, 1, where=f"adam {(n, wd, gs)} step {step}")
    for g in tl.TEXPCA_GEOMS:
        if kc.texpca_contract_expect(*g[:3]):
            inp = kc.texpca_contract_inputs(*g[:3], sum(g[:3]))
            both(kc.texpca_contract_ref(inp, g[3]), kc.texpca_contract_ref(inp, g[3], dt=F32), ("tex", "dcoef"), f"texpca {g}")
    for g in tl.GEOM_CASES:
        if kc.geom_contract_expect(*g[:6]):
            inp = kc.geom_contract_inputs(*g[:6], g[7], sum(g[:6]))
            (o64, g64), (o32, g32) = kc.geom_contract_ref(inp, g[6]), kc.geom_contract_ref(inp, g[6], dt=F32)
            for k in range(5):
                q("geom_out", o32[k][2], o64[k][2], o64[k][1], where=f"geom {g} out[{k}]")
            for n_ in g64:
                q("geom_grad", g32[n_][2], g64[n_][2], g64[n_][1], where=f"geom {g} {n_}")
    for g in tl.JOINT_CASES:
        if kc.joint_contract_expect(g[0], g[5], g[2], g[3]):
            inp = kc.joint_contract_inputs(g[0], g[4], g[0])
            (o64, g64), (o32, g32) = kc.joint_contract_ref(inp, g[1], g[2], g[3]), kc.joint_contract_ref(inp, g[1], g[2], g[3], dt=F32)
            for k, L in enumerate((g[0] * 42, g[0] * 40, g[0] * 60)):
                q("joint_out", o32[k], o64[k], L, where=f"joint {g} out[{k}]")
            for n_ in g64:
                for b in range(g[0]):                                       # (per sample, as the case compares)
                    q("joint_grad", g32[n_][b], g64[n_][b], 6, where=f"joint {g} {n_} sample {b}")
    for g in tl.PHOTO_CASES:
        if kc.photo_contract_expect(*g[:3]) and g[3] != "nan":
            inp = kc.photo_contract_inputs(*g[:3], g[3], sum(g[:3]))
            r64, r32 = kc.photo_contract_ref(inp), kc.photo_contract_ref(inp, dt=F32)
            both(r64, r32, ("re_m", "tex", "mrgb", "sil", "dm"), f"photo {g}")
            out32 = torch.cat([r32[k][2] for k in ("tex", "mrgb", "sil", "dm")])          # the backward starts from the fp32 forward's tensors
            b64 = kc.photo_contract_bwd_ref(inp, r32["re_m"][2], r32["mk"], out32, True, True)
            b32 = kc.photo_contract_bwd_ref(inp, r32["re_m"][2], r32["mk"], out32, True, True, dt=F32)
            q("photo_grad", b32[2], b64[2], 1, where=f"photo {g} grad")
    for counts, lengths, mode in tl.TOTAL_CASES:
        if mode == "ok" and 1 <= len(counts) <= 4 and all(0 <= c <= 64 for c in counts) and sum(counts):
            gen = torch.Generator().manual_seed(len(counts))
            parts = [torch.randn(max(c, 1), generator=gen)[:c] for c in counts]
            s32 = torch.zeros(())
            for p in parts:
                for x in p:
                    s32 = s32 + x
            q("total", s32.reshape(1), sum(p.double().sum() for p in parts).reshape(1), sum(counts), sum(float(p.abs().sum()) for p in parts), f"total {counts}")
    for name, B, family, root_id in tl.MANO_CASES:
        if B > 0 and root_id < 21:
            t, inp = tl.tail_tables(name), kc.mano_contract_inputs(B, family, 5 + B)
            (v64, j64, g64), (v32, j32, g32) = kc.mano_layer_ref(t, inp), kc.mano_layer_ref(t, inp, dt=F32)
            w = f"mano {(name, B, family, root_id)}"
            q("mano_v", v32, v64, 16, where=w + " verts")
            q("mano_v", j32, j64, 16, where=w + " jtr")
            for i in (0, 1):
                q("mano_g", g32["v"][i] + g32["j"][i], g64["v"][i] + g64["j"][i], 778, where=w + " layer grad")
            a64, a32 = kc.mano_joints_ref(t, v32, inp, root_id), kc.mano_joints_ref(t, v32, inp, root_id, dt=F32)
            for i in range(3):
                q("mano_j", a32[i], a64[i], 778, where=w + " joints")
            q("mano_gv", sum(a32[3].values()), sum(a64[3].values()), 22, where=w + " gverts")
            (f64_, fg64), (f32_, fg32) = kc.mano_full_ref(t, inp, root_id), kc.mano_full_ref(t, inp, root_id, dt=F32)
            q("mano_v", f32_["vc"], f64_["vc"], 16, where=w + " verts_cam")
            for i in (0, 1):
                q("mano_g", sum(fg32[k][i] for k in fg32), sum(fg64[k][i] for k in fg64), 778, where=w + " fused grad")
    for V, J, S, B in tl.LBS_CASES:
        if B > 0:
            tabs = kc.random_lbs_tables(V, J, S, V + J + S + B)
            inp = kc.lbs_contract_inputs(tabs, B, V + J + S + B)
            r64, r32 = kc.lbs_contract_ref(tabs, inp), kc.lbs_contract_ref(tabs, inp, dt=F32)
            w = f"lbs {(V, J, S, B)}"
            q("lbs_v", r32[0], r64[0], J, where=w + " verts")
            q("lbs_v", r32[1], r64[1], J, where=w + " joints")
            for i in (0, 1):
                if r64[2]["v"][i].numel():
                    q("lbs_g", r32[2]["v"][i] + r32[2]["j"][i], r64[2]["v"][i] + r64[2]["j"][i], V, where=w + " grad")
            q("lbs_g", r32[3], r64[3], V, where=w + " scratch")
    worst, rel, at = 0.0, 0.0, ""
    for B, N, family in tl.PROCRUSTES_CASES:
        if kc.procrustes_contract_expect(B, N):
            pred, gt = kc.procrustes_contract_inputs(family, B, N, N + len(family))
            a, b = kc.procrustes_contract_ref(pred, gt)["err_sum"], kc.procrustes_contract_ref(pred, gt, route="eigen")["err_sum"]
            d = float(np.abs(a - b).max())
            if d > worst:
                worst, at = d, f"{(B, N, family)} (err_sum {float(a.max()):.3e})"
            rel = max(rel, float((np.abs(a - b) / (N * np.abs(gt.double().numpy()).max((1, 2)))).max()))
    print(f"Procrustes: two float64 routes to err_sum differ by at most {worst:.3e} at {at}; x 4 = {4 * worst:.2e} (table floor {kc.PROCRUSTES_FLOOR:.2e});"
          f" relative to N max|gt|: {rel:.3e}, x 4 = {4 * rel:.2e} (table {kc.PROCRUSTES_FLOOR_REL:.2e})")


def main():
    torch.manual_seed(0)
    for g in lists.BN_GEOMS:
        M, C, act, residual = g[:4]
        if not kc.bn_contract_expect(M, C)["bn_stats"] or (act == 2 and residual):
            continue
        inp = kc.bn_contract_inputs(M, C, residual, sum(map(int, g)))
        r64, mid = kc.bn_contract_ref(inp, act, 1e-5, 0.1)
        mask = (mid["z"] > 0) if act == 1 else None                       # the fp32 run keeps the float64 run's ReLU decisions
        r32, _ = kc.bn_contract_ref(inp, act, 1e-5, 0.1, dt=F32, mask=mask)
        both(r64, r32, ("sum", "sumsq", "mean", "invstd", "rm", "rv", "y", "y_eval", "dx", "dgamma", "dbeta"), f"bn {g}")
    import torch.nn.functional as Fn
    for g in lists.POOL_GEOMS:
        N, H, W, C, k, s, p, mode = g
        if not kc.pool_contract_expect(*g[:7])["maxpool2d_bwd"] or mode == "special":
            continue
        gen = torch.Generator().manual_seed(sum(g[:7]))
        x = torch.randn(N, H, W, C, generator=gen)
        x = torch.relu(x) if mode == "ties" else x
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        gy = torch.randn(N, OH, OW, C, generator=gen)
        grads = []
        for dt in (F64, F32):
            xr = x.to(dt).permute(0, 3, 1, 2).clone().requires_grad_(True)
            Fn.max_pool2d(xr, k, s, p).backward(gy.to(dt).permute(0, 3, 1, 2))
            grads.append(xr.grad)
        note("pool_dx", grads[1], grads[0], ((k + s - 1) // s) ** 2, where=f"pool {g}")
    for g in lists.MMPOOL_GEOMS:
        if kc.mmpool_contract_expect(*g[:3]):
            x, gy = kc.mmpool_contract_inputs(g[0], g[1], g[2], g[4], g[0] + g[1] + g[2])
            both(kc.mmpool_contract_ref(x, g[3], gy), kc.mmpool_contract_ref(x, g[3], gy, dt=F32), ("y", "xavg", "dx", "dp"), f"mmpool {g}")
    for g in lists.DW_GEOMS:
        if kc.dw_contract_expect(*g):
            inp = kc.dw_contract_inputs(g[0], g[1], g[2], g[3], g[4], g[8], g[9], sum(g))
            for pre in (False, True):
                both(kc.dw_contract_ref(inp, g, pre), kc.dw_contract_ref(inp, g, pre, dt=F32), ("y", "sum", "sumsq", "dw") + (() if pre else ("dx",)),
                     f"dw {g} pre={pre}")
    for g in lists.SE_GEOMS:
        B, HW, C, SQ = g
        exp = kc.se_contract_expect(*g)
        inp = kc.se_contract_inputs(B, HW, C, max(SQ, 1), sum(g))
        if exp["se_pool"]:
            both(kc.se_plain_ref(inp), kc.se_plain_ref(inp, dt=F32), ("pool", "bwd_gate", "scale", "scale_add"), f"se {g}")
        if exp["se_mlp_fwd"]:
            f64, f32 = kc.se_mlp_fwd_ref(inp), kc.se_mlp_fwd_ref(inp, dt=F32)
            both(f64, f32, ("z1", "h1", "gate"), f"se {g}")
            saved = [f32[k][2] for k in ("gate", "z1", "h1", "mean")]         # the backward starts from the fp32 forward's tensors, as the entry does
            both(kc.se_mlp_bwd_ref(inp, *saved), kc.se_mlp_bwd_ref(inp, *saved, dt=F32), ("dz2", "dz1", "dmean", "dw1", "db1", "dw2", "db2"), f"se {g}")
    for g in lists.DROP_GEOMS:
        B, n, keep, with_skip = g
        if n % 4 == 0 and keep > 0:
            gen = torch.Generator().manual_seed(B + n)
            x, u = torch.randn(B, n, generator=gen), torch.rand(B, generator=gen)
            m = torch.floor(torch.tensor(keep) + u)
            k32 = float(torch.tensor(keep, dtype=F32))
            note("se_y", x / keep * m.unsqueeze(1), x.double() / k32 * m.double().unsqueeze(1), 1, where=f"drop {g}")
    for g in lists.SSIM_GEOMS:
        a, b = kc.ssim_contract_inputs(g[0], g[1], g[2], g[3], sum(g[:3]))
        both(kc.ssim_contract_ref(a, b, 2.0), kc.ssim_contract_ref(a, b, 2.0, dt=F32), ("value", "partial", "dA", "dB", "dC", "grad"), f"ssim {g}")
    for count in lists.SSIM_FINISH_COUNTS:
        p = torch.rand(count, generator=torch.Generator().manual_seed(count)) * 1024
        note("ssim_val", p.sum().reshape(1), p.double().sum().reshape(1), count, where=f"ssim_finish {count}")
    # the GEMM contract (tests/test_hostsim_gemm_contract.py): torch.matmul in fp32 against float64, every slab of the TN products
    for g in gemm_lists.NT_SHAPES:
        M, N, K, batch = g[:4]
        if kc.bgemm_nt_expect(M, N, K, batch):
            a, b = kc.gemm_operands("randn", batch, M, N, K, sum(g[:4]) % 1000, False)
            note("gemm_nt", torch.matmul(a, b.transpose(1, 2)), torch.matmul(a.double(), b.double().transpose(1, 2)), K, where=f"nt {g[:4]}")
    for g in gemm_lists.TN_SHAPES:
        M, N, T, batch = g[:4]
        if kc.bgemm_tn_expect(M, N, T, batch):
            a, b = kc.gemm_operands("randn", batch, M, N, T, sum(g[:4]) % 1000, True)
            for lo, hi in {(0, T)} | {kc.bgemm_tn_slab_rows(T, 3, z) for z in range(3) if T >= 96}:
                note("gemm_tn", torch.matmul(a[:, lo:hi].transpose(1, 2), b[:, lo:hi]),
                     torch.matmul(a[:, lo:hi].double().transpose(1, 2), b[:, lo:hi].double()), hi - lo, where=f"tn {g[:4]} rows {lo}..{hi}")
    for g in gemm_lists.LINEAR_SHAPES:
        B, I, O, act, bn = g[:5]
        if kc.linear_contract_expect(B, I, O, act, bn):
            inp = kc.linear_contract_inputs(B, I, O, sum(map(int, g)))
            r64 = kc.linear_contract_ref(inp, act, bn)
            mask = (r64["y"][2] > 0) if act == 1 else None                    # the fp32 run keeps the float64 run's ReLU decisions
            r32 = kc.linear_contract_ref(inp, act, bn, dt=F32, mask=mask)
            both(r64, r32, [n for n in r64], f"linear {g}")
    # Winograd: F(2x2) and every weight gradient against fp32 conv2d and its autograd; F(4x4) y / dx / dw are another algorithm than fp32 direct
    # convolution: the test's own chain (kernel transforms on the emulator around a matmul) with the float64 product replaced by an fp32 one
    lib = kc.build_hostsim()
    table = dict(kc.LAYER_CONTRACT_C)
    for g in gemm_lists.WINO_GEOMS:
        if not kc.wino_contract_expect(*g):
            continue
        inp = kc.wino_contract_inputs(*g[:5], sum(g))
        if g[5] == 2:
            r64, r32 = kc.wino_contract_ref(inp), kc.wino_contract_ref(inp, dt=F32)
            for n, kind in (("y", "wino_fwd"), ("dx", "wino_fwd"), ("dw", "wino_wgrad")):
                note(kind, r32[n][1], r64[n][1], r64[n][0], where=f"wino {g} {n}")
        else:
            for kind in ("wino4_fwd", "wino4_wgrad", "bn_sum"):
                kc.LAYER_CONTRACT_C[kind] = (1.0, float("inf"))               # bound = sqrt(L) max|ref| + cond: the logged err / bound is the ratio
            before = {e: v[2] for e, v in kc.LAYER_CONTRACT_LOG.items()}
            for e in ("_wino_output_transform", "_wino_output_transform_act", "_wino_dw_transform_parts"):
                kc.LAYER_CONTRACT_LOG.pop(e, None)
            kc.wino_chain_contract_case(lib, "cpu", *g, seed=sum(g), product=F32, log=False)
            kc.LAYER_CONTRACT_C.update(table)
            for e, kind in (("_wino_output_transform", "wino4_fwd"), ("_wino_dw_transform_parts", "wino4_wgrad")):
                r = kc.LAYER_CONTRACT_LOG[e][2]
                if r > RATIO.get(kind, (0.0, ""))[0]:
                    RATIO[kind] = (r, f"wino {g} (fp32 product, emulator)")
    tail()
    print(f"{'kind':14s} {'fp32 torch ratio':>17s} {'x 4':>10s} {'table c':>10s} {'cap':>8s}   worst at")
    for kind, (c, cap) in kc.LAYER_CONTRACT_C.items():
        r, where = RATIO.get(kind, (0.0, "-"))
        print(f"{kind:14s} {r:17.3e} {4 * r:10.2e} {c:10.2e} {cap:8.0e}   {where}")
    print("floors (references that are zero to rounding): kind, fp32 torch's absolute error, x 4, table floor")
    for kind, (e, where) in sorted(FLOOR.items()):
        print(f"{kind:14s} {e:17.3e} {4 * e:10.2e} {kc.LAYER_CONTRACT_FLOOR.get(kind, 0.0):10.2e}   {where}")


if __name__ == "__main__":
    main()
