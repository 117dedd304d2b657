"""Shared bodies of the tests of the HO-3D device-path extras: hifihr_ho3d_keypoints and hifihr_ho3d_depth_crop (csrc/augment.hip) and
hifihr_depth_points (csrc/depth_points.hip).  tests/test_hostsim_ho3d_extras.py runs them on the emulator (device='cpu'),
tests/test_gpu_ho3d_extras.py on the MI355X (device='cuda').

References: numpy restatements in the number formats include/hifihr.h states (float32 operation by operation for the detections, Pillow's
own crop + NEAREST resize for the depth, np.flatnonzero and the float32 product for the draws, float64 for the back-projection).
Bounds: everything bit for bit / integer for integer, except
  * the back-projected points: one float32 unit in the last place of the sample's largest component (a device double division may differ
    from numpy's in its last bit; the cases print how much of it was used);
  * the closed loop (render -> depth map -> points -> distance to the mesh): twice the residual of the float64 back-projection of the SAME
    float32 depth map plus (8 x 2^-24 x the scene's depth)^2 -- a point rounded to float32 moves by at most sqrt(3) 2^-24 z, and
    (d + e)^2 <= 2 d^2 + 2 e^2 with 2 x 3 <= 8^2.  The same restatement with the pixel centre off by half a pixel must miss that bound by
    orders of magnitude, so the test cannot pass vacuously."""
import numpy as np
import torch

import depth_cases as dc
import kernel_cases as kc
import mesh_reg_cases as mr
import point_mesh_ref as pr

EINVAL = -1
F32 = np.float32
KERNELS = {"ho3d_keypoints_kernel", "ho3d_depth_crop_kernel", "depth_points_kernel"}
MAX_WINDOW = 800                 # HIFIHR_HO3D_MAX_WINDOW
PIXEL_CENTRE = 0.5               # include/hifihr.h "Depth map to points": c


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def pack(idx, box, center, scale):
    """packed_d of hifihr_ho3d_batch: idx[B], box[B][4], window[B][3] (float bits)."""
    win = np.concatenate([np.asarray(center, F32), np.asarray(scale, F32)[:, None]], 1).astype(F32)
    return np.concatenate([np.asarray(idx, np.int32), np.asarray(box, np.int32).reshape(-1), win.reshape(-1).view(np.int32)])


# ---- 1. detections through the crop window ----------------------------------------------------------------------------------------
DET_FRAME = (3, 48, 64, 16)      # n frames of FH x FW, out_size S
DET_CASES = [(1, False), (3, False), (3, True)]       # (B, confidences as [n,21,1])


def det_inputs(B):
    n, FH, FW, S = DET_FRAME
    rng = np.random.default_rng(100 + B)
    uv21 = (rng.random((n, 21, 2)) * [FW, FH]).astype(F32)
    det = (uv21 + 3 * rng.standard_normal((n, 21, 2))).astype(F32)
    con = rng.random((n, 21)).astype(F32)
    con[rng.random((n, 21)) < 0.1] = 0.0
    idx = np.asarray([2] if B == 1 else [1, 0, 1][:B], np.int32)            # a repeated index
    center = (rng.random((B, 2)) * [FW, FH]).astype(F32)
    scale = (0.3 + 2.0 * rng.random(B)).astype(F32)
    box = np.stack([np.asarray([4, 5, 30, 31], np.int32)] * B)
    return uv21, det, con, idx, box, center, scale


def crop_window_ref(pts, idx, center, scale, S):
    """(pts[idx] - centre) * scale + S // 2: three float32 operations, each rounded."""
    p = np.asarray(pts, F32)[idx]
    return ((p - center[:, None, :]).astype(F32) * scale[:, None, None]).astype(F32) + F32(S // 2)


def detections_case(lib, device, B, con3):
    n, FH, FW, S = DET_FRAME
    uv21, det, con, idx, box, center, scale = det_inputs(B)
    G = kc.Guards(device)
    packed = G.inp(_dev(pack(idx, box, center, scale), device))
    con_in = con.reshape(n, 21, 1) if con3 else con
    odet, ocon = G.out(B, 21, 2, fill=float("nan")), G.out(*((B, 21, 1) if con3 else (B, 21)), fill=float("nan"))
    lib.ho3d_keypoints(G.inp(_dev(det, device)), G.inp(_dev(con_in, device)), packed, B, S, odet, ocon)
    want = crop_window_ref(det, idx, center, scale, S)
    assert np.array_equal(odet.cpu().numpy().view(np.int32), want.view(np.int32)), "open_2dj_crop differs from the float32 restatement"
    assert np.array_equal(ocon.cpu().numpy().view(np.int32), con_in[idx].view(np.int32)), "the confidences did not pass through bit for bit"
    # detections equal to uv21 give the bits of hifihr_ho3d_batch's uv21_crop
    ouv = G.out(B, 21, 2, fill=float("nan"))
    ws = torch.empty(lib.ho3d_workspace_bytes(B, S) // 4 + 1, dtype=torch.int32, device=device)
    lib._run("hifihr_ho3d_batch", None, None, None, G.inp(_dev(uv21, device)), None, FH, FW, packed, B, S, ws, ws.numel() * 4, None, None, None,
             ouv, None)
    odet2 = G.out(B, 21, 2, fill=float("nan"))
    lib.ho3d_keypoints(G.inp(_dev(uv21, device)), G.inp(_dev(con, device)), packed, B, S, odet2, None)
    assert torch.equal(odet2.view(torch.int32), ouv.view(torch.int32)), "uv21 as detections does not reproduce uv21_crop's bits"
    assert np.array_equal(ouv.cpu().numpy().view(np.int32), crop_window_ref(uv21, idx, center, scale, S).view(np.int32))
    G.intact("ho3d_keypoints")


def keypoints_refusal_case(lib, device):
    G = kc.Guards(device)
    B, n, S = 2, 4, 16
    det, con = G.inp(torch.rand(n, 21, 2)), G.inp(torch.rand(n, 21))
    center, scale = np.asarray([[3.0, 4.0], [5.0, 6.0]], F32), np.asarray([1.5, 0.5], F32)
    packed = G.inp(_dev(pack([1, 3], [[0, 0, 8, 8]] * 2, center, scale), device))
    odet, ocon = G.out(B, 21, 2), G.out(B, 21)
    call = lambda det=det, con=con, n=n, packed=packed, B=B, S=S, odet=odet, ocon=ocon: lib._call(
        "hifihr_ho3d_keypoints", det, con, n, packed, B, S, odet, ocon)
    for what, kw in [("n = 0", dict(n=0)), ("n < 0", dict(n=-1)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-2)), ("out_size 0", dict(S=0)),
                     ("out_size 257", dict(S=257)), ("open_2dj NULL", dict(det=None)), ("open_2dj_con NULL", dict(con=None)),
                     ("packed NULL", dict(packed=None)), ("no output", dict(odet=None, ocon=None))]:
        assert call(**kw) == EINVAL, f"hifihr_ho3d_keypoints accepted {what}"
    if device == "cuda":
        torch.cuda.synchronize()
    G.intact("ho3d_keypoints refusals")
    assert kc._is_canary(odet) and kc._is_canary(ocon), "a refused call wrote an output"
    assert call() == 0 and call(ocon=None) == 0 and call(odet=None) == 0
    # an index outside the cache cannot be refused (it lives in device memory): that sample is zeros, its neighbour is served
    for outside in (n, -1):
        bad = G.inp(_dev(pack([outside, 2], [[0, 0, 8, 8]] * 2, center, scale), device))
        o2, c2 = G.out(B, 21, 2, fill=float("nan")), G.out(B, 21, fill=float("nan"))
        assert call(packed=bad, odet=o2, ocon=c2) == 0
        assert float(o2[0].abs().max()) == 0.0 and float(c2[0].abs().max()) == 0.0 and torch.equal(c2[1].cpu(), con[2].cpu())
        want = crop_window_ref(det.cpu().numpy(), np.asarray([2]), center[1:], scale[1:], S)
        assert np.array_equal(o2[1].cpu().numpy().view(np.int32), want[0].view(np.int32))
    G.intact("ho3d_keypoints, index outside the cache")


# ---- 2. metric depth through the crop box ----------------------------------------------------------------------------------------
DEPTH_FRAMES = [(48, 64), (37, 53)]
DEPTH_SIZES = [1, 7, 16]
DEPTH_SCALE = 0.00012498664727900177


def depth_boxes(FH, FW):
    """-> [(x0, y0, x1, y1), whether Pillow is asked]: inside, over every edge and corner, larger than the frame, one pixel, wholly outside;
    then the boxes that give zeros by definition (empty, inverted, longer than HIFIHR_HO3D_MAX_WINDOW)."""
    ok = [(5, 7, 21, 23), (3, 4, 40, 30), (0, 0, FW, FH),
          (-10, 6, 20, 24), (FW - 12, 8, FW + 15, 30), (10, -9, 30, 15), (12, FH - 9, 33, FH + 18),                       # the four edges
          (-10, -6, 20, 24), (FW - 5, -7, FW + 9, 7), (-8, FH - 10, 12, FH + 10), (FW - 12, FH - 9, FW + 15, FH + 18),    # the four corners
          (-20, -30, FW + 25, FH + 20), (-3, -3, FW + 3, FH + 300),                                                       # larger than the frame
          (9, 11, 10, 12), (FW - 1, FH - 1, FW, FH), (FW + 3, 2, FW + 20, 19), (-400, -400, 400, 400)]
    zero = [(5, 5, 5, 9), (5, 5, 9, 5), (20, 20, 10, 30), (4, 30, 20, 10), (0, 0, MAX_WINDOW + 1, 10), (-5, -5, 5, MAX_WINDOW - 4)]
    return [(b, True) for b in ok] + [(b, False) for b in zero]


def depth_frames(n, FH, FW, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 65536, (n, FH, FW)).astype(np.uint16)
    a[rng.random((n, FH, FW)) < 0.2] = 0                                  # stored zeros: no measurement
    a[0, 0, 0], a[0, FH - 1, FW - 1] = 65535, 1
    return a


def depth_crop_formula(frames, idx, box, S, scale):
    """include/hifihr.h hifihr_ho3d_depth_crop, element by element."""
    n, FH, FW = frames.shape
    out = np.zeros((len(idx), S, S), F32)
    for b, (i, (x0, y0, x1, y1)) in enumerate(zip(idx, box)):
        w, h = int(x1) - int(x0), int(y1) - int(y0)
        if not (0 <= i < n) or w <= 0 or h <= 0 or w > MAX_WINDOW or h > MAX_WINDOW:
            continue
        for r in range(S):
            sy = int(y0) + int(np.floor((r + 0.5) * h / S))
            for q in range(S):
                sx = int(x0) + int(np.floor((q + 0.5) * w / S))
                if 0 <= sx < FW and 0 <= sy < FH:
                    out[b, r, q] = F32(frames[i, sy, sx]) * F32(scale)
    return out


def depth_crop_pillow(frame, box, S, scale):
    from PIL import Image
    im = Image.fromarray(frame)
    assert im.mode == "I;16", im.mode
    return np.array(im.crop(tuple(int(v) for v in box)).resize((S, S), Image.NEAREST)).astype(F32) * F32(scale)


def depth_crop_case(lib, device, FH, FW, S):
    n = 2
    frames = depth_frames(n, FH, FW, seed=FH * 1000 + S)
    boxes = depth_boxes(FH, FW)
    box = np.asarray([b for b, _ in boxes], np.int32)
    B = len(boxes)
    idx = np.arange(B, dtype=np.int32) % n
    G = kc.Guards(device)
    packed = G.inp(_dev(pack(idx, box, np.zeros((B, 2), F32), np.ones(B, F32)), device))
    d_frames = _dev(frames, device)
    outs = []
    for _ in range(2):
        out = G.out(B, S, S, fill=float("nan"))
        lib.ho3d_depth_crop(d_frames, packed, B, S, DEPTH_SCALE, out)
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    got = outs[0].cpu().numpy()
    want = depth_crop_formula(frames, idx, box, S, DEPTH_SCALE)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{FH}x{FW} -> {S}: depth_crop differs from the closed formula"
    covered = 0
    for b, (bx, ask) in enumerate(boxes):
        if ask:
            pil = depth_crop_pillow(frames[idx[b]], bx, S, DEPTH_SCALE)
            assert np.array_equal(got[b].view(np.int32), pil.view(np.int32)), f"{FH}x{FW} -> {S}, box {bx}: depth_crop differs from Pillow"
            covered += int((pil != 0).sum())
        else:
            assert not got[b].any(), f"box {bx} must give zeros"
    assert covered > 0
    # an index outside the cache: zeros; its neighbour is served
    bad = G.inp(_dev(pack([n, 1, -1], box[:3], np.zeros((3, 2), F32), np.ones(3, F32)), device))
    o = G.out(3, S, S, fill=float("nan"))
    lib.ho3d_depth_crop(d_frames, bad, 3, S, DEPTH_SCALE, o)
    o = o.cpu().numpy()
    assert not o[0].any() and not o[2].any() and np.array_equal(o[1], depth_crop_formula(frames, [1], box[1:2], S, DEPTH_SCALE)[0])
    G.intact("ho3d_depth_crop")


def depth_crop_refusal_case(lib, device):
    G = kc.Guards(device)
    n, FH, FW, B, S = 2, 12, 10, 2, 4
    frames = _dev(depth_frames(n, FH, FW, 3), device)
    packed = G.inp(_dev(pack([0, 1], [[0, 0, 8, 8]] * 2, np.zeros((2, 2), F32), np.ones(2, F32)), device))
    out = G.out(B, S, S)
    call = lambda frames=frames, n=n, FH=FH, FW=FW, packed=packed, B=B, S=S, out=out: lib._call(
        "hifihr_ho3d_depth_crop", frames, n, FH, FW, packed, B, S, DEPTH_SCALE, out)
    for what, kw in [("n = 0", dict(n=0)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("FH = 0", dict(FH=0)), ("FW = 0", dict(FW=0)),
                     ("out_size 0", dict(S=0)), ("out_size 257", dict(S=257)), ("depth NULL", dict(frames=None)), ("packed NULL", dict(packed=None)),
                     ("out NULL", dict(out=None))]:
        assert call(**kw) == EINVAL, f"hifihr_ho3d_depth_crop accepted {what}"
    if device == "cuda":
        torch.cuda.synchronize()
    G.intact("ho3d_depth_crop refusals")
    assert kc._is_canary(out), "a refused call wrote its output"
    assert call() == 0


# ---- 3. point selection ----------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(1, 1), (3, 5), (8, 8), (9, 15), (64, 65)]       # 9 x 15 = 135 pixels: two full words and a ragged third; 64 x 65: 65 words
SELECT_P = [1, 64, 257]
PATTERNS = ("none", "first", "last", "all", "checker", "masked_out", "random", "random_i64")


def select_inputs(H, W):
    """-> depths [B,H,W] f32, mask [B,H,W] f32 (1 everywhere unless the pattern uses it), B = len(PATTERNS)."""
    rng = np.random.default_rng(H * 100 + W)
    B = len(PATTERNS)
    d, m = np.zeros((B, H, W), F32), np.ones((B, H, W), F32)
    val = (0.2 + rng.random((B, H, W))).astype(F32)
    rr, qq = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b, p in enumerate(PATTERNS):
        if p == "first":
            d[b, 0, 0] = val[b, 0, 0]
        elif p == "last":
            d[b, -1, -1] = val[b, -1, -1]
        elif p == "all":
            d[b] = val[b]
        elif p == "checker":
            d[b] = np.where((rr + qq) % 2 == 0, val[b], 0)
        elif p == "masked_out":                                        # the mask removes every depth-valid pixel
            keep = rng.random((H, W)) < 0.5
            d[b], m[b] = np.where(keep, val[b], 0), np.where(keep, 0, 1)
        elif p.startswith("random"):
            d[b] = np.where(rng.random((H, W)) < 0.6, val[b], 0)
            d[b][rng.random((H, W)) < 0.05] = -1.0                       # a negative depth is no measurement either
            m[b] = np.where(rng.random((H, W)) < 0.7, rng.integers(1, 4, (H, W)), 0)
    return d, m


def valid_pixels(d, m):
    return [np.flatnonzero((d[b] > 0) & (m[b] != 0)) for b in range(d.shape[0])]


def select_draws(counts, P, seed):
    """Hand-picked draws first -- 1 - 2^-24, 0, k / n exactly and its float32 neighbours on both sides -- then seeded ones; [B,P] float32."""
    rng = np.random.default_rng(seed)
    rows = []
    for n in counts:
        n = max(int(n), 1)
        special = [F32(1) - F32(2.0 ** -24), F32(0)]
        for k in sorted({1, n // 2, n - 1} & set(range(1, n))):
            u = F32(k) / F32(n)
            special += [u, np.nextafter(u, F32(0)), np.nextafter(u, F32(1))]
        row = np.concatenate([np.asarray(special, F32), rng.random(max(P, 1)).astype(F32)])[:P]
        rows.append(np.minimum(row, F32(1) - F32(2.0 ** -24)))
    return np.stack(rows).astype(F32)


def select_ref(valid, draws):
    """-> (index [B,P] int32, count [B] int32): np.flatnonzero and the float32 product."""
    B, P = draws.shape
    idx = np.full((B, P), -1, np.int32)
    for b, v in enumerate(valid):
        n = len(v)
        if n:
            k = np.minimum(n - 1, np.floor(draws[b] * F32(n)).astype(np.int64))          # float32 x float32 -> float32
            idx[b] = v[k]
    return idx, np.asarray([len(v) for v in valid], np.int32)


def run_depth_points(lib, device, d, K, mask, draws, origin, mask_i64=False):
    """-> (points [B,P,3], count [B], index [B,P]) numpy; outputs start as canaries inside guard bands; two calls, the same bits."""
    B, P = draws.shape
    G = kc.Guards(device)
    dd, KK, uu = G.inp(_dev(d, device)), G.inp(_dev(np.asarray(K, F32), device)), G.inp(_dev(draws, device))
    mm = None
    if mask is not None:
        mm = _dev(mask.astype(np.int64), device) if mask_i64 else G.inp(_dev(mask.astype(F32), device))
    oo = None if origin is None else G.inp(_dev(np.asarray(origin, F32), device))
    runs = []
    for _ in range(2):
        pts, cnt, idx = G.out(B, P, 3, fill=float("nan")), G.out(B, dtype=torch.int32, fill=-99), G.out(B, P, dtype=torch.int32, fill=-99)
        lib.depth_points(dd, KK, mm, uu, oo, pts, cnt, idx)
        runs.append((pts, cnt, idx))
    assert not bool(torch.isnan(runs[0][0]).any()) and not bool((runs[0][1] == -99).any()) and not bool((runs[0][2] == -99).any()), "not written"
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(*runs)), "two calls with the same draws differ in their bits"
    G.intact("depth_points")
    return tuple(t.cpu().numpy() for t in runs[0])


def selection_case(lib, device, H, W, P):
    d, m = select_inputs(H, W)
    valid = valid_pixels(d, m)
    draws = select_draws([len(v) for v in valid], P, seed=H * W + P)
    want_idx, want_cnt = select_ref(valid, draws)
    K = np.tile(np.eye(3, dtype=F32), (d.shape[0], 1, 1))
    for i64 in (False, True):
        pts, cnt, idx = run_depth_points(lib, device, d, K, m, draws, None, mask_i64=i64)
        assert np.array_equal(cnt, want_cnt), (cnt, want_cnt)
        assert np.array_equal(idx, want_idx), f"{H}x{W} P={P}: chosen pixels differ in {int((idx != want_idx).sum())} draws"
        for b, p in enumerate(PATTERNS):
            if want_cnt[b] == 0:
                assert p in ("none", "masked_out") or H * W < 8, p
                assert not pts[b].any(), f"{p}: no valid pixel must give zeros"
            if p in ("first", "last"):
                assert want_cnt[b] == 1 and (pts[b] == pts[b, 0]).all() and pts[b, 0, 2] > 0, f"{p}: P copies of the one point"
        # with K = 1 the point is ((q + c) d, (r + c) d, d): the depth is the chosen pixel's own
        ok = want_idx >= 0
        flat = d.reshape(d.shape[0], -1)
        assert np.array_equal(pts[..., 2][ok], np.take_along_axis(flat, np.maximum(want_idx, 0), 1)[ok])
    # without a mask: the depth alone decides
    pts, cnt, idx = run_depth_points(lib, device, d, K, None, draws, None)
    v2 = valid_pixels(d, np.ones_like(m))
    w_idx, w_cnt = select_ref(v2, draws)
    assert np.array_equal(cnt, w_cnt) and np.array_equal(idx, w_idx)


# ---- 4. back-projection --------------------------------------------------------------------------------------------------------------
K_KINDS = ("upper", "ho3d_raw", "skew")


def intrinsics(kind, B, seed=0):
    rng = np.random.default_rng(seed)
    K = np.zeros((B, 3, 3), F32)
    K[:, 0, 0], K[:, 1, 1] = 100 + 50 * rng.random(B), 100 + 50 * rng.random(B)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 7 + rng.random(B), 4 + rng.random(B), 1
    if kind == "skew":
        K[:, 0, 1] = 3 * rng.standard_normal(B)
    if kind == "ho3d_raw":                                               # camMat . diag(1, -1, -1): third row (0, 0, -1)
        K = K * np.asarray([1, -1, -1], F32)
    return K.astype(F32)


def backproject_ref(d, K, rows, cols, c=PIXEL_CENTRE, origin=None):
    """float64, operation for operation as include/hifihr.h states it: adj(K) . ((q + c) d, (r + c) d, d) / det(K) - origin."""
    k = np.asarray(K, F32).astype(np.float64)
    (k00, k01, k02), (k10, k11, k12), (k20, k21, k22) = k
    c00, c01, c02 = k11 * k22 - k12 * k21, k02 * k21 - k01 * k22, k01 * k12 - k02 * k11
    c10, c11, c12 = k12 * k20 - k10 * k22, k00 * k22 - k02 * k20, k02 * k10 - k00 * k12
    c20, c21, c22 = k10 * k21 - k11 * k20, k01 * k20 - k00 * k21, k00 * k11 - k01 * k10
    det = (k00 * c00 + k01 * c10) + k02 * c20
    d = np.asarray(d, F32).astype(np.float64)
    x, y = (np.asarray(cols, np.float64) + c) * d, (np.asarray(rows, np.float64) + c) * d
    o = np.zeros(3) if origin is None else np.asarray(origin, F32).astype(np.float64)
    return np.stack([((c00 * x + c01 * y) + c02 * d) / det - o[0], ((c10 * x + c11 * y) + c12 * d) / det - o[1],
                     ((c20 * x + c21 * y) + c22 * d) / det - o[2]], -1)


def every_pixel_draws(n):
    """draws that pick the n valid pixels once each, in order: floor(((i + 0.5) / n) n) = i in float32 for the sizes used here."""
    u = ((np.arange(n, dtype=np.float64) + 0.5) / n).astype(F32)
    assert np.array_equal(np.floor(u * F32(n)).astype(np.int64), np.arange(n))
    return u


def backprojection_case(lib, device, kind, with_origin):
    B, H, W = 3, 9, 15
    rng = np.random.default_rng(7 + K_KINDS.index(kind))
    d = (0.3 + 0.6 * rng.random((B, H, W))).astype(F32)
    K = intrinsics(kind, B, seed=11)
    origin = (rng.standard_normal((B, 3)) * [0.05, 0.05, 0.5]).astype(F32) if with_origin else None
    draws = np.tile(every_pixel_draws(H * W), (B, 1))
    pts, cnt, idx = run_depth_points(lib, device, d, K, None, draws, origin)
    assert (cnt == H * W).all() and np.array_equal(idx, np.tile(np.arange(H * W, dtype=np.int32), (B, 1)))
    rows, cols = np.divmod(np.arange(H * W), W)
    worst = 0.0
    for b in range(B):
        want = backproject_ref(d[b].reshape(-1), K[b], rows, cols, origin=None if origin is None else origin[b])
        w32 = want.astype(F32)
        ulp = float(np.spacing(F32(np.abs(w32).max())))
        err = float(np.abs(pts[b].astype(np.float64) - w32.astype(np.float64)).max())
        worst = max(worst, err / ulp)
        assert err <= ulp, f"{kind}, sample {b}: {err:.3e} from the float64 restatement rounded to float32 (one unit in the last place: {ulp:.3e})"
        sign = -1.0 if kind == "ho3d_raw" else 1.0                    # d is the projective depth: z, or -z under HO-3D's raw third row
        assert np.allclose(want[:, 2] + (0 if origin is None else float(origin[b, 2])), sign * d[b].reshape(-1), rtol=1e-12)
    print(f"depth_points back-projection, K {kind}, origin {with_origin}: worst error {worst:.3f} units in the last place of the largest component")
    return worst


def depth_points_refusal_case(lib, device):
    G = kc.Guards(device)
    B, H, W, P = 2, 4, 6, 5
    d, K = G.inp(torch.rand(B, H, W) + 0.1), G.inp(torch.eye(3).repeat(B, 1, 1))
    u, m, o = G.inp(torch.rand(B, P) * 0.99), G.inp(torch.ones(B, H, W)), G.inp(torch.zeros(B, 3))
    pts, cnt, idx = G.out(B, P, 3), G.out(B, dtype=torch.int32), G.out(B, P, dtype=torch.int32)
    call = lambda d=d, K=K, m=m, u=u, o=o, B=B, H=H, W=W, P=P, pts=pts, cnt=cnt, idx=idx: lib._call(
        "hifihr_depth_points", d, K, m, 0, u, o, B, H, W, P, pts, cnt, idx)
    for what, kw in [("B = 0", dict(B=0)), ("B < 0", dict(B=-1)), ("P = 0", dict(P=0)), ("P < 0", dict(P=-3)), ("H = 0", dict(H=0)),
                     ("W = 0", dict(W=0)), ("H W > 512 x 512", dict(H=512, W=513)), ("H W far above it", dict(H=65536, W=65536)),
                     ("depths NULL", dict(d=None)), ("K NULL", dict(K=None)), ("draws NULL", dict(u=None)), ("points NULL", dict(pts=None)),
                     ("count NULL", dict(cnt=None))]:
        assert call(**kw) == EINVAL, f"hifihr_depth_points accepted {what}"
    if device == "cuda":
        torch.cuda.synchronize()
    G.intact("depth_points refusals")
    assert kc._is_canary(pts) and kc._is_canary(cnt) and kc._is_canary(idx), "a refused call wrote an output"
    assert call() == 0 and call(m=None, o=None, idx=None) == 0


# ---- 6. closed loop: render -> depth map -> points -> distance to the mesh ----------------------------------------------------------
LOOP_SIZE = 32
LOOP_Z = 12.0


def loop_scene():
    """A jittered 7 x 6 grid (tests/mesh_reg_cases.py) at depth ~12 under a camera that is neither centred nor square."""
    n, m = 7, 6
    verts = mr.grid_verts(n, m, B=1, jitter=0.3, seed=5)
    verts[..., 2] += LOOP_Z
    faces = mr.grid_faces(n, m)
    K = np.asarray([[58.0, 0.0, 15.3], [0.0, 52.0, 17.1], [0.0, 0.0, 1.0]], F32)
    return verts.contiguous(), faces, K


def camera_from_K(K, s):
    """Model.camera_from_K: (-2 fx / s, -2 fy / s, 1 - 2 cx / s, 1 - 2 cy / s)."""
    return torch.tensor([[-2.0 * K[0, 0] / s, -2.0 * K[1, 1] / s, 1.0 - 2.0 * K[0, 2] / s, 1.0 - 2.0 * K[1, 2] / s]], dtype=torch.float32)


def mean_d2_f64(points, verts, faces):
    """Mean squared distance of float64 points to the mesh (the restatement's own closest-point routine)."""
    a, ab, ac, abab, abac, acac = pr.face_records(np.asarray(verts, F32).astype(np.float64), faces)
    d2 = pr.closest(points[:, None, :] - a[None], ab[None], ac[None], abab[None], abac[None], acac[None])[3]
    return float(d2.min(1).mean())


def closed_loop_case(lib, device, surface_d2):
    """surface_d2(points f32 [1,N,3], verts f32 [1,V,3], faces) -> float: evaluate.point_to_surface on the device under test.
    -> (measured, float64 back-projection, bound, the restatement at c - 0.5)."""
    verts, faces, K = loop_scene()
    S = LOOP_SIZE
    cam = camera_from_K(K, S)
    with dc.Renderer(lib, faces, verts.shape[1], S, 1) as r:
        fid = dc.kernel_face_id(lib, device, r, verts, cam)
        depth, hits, _ = dc.run_depth(lib, device, r, verts, cam, fid.cpu())
    depth, hits = depth.numpy(), hits.numpy()
    covered = np.flatnonzero(hits[0] > 0)
    n = len(covered)
    assert n > 200 and (depth[0].reshape(-1)[covered] > 0).all(), n
    draws = every_pixel_draws(n)[None]
    pts, cnt, idx = run_depth_points(lib, device, depth, K[None], (hits > 0).astype(F32), draws, None)
    assert cnt[0] == n and np.array_equal(idx[0], covered)
    got = surface_d2(pts, verts.numpy(), faces)
    rows, cols = np.divmod(covered, S)
    dsel = depth[0].reshape(-1)[covered]
    v = verts[0].numpy()
    f64 = mean_d2_f64(backproject_ref(dsel, K, rows, cols), v, faces)
    wrong = mean_d2_f64(backproject_ref(dsel, K, rows, cols, c=PIXEL_CENTRE - 0.5), v, faces)
    bound = 2.0 * f64 + (8.0 * 2.0 ** -24 * float(v[:, 2].max())) ** 2
    print(f"depth_points closed loop ({n} covered pixels of {S} x {S}): point_to_surface {got:.6e}, float64 back-projection {f64:.6e}, "
          f"bound {bound:.6e}, at c - 0.5: {wrong:.6e}")
    assert got <= bound, f"the points do not lie on the mesh: {got:.3e} > {bound:.3e}"
    assert wrong > 1000.0 * bound, f"half a pixel off must miss the bound by orders of magnitude: {wrong:.3e} against {bound:.3e}"
    return got, f64, bound, wrong


def lib_surface_d2(lib, device):
    """The kernels evaluate.point_to_surface runs (hifihr_point_mesh_fwd, points -> faces only), through the C ABI."""
    import point_mesh_cases as pmc
    return lambda p, v, faces: float(pmc.run_kernels(lib, device, p, v, faces, 1.0, 0.0, grads="p")["sums"][0, 0]) / p.shape[1]
