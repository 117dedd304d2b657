"""The C ABI contract of the entries behind the network's heads on the hostsim emulator: Procrustes, the HO-3D and FreiHAND data paths, Adam,
texture PCA, the fused losses, the small loss / light entries, MANO and generic skinning -- on fixed lists that sit on the kernels' own
boundaries (workgroup widths, batch tiles, vector widths, grid caps, filter-tap counts).  An entry either refuses a call (HIFIHR_EINVAL,
nothing launched, every output untouched) or matches a float64 reference inside guard bands, twice (tests/kernel_cases.py, "The tail
contract").  The GPU half runs the same lists, and a few larger shapes, in tests/test_gpu_tail.py and tests/test_gpu_mano.py."""
import numpy as np
import pytest
import torch

import kernel_cases as kc

# ---- Procrustes: (B, N, family); 256 is the workgroup width ---------------------------------------------------------------------------------
PROCRUSTES_CASES = [(1, N, "generic") for N in (1, 2, 3, 4, 21, 255, 256, 257, 778)]
PROCRUSTES_CASES += [(3, 21, f) for f in kc.PROCRUSTES_FAMILIES]
PROCRUSTES_CASES += [(1, 50, "gt_planar"), (1, 50, "gt_line"), (1, 778, "similar"), (3, 257, "reflect"), (1, 4, "gt_planar_fp32"), (1, 3, "gt_point")]
PROCRUSTES_CASES += [(0, 21, "generic"), (3, 0, "generic")]                                                           # refused

# ---- HO-3D: (frame H, W, out_size, boxes (x0, y0, x1, y1), mode) -------------------------------------------------------------------------------
HO3D_CASES = [
    (48, 64, 32, ((5, 7, 15, 17),), "ok"),                                  # up-sampling
    # (taps as Pillow's own tables count them, kc.ho3d_taps_needed: the widest row of any table of the case)
    (100, 120, 16, ((10, 10, 70, 70),), "ok"),                              # 60 -> 16: 15 bicubic taps
    (100, 120, 16, ((10, 10, 72, 72),), "ok"),                              # 62 -> 16: exactly 16 bicubic taps, the old table's width
    (100, 120, 16, ((0, 0, 67, 67),), "ok"),                                # 67 -> 16: 17 bicubic taps, one more than the old table held (the outermost
                                                                            # coefficient is small: the detection test shows that this box exposes it)
    (200, 200, 16, ((20, 30, 142, 152),), "ok"),                            # 122 -> 16: 16 bilinear taps (31 bicubic)
    (200, 200, 16, ((0, 0, 130, 130),), "ok"),                              # 130 -> 16: 17 bilinear taps
    (480, 640, 128, ((-80, -160, 720, 640),), "ok"),                        # 800 -> 128: 25 bicubic taps
    (480, 640, 64, ((0, 0, 640, 480),), "ok"), (480, 640, 7, ((0, 0, 640, 480),), "ok"),             # the whole frame
    (48, 64, 8, ((5, 5, 6, 6),), "ok"),                                     # a one-pixel box
    (48, 64, 16, ((5, 5, 45, 20), (5, 5, 20, 45)), "ok"),                   # non-square boxes
    (48, 64, 16, ((-10, 5, 30, 45), (40, 5, 80, 45), (5, -10, 45, 30), (5, 30, 45, 70)), "ok"),      # off each frame edge
    (48, 64, 16, ((100, 100, 140, 140),), "ok"),                            # fully outside the frame
    (48, 64, 16, ((-20, -20, 100, 100),), "ok"),                            # the frame inside the box
    (48, 64, 1, ((0, 0, 40, 40),), "ok"), (48, 64, 7, ((3, 3, 30, 30),), "ok"), (48, 64, 256, ((3, 3, 30, 30),), "ok"),
    (480, 640, 16, ((-80, -160, 720, 640),), "ok"),                         # 800 -> 16: 200 taps of the 201 a table row holds
    (48, 64, 16, ((10, 10, 10, 30), (30, 10, 10, 30), (10, 10, 30, 5), (3, 3, 30, 30)), "ok"),       # empty / inverted boxes next to a good one: zeros
    (480, 640, 16, ((-80, -160, 721, 640), (0, 0, 640, 480)), "ok"),        # 801 pixels: above the window limit, zeros
    (48, 64, 0, ((3, 3, 30, 30),), "ok"), (48, 64, 257, ((3, 3, 30, 30),), "ok"), (48, 64, 16, (), "ok"),                # refused: out_size, B = 0
    (0, 64, 16, ((3, 3, 30, 30),), "ok"),
    (48, 64, 16, ((3, 3, 30, 30),), "short_ws"), (48, 64, 16, ((3, 3, 30, 30),), "no ws"), (48, 64, 16, ((3, 3, 30, 30),), "no packed"),
] + [(48, 64, 16, ((3, 3, 30, 30),), f"no_{k}") for k in ("img_crop", "hand_mask_crop", "K_crop", "uv21_crop", "xyz21")]

# ---- FreiHAND: (H, W, J, V); every map of kc.FREIHAND_MAPS, root_id in {-1, 0, J - 1} and the refused calls run inside each ----------------------
FREIHAND_GEOMS = [(1, 4, 0, 0), (17, 33, 1, 50), (32, 32, 21, 50), (40, 24, 21, 0)]

# ---- Adam: (n, weight decay, grad_scale); 4 floats per lane, 1024 per workgroup ------------------------------------------------------------------
ADAM_CASES = [(1, 0.0, 1.0), (3, 0.01, 0.5), (4, 0.0, 0.5), (5, 0.01, 1.0), (1023, 0.0, 1.0), (1024, 0.01, 0.5), (1027, 0.0, 0.5), (1027, 0.01, 1.0)]

# ---- texture PCA: (B, K, n, with_mean); batch tile 16, K <= 32, n % 4 == 0 -----------------------------------------------------------------------
TEXPCA_GEOMS = [(1, 1, 4, True), (15, 10, 8, False), (16, 31, 1020, True), (17, 32, 1024, True), (33, 10, 1028, False), (1, 10, 2336, True),
                (17, 1, 2336, False),
                (1, 0, 8, True), (1, 33, 8, True), (2, 4, 0, True), (2, 4, 2, True), (2, 4, 6, True), (2, 4, 2334, True), (0, 4, 8, True)]      # refused

# ---- geometry terms: (B, J, V, F, NS, NP, mse, special); 256 threads per sample, 3 * 86 > 256 -----------------------------------------------------
GEOM_CASES = [(1, 1, 1, 0, 0, 0, False, "random"), (2, 21, 85, 1, 10, 48, True, "random"), (33, 86, 86, 257, 257, 0, False, "zero_edges"),
              (1, 21, 256, 1538, 10, 48, False, "identical"), (2, 21, 257, 257, 0, 48, True, "zero_edges"), (2, 21, 778, 1538, 10, 48, False, "zero_edges"),
              (1, 21, 778, 1538, 10, 48, True, "identical"),
              (0, 21, 8, 0, 0, 0, False, "random"), (1, 0, 8, 0, 0, 0, False, "random"), (1, 21, 0, 0, 0, 0, False, "random")]                 # refused

# ---- joint terms: (B, mse, 2-D set, 3-D set, special, J); 13 * 20 bones > 256 threads, 65 samples = two backward workgroups ------------------------
JOINT_CASES = [(1, False, True, True, "random", 21), (12, True, True, True, "random", 21), (13, False, True, False, "zero_bones", 21),
               (64, True, False, True, "zero_bones", 21), (65, False, True, True, "identical", 21), (65, True, True, True, "zero_bones", 21),
               (2, False, True, True, "random", 20), (2, False, True, True, "random", 22), (0, False, True, True, "random", 21),                # refused
               (2, False, False, False, "random", 21)]

# ---- photometric terms: (B, H, W, seg kind); four pixels per lane ---------------------------------------------------------------------------------
PHOTO_CASES = [(1, 1, 4, "binary"), (1, 2, 2, "ints"), (2, 16, 16, "binary"), (3, 12, 20, "binary"), (5, 23, 44, "ints"), (2, 16, 16, "nan"),
               (1, 3, 3, "binary"), (1, 2, 3, "binary"), (0, 4, 4, "binary"), (1, 0, 4, "binary"), (1, 4, 0, "binary")]                         # refused

# ---- the small entries ----------------------------------------------------------------------------------------------------------------------------
TOTAL_CASES = [((5,), None, "ok"), ((5, 3), (5, 4), "ok"), ((5, 3, 1), (5, 4, 1), "ok"), ((0, 64, 1, 2), None, "ok"), ((1,), (1,), "ok"),
               ((), None, "ok"), ((1, 1, 1, 1, 1), None, "ok"), ((65,), None, "ok"), ((3,), (2,), "ok"), ((3,), (65,), "ok"),                   # refused
               ((3, 2), None, "null"), ((3, 2), None, "null_total")]
LIGHT_CASES = [1, 7, 300, 0]

# ---- MANO: (tables, B, pose family, root_id); LBS: (V, J, S, B) ------------------------------------------------------------------------------------
MANO_CASES = [("synth", 1, "zero", 9), ("synth", 3, "0.6", 9), ("dense", 1, "1e-7", 0), ("synth", 1, "1e-4", -1), ("dense", 3, "3.0", 20),
              ("synth", 1, "root0", 9), ("dense", 3, "rootpi", 9), ("synth", 0, "0.6", 9),
              ("synth", 1, "0.6", 21), ("synth", -1, "0.6", 9)]                                                                                    # refused
LBS_CASES = [(64, 1, 0, 3), (257, 32, 32, 1), (300, 7, 5, 3), (64, 1, 0, 0), (64, 1, 0, -1)]

_ids = lambda g: "-".join(str(v).replace(" ", "") for v in g)[:80] if isinstance(g, tuple) else str(g)

EXPECT_LAUNCHED = {
    "geom_loss_fwd_kernel", "geom_loss_finish_kernel", "geom_loss_bwd_kernel", "photo_loss_fwd_kernel", "photo_loss_finish_kernel",
    "photo_loss_bwd_kernel", "sil_post_kernel", "loss_total_fwd_kernel", "loss_total_bwd_kernel", "joint_terms_fwd_kernel", "joint_terms_bwd_kernel",
    "light_split_fwd_kernel", "light_split_bwd_kernel", "adam_kernel", "adam_kernel_counted", "texpca_fwd_kernel", "texpca_bwd_kernel",
    "procrustes_kernel", "freihand_augment_kernel", "freihand_augment4_kernel", "freihand_batch_meta_kernel", "ho3d_coeff_kernel",
    "ho3d_resample_kernel", "ho3d_meta_kernel", "mano_fwd_kernel", "mano_bwd_kernel", "mano_joints_fwd_kernel", "mano_joints_bwd_kernel",
    "lbs_fwd_kernel", "lbs_bwd_vert_kernel", "lbs_bwd_chain_kernel"}
TAIL_ENTRIES = kc.TAIL_CONTRACT_ENTRIES

_DONE = {}
_TABLES = {}


def tail_tables(name):
    """"synth": hifihr_amd.mano_tables.synthetic_mano_tables(0); "dense": the shipped MANO-structured tables (conftest.mano_dense)."""
    if not _TABLES:
        import dataclasses
        import os
        from hifihr_amd.mano_tables import synthetic_mano_tables
        g = dict(np.load(os.path.join(kc.REPO, "tests", "golden", "mano_dense.npz")))
        _TABLES["synth"] = synthetic_mano_tables(0)
        _TABLES["dense"] = dataclasses.replace(synthetic_mano_tables(0), weights=g["weights"], hands_components=g["hands_components"],
                                               hands_mean=g["hands_mean"], source="mano-dense(seed=6)")
    return _TABLES[name]


def tail_runners(device):
    """family -> (lib, case) -> accepted?  (the GPU half, tools/layer_contract_c.py and tools/asan_hostsim.py walk the same lists through it)"""
    return {
        "procrustes": lambda lib, g: kc.procrustes_contract_case(lib, device, *g, seed=g[1] + len(g[2])),
        "ho3d": lambda lib, g: kc.ho3d_contract_case(lib, device, *g, seed=g[2]),
        "freihand": lambda lib, g: kc.freihand_contract_case(lib, device, *g, seed=sum(g)),
        "adam": lambda lib, g: kc.adam_contract_case(lib, device, *g, seed=g[0]),
        "texpca": lambda lib, g: kc.texpca_contract_case(lib, device, *g, seed=sum(g[:3])),
        "geom": lambda lib, g: kc.geom_contract_case(lib, device, *g, seed=sum(g[:6])),
        "joint": lambda lib, g: kc.joint_contract_case(lib, device, g[0], g[1], g[2], g[3], g[4], J=g[5], seed=g[0]),
        "photo": lambda lib, g: kc.photo_contract_case(lib, device, *g, seed=sum(g[:3])),
        "total": lambda lib, g: kc.loss_total_contract_case(lib, device, list(g[0]), g[1], g[2], seed=len(g[0])),
        "light": lambda lib, g: kc.light_split_contract_case(lib, device, g, seed=g),
        "mano": lambda lib, g: kc.mano_contract_case(lib, device, tail_tables(g[0]), g[1], g[2], g[3], seed=5 + g[1]),
        "lbs": lambda lib, g: kc.lbs_contract_case(lib, device, *g, seed=sum(g)),
    }


LISTS = {"procrustes": PROCRUSTES_CASES, "ho3d": HO3D_CASES, "freihand": FREIHAND_GEOMS, "adam": ADAM_CASES, "texpca": TEXPCA_GEOMS,
         "geom": GEOM_CASES, "joint": JOINT_CASES, "photo": PHOTO_CASES, "total": TOTAL_CASES, "light": LIGHT_CASES, "mano": MANO_CASES,
         "lbs": LBS_CASES}
_RUNNERS = tail_runners("cpu")


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.fixture(scope="module")
def tally():
    yield None
    kc.layer_contract_report("the tail entries on the emulator", TAIL_ENTRIES)


def _run(lib, family, case):
    """One case, once per session."""
    key = (family, case)
    if key not in _DONE:
        _DONE[key] = _RUNNERS[family](lib, case)
    return _DONE[key]


@pytest.mark.parametrize("case", PROCRUSTES_CASES, ids=_ids)
def test_procrustes_on_every_point_set(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "procrustes", case) == kc.procrustes_contract_expect(*case[:2])


@pytest.mark.parametrize("case", HO3D_CASES, ids=_ids)
def test_ho3d_batch_on_every_window(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "ho3d", case) == kc.ho3d_contract_expect(*case)


@pytest.mark.parametrize("case", FREIHAND_GEOMS, ids=_ids)
def test_every_freihand_entry_on_every_map(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "freihand", case)


@pytest.mark.parametrize("case", ADAM_CASES, ids=_ids)
def test_every_adam_entry_on_one_trajectory(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "adam", case)


@pytest.mark.parametrize("case", TEXPCA_GEOMS, ids=_ids)
def test_texture_pca_on_every_geometry(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "texpca", case) == kc.texpca_contract_expect(*case[:3])


@pytest.mark.parametrize("case", GEOM_CASES, ids=_ids)
def test_geometry_terms_on_every_geometry(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "geom", case) == kc.geom_contract_expect(*case[:6])


@pytest.mark.parametrize("case", JOINT_CASES, ids=_ids)
def test_joint_terms_on_every_batch(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "joint", case) == kc.joint_contract_expect(case[0], case[5], case[2], case[3])


@pytest.mark.parametrize("case", PHOTO_CASES, ids=_ids)
def test_photometric_terms_on_every_image_size(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "photo", case) == kc.photo_contract_expect(*case[:3])


@pytest.mark.parametrize("case", TOTAL_CASES, ids=_ids)
def test_loss_total_on_every_part_list(hostsim_lib, tally, case):
    _run(hostsim_lib, "total", case)


@pytest.mark.parametrize("case", LIGHT_CASES, ids=_ids)
def test_light_split_on_every_batch(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "light", case) == (case > 0)


@pytest.mark.parametrize("case", MANO_CASES, ids=_ids)
def test_every_mano_entry_on_every_pose_family(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "mano", case) == (case[1] >= 0 and case[3] < 21)


@pytest.mark.parametrize("case", LBS_CASES, ids=_ids)
def test_lbs_on_every_table_size(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "lbs", case) == (case[3] >= 0)


def test_procrustes_reference_is_scipys():
    """The float64 restatement the Procrustes cases compare with equals scipy's align_w_scale route wherever R is unique, and its distances
    everywhere (scipy and numpy call the same LAPACK driver; the check is of the restatement)."""
    sl = pytest.importorskip("scipy.linalg")
    for B, N, family in PROCRUSTES_CASES:
        if not kc.procrustes_contract_expect(B, N):
            continue
        pred, gt = kc.procrustes_contract_inputs(family, B, N, N + len(family))
        ref = kc.procrustes_contract_ref(pred, gt)
        for b in range(B):
            m1, m2 = gt[b].double().numpy(), pred[b].double().numpy()
            t1, t2 = m1.mean(0), m2.mean(0)
            a, c = m1 - t1, m2 - t2
            s1 = np.linalg.norm(a) + 1e-8
            a = a / s1
            c = c / (np.linalg.norm(c) + 1e-8)
            R, s = sl.orthogonal_procrustes(a, c)
            al = c.dot(R.T) * s * s1 + t1
            tol = 1e-12 * max(1.0, float(np.abs(al).max()))
            assert not ref["unique"][b] or float(np.abs(al - ref["aligned"][b]).max()) <= tol, (B, N, family)
            assert float(np.abs(np.linalg.norm(al - m1, axis=1) - ref["dist"][b]).max()) <= tol, (B, N, family)


def test_ho3d_and_freihand_references_are_pillows():
    """The two pixel references against Pillow itself: crop + resize on the frames of the HO-3D cases, Image.transform on the FreiHAND maps."""
    Image = pytest.importorskip("PIL.Image")
    for FH, FW, S, boxes, mode in HO3D_CASES:
        if not kc.ho3d_contract_expect(FH, FW, S, boxes, mode):
            continue
        frames, masks = kc.ho3d_contract_frames(3, FH, FW)
        idx = [(2 * b + 1) % 3 for b in range(len(boxes))]
        ref_img, ref_mask = kc.ho3d_contract_ref(frames, masks, idx, boxes, S)
        for b, box in enumerate(boxes):
            if box[2] - box[0] <= 0 or box[3] - box[1] <= 0 or max(box[2] - box[0], box[3] - box[1]) > kc.HO3D_MAX_WINDOW:
                continue                                                     # (Pillow raises / the entry's own rule)
            im = Image.fromarray(frames[idx[b], :, :, :3]).crop(box).resize((S, S), Image.BILINEAR)
            mk = Image.fromarray(masks[idx[b]]).crop(box).resize((S, S), Image.BICUBIC)
            assert np.array_equal(np.asarray(im), ref_img[b]) and np.array_equal(np.asarray(mk), ref_mask[b]), (FH, FW, S, box)
    rng = np.random.default_rng(0)
    for H, W, _, _ in FREIHAND_GEOMS:
        src = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        for name, m in kc.FREIHAND_MAPS.items():
            coefs = tuple(float(v) for v in m(H, W))
            want = np.asarray(Image.fromarray(src[0]).transform((W, H), Image.AFFINE, coefs, Image.NEAREST))
            assert np.array_equal(kc.pil_affine_nearest_ref(src, [0], [kc.pil_affine_fixed(coefs)])[0], want), (H, W, name)


def test_detection_the_comparator_notices_one_missing_contribution():
    """No kernel involved: a float64 reference with ONE contribution removed -- a point, a tap, a basis row, a texel, a vertex, a face, a
    bone, a pixel quad, a gradient element -- must fail the comparator on every accepted case of the lists."""
    missed = []
    for B, N, family in PROCRUSTES_CASES:
        if kc.procrustes_contract_expect(B, N):
            pred, gt = kc.procrustes_contract_inputs(family, B, N, N + len(family))
            ref = kc.procrustes_contract_ref(pred, gt)
            worst = int(ref["dist"][0].argmax())
            gmax = gt.abs().amax((1, 2))
            if ref["dist"][0, worst] > 1e-9 * float(gmax[0]):                # (N = 1, gt a single point: every distance is zero to rounding)
                bad = kc.procrustes_contract_ref(pred, gt, drop_point=worst)
                missed += [("procrustes", B, N, family)] if kc.procrustes_err_passes(bad["err_sum"][:1], ref["err_sum"][:1], N, gmax[:1]) else []
    above16 = 0
    for FH, FW, S, boxes, mode in HO3D_CASES:                              # the tables cut to 16 taps, as the kernel's were
        if kc.ho3d_contract_expect(FH, FW, S, boxes, mode):
            need = kc.ho3d_taps_needed(boxes, S)
            if max(need) > 16:
                above16 += 1
                frames, masks = kc.ho3d_contract_frames(3, FH, FW)
                idx = [(2 * b + 1) % 3 for b in range(len(boxes))]
                ri, rm = kc.ho3d_contract_ref(frames, masks, idx, boxes, S)
                ci, cm = kc.ho3d_contract_ref(frames, masks, idx, boxes, S, max_taps=16)
                ok_i, ok_m = kc.ho3d_pixels_match(torch.from_numpy(ri).permute(0, 3, 1, 2).float().div(255),
                                                  torch.round(torch.from_numpy(rm).float().div(255)).unsqueeze(1), ci, cm)
                missed += [("ho3d frame", FH, FW, S, boxes)] if need[0] > 16 and ok_i else []
                missed += [("ho3d mask", FH, FW, S, boxes)] if need[1] > 16 and ok_m else []
    assert above16 >= 6
    fails = lambda q, bad: not kc.tail_passes(q[0], bad[2], q[2], q[1], q[3] if len(q) > 3 else 0.0)
    for g in TEXPCA_GEOMS:
        if kc.texpca_contract_expect(*g[:3]):
            inp = kc.texpca_contract_inputs(*g[:3], sum(g[:3]))
            ref = kc.texpca_contract_ref(inp, g[3])
            bad_k = kc.texpca_contract_ref(inp, g[3], drop_row=g[1] - 1)      # one basis row of the forward's sum
            missed += [("texpca tex", g)] if not fails(ref["tex"], bad_k["tex"]) else []
            gz = inp["g"].clone()
            gz[:, g[2] - 1] = 0                                              # one texel of the backward's sum
            bad_n = kc.texpca_contract_ref(dict(inp, g=gz), g[3])
            missed += [("texpca dcoef", g)] if not fails(ref["dcoef"], bad_n["dcoef"]) else []
    for g in GEOM_CASES:
        if kc.geom_contract_expect(*g[:6]) and g[7] != "identical":
            inp = kc.geom_contract_inputs(*g[:6], g[7], sum(g[:6]))
            ref, gref = kc.geom_contract_ref(inp, g[6])
            bad, gbad = kc.geom_contract_ref(inp, g[6], drop_vertex=g[2] - 1, drop_face=(g[3] - 1) if inp["faces"] is not None else None)
            missed += [("geom vert_3d", g)] if not fails(ref[1], bad[1]) else []
            missed += [("geom gv", g)] if not fails(gref["gv"], gbad["gv"]) else []
            if inp["faces"] is not None:
                missed += [("geom edge", g)] if not fails(ref[2], bad[2]) else []
    for g in JOINT_CASES:
        if kc.joint_contract_expect(g[0], g[5], g[2], g[3]) and g[4] != "identical":
            inp = kc.joint_contract_inputs(g[0], g[4], g[0])
            ref, gref = kc.joint_contract_ref(inp, g[1], g[2], g[3])
            bad, gbad = kc.joint_contract_ref(inp, g[1], g[2], g[3], drop_bone=0)
            Ls = (g[0] * 42, g[0] * 40, g[0] * 60)
            for k, name in ((1, "g2"), (2, "g3")):
                if (g[2], g[2], g[3])[k]:
                    missed += [("joint term", g, k)] if kc.tail_passes("joint_out", bad[k], ref[k], Ls[k]) else []
                    missed += [("joint grad", g, name)] if kc.tail_passes("joint_grad", gbad[name][-1], gref[name][-1], 6) else []      # (per sample, as the case compares)
    for g in PHOTO_CASES:
        if kc.photo_contract_expect(*g[:3]) and g[3] != "nan":
            inp = kc.photo_contract_inputs(*g[:3], g[3], sum(g[:3]))
            ref, bad = kc.photo_contract_ref(inp), kc.photo_contract_ref(inp, drop_quad=True)
            for name in ("tex", "sil"):
                missed += [("photo", g, name)] if not fails(ref[name], bad[name]) else []
            out = torch.cat([ref[k][2] for k in ("tex", "mrgb", "sil", "dm")]).float()
            q = kc.photo_contract_bwd_ref(inp, ref["re_m"][2].float(), ref["mk"].float(), out, True, True)
            qb = kc.photo_contract_bwd_ref(inp, ref["re_m"][2].float(), ref["mk"].float(), out, True, True, drop_quad=True)
            missed += [("photo grad", g)] if not fails(q, qb) else []
    for n, wd, gs in ADAM_CASES:
        inp = kc.adam_contract_inputs(n, n)
        ref = kc.adam_contract_ref(inp["p"], inp["g"][0], inp["m"], inp["v"], 1000, wd, gs)
        bad = kc.adam_contract_ref(inp["p"], inp["g"][0], inp["m"], inp["v"], 1000, wd, gs, drop=n - 1)
        for kind, b_, r in zip(("adam_p", "adam_m", "adam_v"), bad, ref):
            missed += [("adam", n, wd, gs, kind)] if kc.adam_passes(kind, b_, r)[0] else []
    for name, B, family, root_id in MANO_CASES:
        if B > 0 and root_id < 21 and family != "zero":
            inp = kc.mano_contract_inputs(B, family, 5 + B)
            rv, rj, rg = kc.mano_layer_ref(tail_tables(name), inp)
            worst = int(inp["wv"].abs().sum((0, 2)).argmax())
            _, _, bg = kc.mano_layer_ref(tail_tables(name), inp, drop_vertex=worst)
            missed += [("mano gbeta", name, B, family)] if kc.tail_passes("mano_g", bg["v"][1] + bg["j"][1], rg["v"][1] + rg["j"][1], 778) else []
            qjr, _, _, _ = kc.mano_joints_ref(tail_tables(name), rv, inp, root_id)
            bjr, _, _, _ = kc.mano_joints_ref(tail_tables(name), rv, inp, root_id, drop_vertex=int(np.abs(tail_tables(name).J_regressor).sum(0).argmax()))
            missed += [("mano joints_rel", name, B, family)] if kc.tail_passes("mano_j", bjr, qjr, 778) else []
    for V, J, S, B in LBS_CASES:
        if B > 0:
            tabs = kc.random_lbs_tables(V, J, S, V + J + S + B)
            inp = kc.lbs_contract_inputs(tabs, B, V + J + S + B)
            _, _, rg, rA = kc.lbs_contract_ref(tabs, inp)
            _, _, bg, bA = kc.lbs_contract_ref(tabs, inp, drop_vertex=int(inp["wv"].abs().sum((0, 2)).argmax()))
            missed += [("lbs gtheta", V, J, S, B)] if kc.tail_passes("lbs_g", bg["v"][0] + bg["j"][0], rg["v"][0] + rg["j"][0], V) else []
            missed += [("lbs scratch", V, J, S, B)] if kc.tail_passes("lbs_g", bA, rA, V) else []
    assert not missed, f"the comparator accepts a reference with one contribution removed: {missed}"


def test_no_bound_is_looser_than_the_family_case_it_replaces():
    """c sqrt(L) max|ref| is capped by the older case's tolerance for the same quantity (kc.TAIL_LEGACY; the cap column of LAYER_CONTRACT_C
    is what that tolerance is relative to max|ref|, where it is relative)."""
    kinds = set(kc.TAIL_CONTRACT_KINDS)
    assert kinds <= set(kc.LAYER_CONTRACT_C) and set(kc.TAIL_LEGACY) | {"adam_p", "adam_m", "adam_v"} == kinds
    for kind in sorted(kinds):
        c, cap = kc.LAYER_CONTRACT_C[kind]
        assert 0 < c <= cap, kind
        for scale in (1e-3, 1.0, 50.0):
            ref = torch.full((3,), scale, dtype=torch.float64)
            for L in (1, 778, 10 ** 12):
                if kind in kc.TAIL_LEGACY:
                    assert kc.tail_bound(kind, ref, L) <= kc.TAIL_LEGACY[kind](ref, L), (kind, scale, L)
    ref = torch.tensor([0.0, 1.0, -3.0], dtype=torch.float64)                # Adam: never above adam_case's 2e-6 + 1e-5 |p| per element
    assert kc.adam_passes("adam_p", ref + 0.99 * (2e-6 + 1e-5 * ref.abs()), ref)[0] is False or kc.LAYER_CONTRACT_C["adam_p"][0] * 3 >= 2e-6
    assert not kc.adam_passes("adam_p", ref + 1.01 * (2e-6 + 1e-5 * ref.abs()), ref)[0]


def test_the_lists_reach_every_kernel_every_entry_and_both_answers(hostsim_lib):
    """A list edit that stops reaching a kernel, an entry's accepted or refused side, or a size class fails here."""
    lib = hostsim_lib
    for family, cases in LISTS.items():                                      # (whatever a -k selection left out runs now)
        for c in cases:
            _run(lib, family, c)
    assert EXPECT_LAUNCHED <= kc.TAIL_LAUNCHED, f"no case reaches {sorted(EXPECT_LAUNCHED - kc.TAIL_LAUNCHED)}"
    for e in TAIL_ENTRIES:
        row = kc.LAYER_CONTRACT_LOG.get(e, [0, 0, 0.0])
        assert row[0] > 0 and row[1] > 0, f"{e}: accepted {row[0]}, refused {row[1]} calls"
    for family in ("procrustes", "ho3d", "texpca", "geom", "joint", "photo", "light", "mano", "lbs"):
        assert {bool(_DONE[(family, c)]) for c in LISTS[family]} == {True, False}, family
    # the classes the lists exist for
    acc = [c for c in PROCRUSTES_CASES if kc.procrustes_contract_expect(*c[:2])]
    assert {c[1] for c in acc} >= {1, 2, 3, 4, 21, 255, 256, 257, 778} and {c[0] for c in acc} == {1, 3} and {c[2] for c in acc} == set(kc.PROCRUSTES_FAMILIES)
    ho = [c for c in HO3D_CASES if kc.ho3d_contract_expect(*c)]
    taps = {kc.ho3d_taps_needed(c[3], c[2]) for c in ho}
    assert {t[1] for t in taps} >= {15, 16, 17, 25, 200} and {t[0] for t in taps} >= {16, 17}
    assert {c[2] for c in ho} >= {1, 7, 8, 16, 32, 64, 128, 256} and {c[2] for c in HO3D_CASES} >= {0, 257}
    edges = [b for c in ho for b in c[3]]
    assert any(b[2] <= b[0] for b in edges) and any(b[3] <= b[1] for b in edges) and any(b[2] - b[0] > kc.HO3D_MAX_WINDOW for b in edges)
    assert any(b[2] - b[0] == kc.HO3D_MAX_WINDOW for b in edges) and any(b[2] - b[0] == 1 for b in edges) and any(b[2] - b[0] != b[3] - b[1] > 0 for b in edges)
    assert any(b[0] < 0 < b[2] for b in edges) and any(b[1] < 0 < b[3] for b in edges) and any(b[0] >= 64 for b in edges)
    assert {c[4] for c in HO3D_CASES} >= {"short_ws", "no_img_crop", "no_hand_mask_crop", "no_K_crop", "no_uv21_crop", "no_xyz21"}
    assert {(c[0], c[1]) for c in FREIHAND_GEOMS} == {(1, 4), (17, 33), (32, 32), (40, 24)} and {c[2] for c in FREIHAND_GEOMS} == {0, 1, 21}
    assert {c[3] for c in FREIHAND_GEOMS} == {0, 50} and set(kc.FREIHAND_MAPS) == {"identity", "rotation", "flip", "half", "triple", "away", "subpixel"}
    assert {c[0] for c in ADAM_CASES} == {1, 3, 4, 5, 1023, 1024, 1027} and {c[1] for c in ADAM_CASES} == {0.0, 0.01} and {c[2] for c in ADAM_CASES} == {1.0, 0.5}
    tx = [c for c in TEXPCA_GEOMS if kc.texpca_contract_expect(*c[:3])]
    assert {c[0] for c in tx} == {1, 15, 16, 17, 33} and {c[1] for c in tx} == {1, 10, 31, 32} and {c[2] for c in tx} == {4, 8, 1020, 1024, 1028, 2336}
    assert {c[3] for c in tx} == {True, False} and {c[1] for c in TEXPCA_GEOMS} >= {0, 33} and {c[2] for c in TEXPCA_GEOMS} >= {0, 2, 6, 2334}
    ge = [c for c in GEOM_CASES if kc.geom_contract_expect(*c[:6])]
    assert {c[0] for c in ge} == {1, 2, 33} and {c[1] for c in ge} == {1, 21, 86} and {c[2] for c in ge} == {1, 85, 86, 256, 257, 778}
    assert {c[3] for c in ge} == {0, 1, 257, 1538} and {c[4] for c in ge} == {0, 10, 257} and {c[5] for c in ge} == {0, 48}
    assert {c[6] for c in ge} == {True, False} and {c[7] for c in ge} == {"random", "identical", "zero_edges"}
    jo = [c for c in JOINT_CASES if kc.joint_contract_expect(c[0], c[5], c[2], c[3])]
    assert {c[0] for c in jo} == {1, 12, 13, 64, 65} and {c[1] for c in jo} == {True, False} and {(c[2], c[3]) for c in jo} == {(True, True), (True, False), (False, True)}
    assert {c[4] for c in jo} == {"random", "identical", "zero_bones"} and {c[5] for c in JOINT_CASES} == {20, 21, 22}
    ph = [c for c in PHOTO_CASES if kc.photo_contract_expect(*c[:3])]
    assert {c[:3] for c in ph} == {(1, 1, 4), (1, 2, 2), (2, 16, 16), (3, 12, 20), (5, 23, 44)} and {c[3] for c in ph} == {"binary", "ints", "nan"}
    assert {c[:3] for c in PHOTO_CASES} >= {(1, 3, 3), (1, 2, 3)}
    assert {len(c[0]) for c in TOTAL_CASES} == {0, 1, 2, 3, 4, 5} and {n for c in TOTAL_CASES for n in c[0]} >= {0, 64, 65} and set(LIGHT_CASES) == {0, 1, 7, 300}
    ma = [c for c in MANO_CASES if c[1] > 0 and c[3] < 21]
    assert {c[2] for c in ma} == set(kc.MANO_POSE_FAMILIES) and {c[3] for c in ma} == {-1, 0, 9, 20} and {c[1] for c in ma} == {1, 3} and {c[0] for c in ma} == {"synth", "dense"}
    assert {c[1] for c in MANO_CASES} >= {0, -1} and {c[3] for c in MANO_CASES} >= {21}
    assert {c[:3] for c in LBS_CASES if c[3] > 0} == {(64, 1, 0), (257, 32, 32), (300, 7, 5)} and {c[3] for c in LBS_CASES} == {-1, 0, 1, 3}
