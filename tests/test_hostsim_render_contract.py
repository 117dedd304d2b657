"""The C ABI contract of the ten renderer entries on the hostsim emulator (tests/kernel_cases.py, "The renderer contract"): fixed case
lists on the kernels' own boundaries -- the forward's 8-pixel and the backward's 16-pixel tiles, the 128 merge slots of an image, the 512
vertex and 2 048 texel slots of a backward tile, the two list caps, the second forward form above 512 pixels -- with face ids bit for bit
the float32 oracle's, pixels and every gradient against a float64 reference per image, NaN prefill and guard bands (the workspace
included), and every refused call of every entry.  The GPU half runs the same lists, and a few larger shapes, in tests/test_gpu_render.py."""
import pytest
import torch

import kernel_cases as kc

# (scene, V/F source[/options], B, image_size, aa, mode): kernel_cases.render_contract_inputs
_MODES = ("vc", "shared", "uv", "point")
# hand: every size around the 8- and 16-pixel tile edges x every aa; the modes and B in {1, 3} go round
# (33, 3): the second pose -- in the first a sliver between vertices 741 and 742 wins samples, and plain float32 torch is 1.8e-3 of
# max|gverts| off the float64 answer there, 0.9 of the cap: kernel_cases.render_contract_admits, the test of that name below
HAND_CASES = [("hand", ("mano/mat" if (i % 5) == 0 else "mano") + ("/pose1" if (H, aa) == (33, 3) else ""), 3 if (i % 2) else 1, H, aa, _MODES[(i + i // 4) % 4])
              for i, (H, aa) in enumerate((H, aa) for H in (1, 7, 8, 9, 16, 17, 33) for aa in (1, 2, 3))]
RENDER_CASES = HAND_CASES + [
    ("sheets", "quads96", 1, 128, 1, "vc"),                      # 256 long tiles, 128 merge slots: the other 128 walk two passes of 128 faces
    ("offscreen", "mano", 6, 20, 2, "vc"), ("offscreen", "mano/mat", 6, 20, 3, "uv"),         # a ragged last tile (20 = 8 + 8 + 4)
    ("straddle", "tris", 2, 16, 2, "vc"), ("straddle", "tris/mat", 1, 9, 3, "point"), ("straddle", "tris", 1, 16, 1, "uv"),
    ("degenerate", "odd", 2, 16, 2, "vc"), ("degenerate", "odd", 2, 8, 2, "uv"), ("degenerate", "odd/mat", 2, 9, 1, "point"),
    ("degenerate", "one", 1, 8, 1, "shared"),                    # F = 1, V = 3
    ("confetti", "confetti196", 1, 16, 3, "vc"), ("confetti", "confetti196", 1, 16, 3, "uv"),  # 588 vertices in one backward tile
    ("hand", "mano/tex384", 1, 32, 3, "uv"),                     # more texels in a backward tile than its table holds
    ("batch", "ico", 300, 8, 1, "vc"),                           # the item code's image field, grid-stride loops over images
    ("dim", "mano/dim", 2, 16, 2, "vc"),                         # the second image at 1 / 100 of the first (the detection test)
]
RENDER_CASES += [("dense", "skin/mat" if aa == 2 else "skin", 1, 16, aa, m) for aa in (1, 2, 3) for m in ("shared", "uv")]      # CAP = 256, parts of 512
RENDER_CASES += [("second_form", "one/small", 1, 513, aa, m) for aa, m in ((1, "vc"), (2, "uv"), (3, "point"), (1, "uv"), (2, "shared"), (3, "uv"))]
ENTRIES = kc.RENDER_CONTRACT_ENTRIES

EXPECT_LAUNCHED = {"render_vertex_kernel", "render_vertex_bwd_kernel"}
EXPECT_LAUNCHED |= {f"render_bin_kernel<{aa},8>" for aa in (1, 2, 3)}                             # (<AA, 16>: HIFIHR_RENDER_TILE=16 builds' A/B only)
EXPECT_LAUNCHED |= {f"render_fwd3_kernel<{aa},{uv},{cap}>" for aa in (1, 2, 3) for uv in ("true", "false") for cap in ("kF3Cap", "256")}
EXPECT_LAUNCHED |= {f"render_fwd2_kernel<{aa},8,{uv}>" for aa in (1, 2, 3) for uv in ("true", "false")}
EXPECT_LAUNCHED |= {f"render_bwd_kernel<{aa},{uv}>" for aa in (1, 2, 3) for uv in ("true", "false")}

_ids = lambda g: "-".join(str(v) for v in g) if isinstance(g, tuple) else str(g)
_DONE = {}


def render_runners(device):
    """family -> (lib, case) -> accepted?  (the GPU half walks the same lists through it)"""
    return {"render": lambda lib, g: kc.render_contract_case(lib, device, g), "refuse": lambda lib, e: kc.render_refusal_case(lib, device, e)}


LISTS = {"render": RENDER_CASES, "refuse": list(ENTRIES)}
_RUNNERS = render_runners("cpu")


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.fixture(scope="module")
def tally():
    yield None
    kc.layer_contract_report("the renderer entries on the emulator", ENTRIES)


def _run(lib, family, case):
    """One case, once per session."""
    key = (family, case)
    if key not in _DONE:
        _DONE[key] = _RUNNERS[family](lib, case)
    return _DONE[key]


@pytest.mark.parametrize("case", RENDER_CASES, ids=_ids)
def test_render_on_every_scene_size_and_mode(hostsim_lib, tally, case):
    assert _run(hostsim_lib, "render", case)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_refuses_and_touches_nothing(hostsim_lib, tally, entry):
    assert _run(hostsim_lib, "refuse", entry) == (entry not in ("renderer_destroy", "render_workspace_bytes", "render_uv_scratch_bytes"))


def test_the_scenes_are_what_they_claim():
    """The properties the lists rely on, from the float32 oracle's face ids alone."""
    import numpy as np
    for case in RENDER_CASES:
        inp = kc.render_contract_inputs(case)
        p2f, scene = inp["p2f"], case[0]
        if scene == "sheets":
            won = set(np.unique(p2f).tolist())
            assert (p2f >= 0).all() and not won & {22, 23, 102, 103} and won & {20, 21} and won & {100, 101}, "coplanar copies: the lower index wins"
            assert len(won) >= 6                                         # the planes cross: depth competition everywhere
        if scene == "offscreen":
            hit = p2f >= 0
            assert hit[0][:, 0].any() and hit[1][:, -1].any() and hit[2][0].any() and hit[3][-1].any(), "the hand crosses each border"
            assert not hit[4].any() and hit[5].any() and not hit[:4].all((1, 2)).any()
        if scene == "straddle":
            assert (inp["verts"][..., 2] < 0).any() and (inp["verts"][..., 2] != 0).all()
            won = [set(np.unique(p2f[b]).tolist()) for b in range(inp["B"])]
            assert all({1, 2} <= w and not w & {0, 3} for w in won), "two vertices behind the camera: covers samples; one: none (pz < 0)"
            assert float(kc.render_contract_ref_once(case)[0]["gverts"][:, 3:6].abs().max()) > 0
        if scene == "degenerate" and case[1].startswith("odd"):
            won = set(np.unique(p2f).tolist())
            assert 0 in won and not won & {1, 3, 4} and 9 not in inp["faces"]
        if scene == "confetti":
            assert inp["V"] > 512 and len(np.unique(p2f[p2f >= 0])) == inp["F"], "every triangle covers a sample of the one backward tile"
        if scene in ("hand", "dense", "batch", "second_form", "dim"):
            assert (p2f >= 0).any()


def test_float32_itself_leaves_half_of_every_cap_on_every_case():
    """kernel_cases.render_contract_admits: on no case of the list does the reference's own float32 run use up more than half of a cap
    (the first pose of the 33-pixel, aa = 3 hand did: 1.8e-3 of max|gverts| against the cap of 2e-3)."""
    out = {case: kc.render_contract_admits(case) for case in RENDER_CASES}
    assert not any(out.values()), {c: v for c, v in out.items() if v}
    first = ("hand", "mano/mat", 1, 33, 3, "shared")
    assert first not in RENDER_CASES and [r[1] for r in kc.render_contract_admits(first)] == ["render_gv"]


def test_detection_the_comparator_notices_one_missing_contribution():
    """No kernel involved: the float64 reference with ONE contribution removed -- a sample of a pixel's aa x aa block (and so of every gradient
    sum it feeds), a face of a vertex normal, a bilinear tap of the texture gradient -- must fail the comparator for the quantities it feeds,
    on every case of the list."""
    from oracle import render_oracle as ro
    missed, n_moved = [], 0
    for case in RENDER_CASES:
        inp = kc.render_contract_inputs(case)
        ref, cond = kc.render_contract_ref_once(case)
        pick = kc.render_drop_choice(inp, ref)
        if pick is None:
            continue
        b, y, x, f = pick
        K = cond[b][3]
        bad = kc.render_contract_ref(inp, drop=("sample", b, y, x))
        assert not torch.equal(bad["alpha"][b], ref["alpha"][b])          # (alpha is compared exactly)
        lit = float((bad["rgb"][b] - ref["rgb"][b]).abs().max()) > 0      # (an unlit sample without ambient term is black: nothing to miss)
        if lit and kc.render_passes("render_rgb", bad["rgb"][b], ref["rgb"][b], inp["aa"] ** 2, K):
            missed.append((case, "sample", "rgb"))
        for name, kind, li in kc.render_quantities(inp):
            changed = float((bad[name][b] - ref[name][b]).abs().max()) > 0
            if changed and kc.render_passes(kind, bad[name][b], ref[name][b], cond[b][li], K):
                missed.append((case, "sample", name))
        if inp["uv"] is not None:
            badt = kc.render_contract_ref(inp, drop=("tap", b, y, x))
            if kc.render_passes("render_gmap", badt["gmaps"][b], ref["gmaps"][b], cond[b][2], K):
                missed.append((case, "tap", "gmaps"))
        fl = torch.as_tensor(inp["faces"]).long()
        n_all, n_cut = (ro.vertex_normals(inp["verts"][b:b + 1].double(), fl, sk)[0, fl[f, 0]] for sk in (None, (f, 0)))
        if float(n_cut.norm()) < 0.5 or float((n_all - n_cut).abs().max()) < 1e-3:      # the vertex's only face, or all its faces coplanar: no direction changes
            continue
        n_moved += 1
        badn = kc.render_contract_ref(inp, drop=("normal", f, 0))
        for name, kind, L in [("rgb", "render_rgb", inp["aa"] ** 2), ("gverts", "render_gv", cond[b][0])]:
            changed = float((badn[name][b] - ref[name][b]).abs().max()) > 0
            if changed and kc.render_passes(kind, badn[name][b], ref[name][b], L, K):
                missed.append((case, "normal", name))
    assert n_moved >= 30
    assert not missed, f"the comparator accepts a reference with one contribution removed: {missed}"


def test_detection_a_dim_image_no_longer_hides_behind_a_bright_one():
    """The weakness of the criterion this contract replaces: two images of one hand, the second lit at 1 / 100 of the first, under the loss
    sum(rgb^2) / 2 (its gradients are 1e-4 of the first image's).  The second image's gradients DOUBLED pass render_case's one-maximum-over-the-batch test and fail the per-image bounds."""
    case = next(c for c in RENDER_CASES if c[0] == "dim")
    inp = kc.render_contract_inputs(case)
    ref, cond = kc.render_contract_ref_once(case)
    for name, kind, li in kc.render_quantities(inp)[:2]:                 # gverts, gvcolors (the light colour's gradient does not scale with the light)
        bad = ref[name].clone()
        bad[1] *= 2
        assert float(ref[name][1].abs().max()) > 0
        assert kc.render_legacy_passes(bad, ref[name]), name
        assert not kc.render_passes(kind, bad[1], ref[name][1], cond[1][li], cond[1][3]), name
        assert kc.render_passes(kind, bad[0], ref[name][0], cond[0][li], cond[0][3]), name


def test_no_bound_is_looser_than_the_case_it_replaces():
    """min(c (sqrt(L) + K), cap) max|ref of one image| never exceeds what render_case / render_uv_case allow for the same quantity: 2e-5
    absolute on pixels of the order of 1, 2e-3 (3e-3 for the texture) of the batch's largest gradient."""
    legacy = {"render_rgb": 2e-5, "render_gv": 2e-3, "render_gc": 2e-3, "render_gmap": 3e-3, "render_glc": 2e-3, "render_gld": 2e-3}
    assert set(kc.RENDER_CONTRACT_KINDS) == set(legacy) and set(legacy) <= set(kc.LAYER_CONTRACT_C)
    for kind, tol in legacy.items():
        c, cap = kc.LAYER_CONTRACT_C[kind]
        assert 0 < c <= cap == tol, kind
        for scale in (1e-3, 1.0, 50.0):
            ref = torch.full((3,), scale, dtype=torch.float64)
            for L in (1, 9, 10 ** 12):
                for K in (0.0, 4.0, 1e9):
                    assert kc.render_bound(kind, ref, L, K) <= tol * scale, (kind, scale, L, K)
        ref = torch.tensor([0.0, 1.0, -3.0], dtype=torch.float64)
        assert not kc.render_passes(kind, ref + 1.01 * tol * 3.0, ref, 10 ** 12, 1e9)


def test_the_lists_reach_every_kernel_every_entry_and_both_answers(hostsim_lib):
    """A list edit that stops reaching a kernel spelling, a path counter, an entry's accepted or refused side, or a size class fails here."""
    lib = hostsim_lib
    for family, cases in LISTS.items():                                      # (whatever a -k selection left out runs now)
        for c in cases:
            _run(lib, family, c)
    assert EXPECT_LAUNCHED <= kc.RENDER_LAUNCHED, f"no case reaches {sorted(EXPECT_LAUNCHED - kc.RENDER_LAUNCHED)}"
    assert all(v > 0 for v in kc.RENDER_COUNTS.values()), kc.RENDER_COUNTS
    for e in ENTRIES:
        row = kc.LAYER_CONTRACT_LOG.get(e, [0, 0, 0.0])
        assert row[0] > 0 and (row[1] > 0 or e in ("renderer_destroy", "render_workspace_bytes", "render_uv_scratch_bytes")), f"{e}: accepted {row[0]}, refused {row[1]} calls"
    # the classes the lists exist for
    hand = [c for c in RENDER_CASES if c[0] == "hand"]
    assert {(c[3], c[4]) for c in hand} >= {(H, aa) for H in (1, 7, 8, 9, 16, 17, 33) for aa in (1, 2, 3)}
    assert {c[0] for c in RENDER_CASES} >= {"hand", "sheets", "offscreen", "straddle", "degenerate", "confetti", "dense", "batch", "second_form", "dim"}
    assert {c[5] for c in RENDER_CASES} == set(_MODES) and {c[5] for c in hand} == set(_MODES)
    assert {c[5] for c in RENDER_CASES if "mat" in c[1].split("/")} == set(_MODES), "non-default materials in every mode"
    assert {c[2] for c in RENDER_CASES} >= {1, 3, 300} and {c[2] for c in hand} >= {1, 3}
    assert {(c[4], c[5] == "uv") for c in RENDER_CASES if c[0] == "dense"} == {(aa, u) for aa in (1, 2, 3) for u in (True, False)}
    assert {(c[4], c[5] == "uv") for c in RENDER_CASES if c[3] > 512} == {(aa, u) for aa in (1, 2, 3) for u in (True, False)}
    assert any(c[0] == "degenerate" and c[1] == "one" for c in RENDER_CASES) and any("tex384" in c[1] for c in RENDER_CASES)
    assert ("sheets", "quads96", 1, 128, 1, "vc") in RENDER_CASES and ("batch", "ico", 300, 8, 1, "vc") in RENDER_CASES
