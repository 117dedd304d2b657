"""What LossFunction hands to the kernels, host only: every `ops` entry of the loss terms is replaced by a stub that records its arguments
and returns a recognisable CPU vector, so no kernel runs and no library is needed.  Per case: the sequence of entries, the weight tuples,
the identity of the tensor arguments, the keys of loss_dic in order with their values, and the parts registered for total()'s one launch.
Every expectation is written out here; none is recorded from the code under test."""
import pytest
import torch

from hifihr_amd import losses, ops, options
from hifihr_amd.losses import LossFunction

B, V = 2, 4
GEOM = ("joint_3d", "vert_3d", "edge_length", "mshape", "mpose")
JOINT = ("joint_2d", "bone_direc", "bone_direc_3d")
OPEN2D = ("open_2dj", "open_bone_direc", "open_2dj_de")
SOFT = ("sil_soft", "iou_soft")
MESH = ("triangle", "normal_consistency")
ALL_TERMS = GEOM + JOINT + OPEN2D + ("mscale", "scale", "texture_self", "mrgb_self", "ssim_tex_self", "texture", "mrgb", "ssim_tex", "sil",
                                      "perceptual", "lpips", "iou") + SOFT + MESH + ("chamfer", "point_mesh", "depth", "mtex")
# first element of each stub's result, and its length (0 = a 0-d tensor)
BASE = dict(geom_losses=(100.0, 5), joint_terms=(200.0, 3), open2d_terms=(300.0, 3), photo_losses=(400.0, 4), soft_sil_losses=(600.0, 2),
            mesh_regularizers=(700.0, 2), chamfer_distance=(800.0, 0), point_mesh_distance=(900.0, 0), depth_loss=(1000.0, 0))
# distinct weights inside every fused group (the defaults give joint_3d / vert_3d and the two bone terms the same one)
ARGS = dict(lambda_vert_3d=150.0, lambda_bone_direc=0.2, lambda_bone_direc_3d=0.3)
W_GEOM = (100.0, 150.0, 0.1, 1e-5, 1e-4)
W_JOINT = (1e-5, 0.2, 0.3)
W_OPEN2D = (1e-3, 0.2, 1e-4)
W_SOFT = (0.005, 1e-3)
W_MESH = (0.1, 0.01)
W_PHOTO = (0.003, 1e-3, 0.005)


class Recorder:
    def __init__(self, monkeypatch):
        self.calls = []
        self.photo_images = None
        for name, (base, n) in BASE.items():
            monkeypatch.setattr(ops, name, self._vector(name, base, n))
        monkeypatch.setattr(ops, "photo_losses", self._photo)
        monkeypatch.setattr(ops, "ssim_loss", self._ssim)
        monkeypatch.setattr(ops, "mesh_topology_of", self._topology)

    def _vector(self, name, base, n):
        def stub(*a):
            self.calls.append((name, a))
            return torch.tensor(base) if n == 0 else base + torch.arange(n, dtype=torch.float32)
        return stub

    def _photo(self, *a):
        self.calls.append(("photo_losses", a))
        self.photo_images = (torch.full((B, 3, 8, 8), 0.25), torch.full((B, 3, 8, 8), 0.75))
        return (400.0 + torch.arange(4, dtype=torch.float32), *self.photo_images)

    def _ssim(self, *a):
        self.calls.append(("ssim_loss", a))
        return torch.tensor(500.0 + sum(1 for k, _ in self.calls if k == "ssim_loss"))       # 501, then 502

    def _topology(self, *a):
        self.calls.append(("mesh_topology_of", a))
        return ("topology of", a[0])

    def perceptual(self, *a):
        self.calls.append(("perceptual", a))
        return torch.tensor(1100.0)

    def lpips(self, *a, **kw):
        self.calls.append(("lpips", a + (kw,)))
        return torch.tensor([1200.0, 1202.0])

    def entries(self):
        return [k for k, _ in self.calls]

    def only(self, name):
        hits = [a for k, a in self.calls if k == name]
        assert len(hits) == 1, (name, self.entries())
        return hits[0]


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


def make_batch():
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    ex = dict(joints=r(B, 21, 3), verts=r(B, V, 3), j2d_gt=r(B, 21, 2), imgs=r(B, 3, 8, 8), segms_gt=(r(B, 8, 8) > 0.5).long(), scales=r(B),
              open_2dj=r(B, 21, 2), open_2dj_con=r(B, 21), depths=r(B, 8, 8))
    out = dict(joints=r(B, 21, 3), mano_verts=r(B, V, 3), shape_params=r(B, 10), pose_params=r(B, 48), j2d=r(B, 21, 2),
               mano_faces=torch.tensor([[[0, 1, 2], [0, 2, 3]]] * B), _faces_i32=torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32),
               _mesh_topo=("the model's topology",), re_img=r(B, 3, 8, 8), re_sil=(r(B, 1, 8, 8) > 0.5).float() * 255, _rgba=r(B, 4, 8, 8),
               maskRGBs=r(B, 3, 8, 8), re_sil_soft=r(B, 1, 8, 8), re_depth=r(B, 1, 8, 8),
               _re_depth_hits=torch.ones(B, 8, 8, dtype=torch.int32), texture_params=r(B, 10))
    return ex, out


def without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def run(rec, ex, out, names, dat_name="FreiHand", **overrides):
    args = options.make_args(**{**ARGS, **overrides})
    lf = LossFunction(perceptual=rec.perceptual, lpips=rec.lpips)
    dic = lf(ex, out, list(names), dat_name, args)
    return lf, dic, [(n, list(k)) for _, n, k in lf._total_parts]


def value(dic, name):
    assert dic[name].dim() == 0, name
    return float(dic[name])


def bone_length(out):
    return torch.sqrt(torch.sum((out["joints"][:, 9] - out["joints"][:, 10]) ** 2, 1))


def composite(ex, out):
    seg = ex["segms_gt"].unsqueeze(1)
    return out["re_img"] * seg + ex["imgs"] * (1 - seg)


@pytest.mark.parametrize("with_sil", [True, False])
def test_default_list_on_a_rendering_model(rec, with_sil):
    ex, out = make_batch()
    names = options.make_args().losses
    assert names == ["joint_3d", "vert_3d", "mpose", "mshape", "edge_length", "sil", "texture", "mrgb", "ssim_tex"]
    names = [k for k in names if with_sil or k != "sil"]
    lf, dic, parts = run(rec, ex, out, names)
    assert rec.entries() == ["geom_losses", "photo_losses", "ssim_loss"]
    a = rec.only("geom_losses")
    assert a[0] is out["joints"] and a[1] is ex["joints"] and a[2] is out["mano_verts"] and a[3] is ex["verts"]
    assert a[4] is out["shape_params"] and a[5] is out["pose_params"] and a[6] is out["_faces_i32"] and a[7] is False
    assert tuple(a[8]) == W_GEOM
    a = rec.only("photo_losses")
    assert a[0] is out["_rgba"] and a[1] is ex["imgs"] and a[2] is ex["segms_gt"]
    assert tuple(a[3:]) == W_PHOTO                                  # `sil` keeps its weight when it is not requested
    a = rec.only("ssim_loss")
    assert a[0] is rec.photo_images[0] and a[1] is rec.photo_images[1] and a[2] == 0.001
    assert list(dic) == list(GEOM) + ["texture", "mrgb", "ssim_tex"] + (["sil"] if with_sil else [])
    assert [value(dic, k) for k in GEOM] == [100.0, 101.0, 102.0, 103.0, 104.0]
    assert (value(dic, "texture"), value(dic, "mrgb"), value(dic, "ssim_tex")) == (400.0, 401.0, 501.0)
    assert parts == [(5, list(GEOM)), (3, ["texture", "mrgb", "sil"]) if with_sil else (2, ["texture", "mrgb"]), (1, ["ssim_tex"])]
    want = 510.0 + 400.0 + 401.0 + 501.0 + (402.0 if with_sil else 0.0)
    assert value(dic, "sil") == 402.0 if with_sil else "sil" not in dic
    assert float(lf.total(dic, names)) == want


def test_outputs_without_rgba_get_the_binarised_silhouette_as_alpha(rec):
    ex, out = make_batch()
    _, dic, parts = run(rec, ex, without(out, "_rgba"), ["texture"])
    a = rec.only("photo_losses")
    assert torch.equal(a[0], torch.cat([out["re_img"], (out["re_sil"] > 0).float()], 1)) and a[0].dtype == out["re_img"].dtype
    assert list(dic) == ["texture", "mrgb", "ssim_tex"] and parts == [(2, ["texture", "mrgb"]), (1, ["ssim_tex"])]


def test_a_rendering_model_under_a_keypoint_list_still_runs_the_photo_block(rec):
    ex, out = make_batch()
    lf, dic, parts = run(rec, ex, out, ["joint_3d"])
    assert rec.entries() == ["geom_losses", "photo_losses", "ssim_loss"]
    assert list(dic) == ["joint_3d", "texture", "mrgb", "ssim_tex"]
    assert parts == [(5, ["joint_3d"]), (2, ["texture", "mrgb"]), (1, ["ssim_tex"])]
    assert float(lf.total(dic, ["joint_3d"])) == 100.0


def subsets_one_and_all(names):
    return [(k,) for k in names] + [tuple(names)]


def masked(weights, names, asked):
    return tuple(w if k in asked else 0.0 for k, w in zip(names, weights))


@pytest.mark.parametrize("asked", subsets_one_and_all(GEOM))
@pytest.mark.parametrize("faces_key", ["_faces_i32", "mano_faces"])
def test_geometry_group(rec, asked, faces_key):
    ex, out = make_batch()
    out = without(out, "re_img", "_faces_i32" if faces_key == "mano_faces" else "")
    _, dic, parts = run(rec, ex, out, asked, base_loss_fn="L2" if len(asked) > 1 else "L1")
    assert rec.entries() == ["geom_losses"]
    a = rec.only("geom_losses")
    assert a[0] is out["joints"] and a[1] is ex["joints"] and a[2] is out["mano_verts"] and a[3] is ex["verts"]
    assert a[4] is out["shape_params"] and a[5] is out["pose_params"] and a[7] is (len(asked) > 1)
    w = tuple(a[8])
    assert w == masked(W_GEOM, GEOM, asked) and all(type(x) is float for x in w if x == 0.0)
    if "edge_length" not in asked:                # edge_length always runs on the MANO faces; no other term reads them
        assert a[6] is None
    elif faces_key == "_faces_i32":
        assert a[6] is out["_faces_i32"]
    else:
        assert a[6].dtype == torch.int32 and a[6].is_contiguous() and torch.equal(a[6], out["mano_faces"][0].int())
    assert list(dic) == list(asked) and [value(dic, k) for k in asked] == [100.0 + GEOM.index(k) for k in asked]
    assert parts == [(5, list(asked))]


def test_geometry_without_ground_truth_gets_the_detached_outputs(rec):
    """examples without 'joints' / 'verts' (a dataset that has none): the regularisers still run, joint_3d / vert_3d are not requested and
    so not reported, and their weight-0 slots read the detached outputs in place of the absent ground truth."""
    ex, out = make_batch()
    out["joints"].requires_grad_(True)
    out["mano_verts"].requires_grad_(True)
    _, dic, parts = run(rec, without(ex, "joints", "verts"), without(out, "re_img"), ["mpose", "mshape"])
    a = rec.only("geom_losses")
    assert a[0] is out["joints"] and a[2] is out["mano_verts"]
    assert a[1].data_ptr() == out["joints"].data_ptr() and not a[1].requires_grad
    assert a[3].data_ptr() == out["mano_verts"].data_ptr() and not a[3].requires_grad
    assert tuple(a[8]) == (0.0, 0.0, 0.0, 1e-5, 1e-4) and a[6] is None
    assert list(dic) == ["mshape", "mpose"] and parts == [(5, ["mshape", "mpose"])]


@pytest.mark.parametrize("asked", [("joint_2d",), ("bone_direc",), ("bone_direc_3d",), ("joint_2d", "bone_direc"), ("joint_2d", "bone_direc_3d"),
                                   ("bone_direc", "bone_direc_3d"), JOINT])
def test_joint_terms_group(rec, asked):
    ex, out = make_batch()
    lf, dic, parts = run(rec, ex, without(out, "re_img"), asked)
    assert rec.entries() == ["joint_terms"]
    a = rec.only("joint_terms")
    if "joint_2d" in asked or "bone_direc" in asked:
        assert a[0] is out["j2d"] and a[1] is ex["j2d_gt"]
    else:
        assert a[0] is None and a[1] is None
    if "bone_direc_3d" in asked:
        assert a[2] is out["joints"] and a[3] is ex["joints"]
    else:
        assert a[2] is None and a[3] is None
    assert a[4] is False and tuple(a[5]) == masked(W_JOINT, JOINT, asked)
    assert list(dic) == list(asked) and [value(dic, k) for k in asked] == [200.0 + JOINT.index(k) for k in asked]
    assert parts == []                            # the joint terms stay outside total()'s one launch
    assert float(lf.total(dic, list(asked))) == sum(200.0 + JOINT.index(k) for k in asked)


@pytest.mark.parametrize("asked", subsets_one_and_all(OPEN2D))
def test_open2d_group(rec, asked):
    ex, out = make_batch()
    _, dic, parts = run(rec, ex, without(out, "re_img"), asked)
    assert rec.entries() == ["open2d_terms"]
    a = rec.only("open2d_terms")
    assert a[0] is out["j2d"] and a[1] is ex["open_2dj"] and a[2] is ex["open_2dj_con"] and tuple(a[3]) == masked(W_OPEN2D, OPEN2D, asked)
    assert list(dic) == list(asked) and [value(dic, k) for k in asked] == [300.0 + OPEN2D.index(k) for k in asked]
    assert parts == [(3, list(asked))]


@pytest.mark.parametrize("asked", subsets_one_and_all(SOFT))
def test_soft_silhouette_group(rec, asked):
    ex, out = make_batch()
    _, dic, parts = run(rec, ex, without(out, "re_img"), asked)
    assert rec.entries() == ["soft_sil_losses"]
    a = rec.only("soft_sil_losses")
    assert a[0] is out["re_sil_soft"] and a[1] is ex["segms_gt"] and tuple(a[2:]) == masked(W_SOFT, SOFT, asked)
    assert list(dic) == list(asked) and [value(dic, k) for k in asked] == [600.0 + SOFT.index(k) for k in asked]
    assert parts == [(2, list(asked))]


@pytest.mark.parametrize("asked", subsets_one_and_all(MESH))
def test_mesh_regulariser_group(rec, asked):
    ex, out = make_batch()
    _, dic, parts = run(rec, ex, without(out, "re_img"), asked)
    assert rec.entries() == ["mesh_regularizers"]
    a = rec.only("mesh_regularizers")
    assert a[0] is out["_mesh_topo"] and a[1] is out["mano_verts"] and tuple(a[2:]) == masked(W_MESH, MESH, asked)
    assert list(dic) == list(asked) and [value(dic, k) for k in asked] == [700.0 + MESH.index(k) for k in asked]
    assert parts == [(2, list(asked))]


def test_texture_con_puts_the_self_terms_before_the_photo_block(rec):
    ex, out = make_batch()
    ex["texture_con"] = torch.tensor([0.5, 0.25])
    names = options.make_args().losses
    _, dic, parts = run(rec, ex, out, names)
    assert rec.entries() == ["geom_losses", "ssim_loss", "photo_losses", "ssim_loss"]
    first, second = [a for k, a in rec.calls if k == "ssim_loss"]
    assert first[0] is out["re_img"] and first[1] is out["maskRGBs"] and first[2] == 0.001
    assert second[0] is rec.photo_images[0] and second[1] is rec.photo_images[1] and second[2] == 0.001
    assert list(dic) == list(GEOM) + ["texture_self", "mrgb_self", "ssim_tex_self", "texture", "mrgb", "ssim_tex", "sil"]
    c2 = ex["texture_con"] ** 2
    per = torch.abs(out["re_img"] - out["maskRGBs"]).reshape(B, -1).sum(1)
    assert torch.equal(dic["texture_self"], 0.003 * (torch.sum(per * c2) / (torch.sum(c2) * 192)))
    dm = torch.abs(out["re_img"].reshape(B, -1).mean(1) - out["maskRGBs"].reshape(B, -1).mean(1))
    assert torch.equal(dic["mrgb_self"], 1e-3 * (torch.sum(dm * c2) / torch.sum(c2)))
    assert (value(dic, "ssim_tex_self"), value(dic, "ssim_tex")) == (501.0, 502.0)
    assert parts == [(5, list(GEOM)), (3, ["texture", "mrgb", "sil"]), (1, ["ssim_tex"])]     # the self terms are outside total()'s launch


def test_scale_runs_for_freihand_and_rhd_only(rec):
    ex, out = make_batch()
    out = without(out, "re_img")
    for dat_name in ("FreiHand", "RHD"):
        _, dic, parts = run(rec, ex, out, ["scale", "mscale"], dat_name)
        assert list(dic) == ["mscale", "scale"] and parts == []
        bl = bone_length(out)
        assert torch.equal(dic["mscale"], 0.1 * torch.nn.functional.l1_loss(bl, torch.ones_like(bl) * 0.0282))
        assert torch.equal(dic["scale"], 100.0 * torch.nn.functional.mse_loss(bl, ex["scales"]))
    _, dic, _ = run(rec, ex, out, ["scale", "mscale"], "HO3D")
    assert list(dic) == ["mscale"] and rec.calls == []


def test_mtex_runs_with_texture_params_only(rec):
    ex, out = make_batch()
    out = without(out, "re_img")
    _, dic, parts = run(rec, ex, out, ["mtex"])
    tex = out["texture_params"]
    assert list(dic) == ["mtex"] and parts == [] and torch.equal(dic["mtex"], 1e-5 * torch.nn.functional.mse_loss(tex, torch.zeros_like(tex)))
    for absent in (without(out, "texture_params"), dict(out, texture_params=None)):
        assert run(rec, ex, absent, ["mtex"])[1] == {}
    assert rec.calls == []


def test_perceptual_lpips_and_iou_are_single_torch_terms(rec):
    ex, out = make_batch()
    _, dic, parts = run(rec, ex, out, ["iou", "lpips", "perceptual"])
    assert rec.entries() == ["photo_losses", "ssim_loss", "perceptual", "lpips"]
    a = rec.only("perceptual")
    assert torch.equal(a[0], composite(ex, out)) and a[1] is ex["imgs"]
    a = rec.only("lpips")
    assert torch.equal(a[0], composite(ex, out)) and a[1] is ex["imgs"] and a[2] == {"normalize": True}
    assert list(dic) == ["texture", "mrgb", "ssim_tex", "perceptual", "lpips", "iou"]
    assert torch.equal(dic["perceptual"], 1e-5 * torch.tensor(1100.0)) and torch.equal(dic["lpips"], 0.01 * torch.tensor(1201.0))
    assert torch.equal(dic["iou"], 1e-3 * losses.iou(out["re_sil"], ex["segms_gt"].unsqueeze(1).float()))
    assert parts == [(2, ["texture", "mrgb"]), (1, ["ssim_tex"])]


FACES_2D = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
MESH_VARIANTS = ["caller_2d", "caller_3d", "nimble", "nimble_no_skin_faces", "mano_model", "mano_faces_i32", "mano_faces"]


def mesh_variant(out, variant):
    """-> (outputs, hand_model).  caller_*: outputs['verts'] + ['faces']; nimble*: the dense skin outputs['verts'] with its root and (or
    not) its faces; mano_*: neither -- with the model's own tables, with the int32 faces only, with the reference's 'mano_faces' only."""
    out = without(out, "re_img")
    skin = torch.rand(B, V, 3, generator=torch.Generator().manual_seed(1))
    if variant == "caller_2d":
        return dict(out, verts=skin, faces=FACES_2D), "mano"
    if variant == "caller_3d":
        return dict(out, verts=skin, faces=FACES_2D.unsqueeze(0).repeat(B, 1, 1)), "mano"
    if variant.startswith("nimble"):
        out = dict(out, verts=skin, _pred_root=torch.full((B, 1, 3), 0.5))
        return (out if variant == "nimble_no_skin_faces" else dict(out, _skin_faces_i32=FACES_2D.clone())), "nimble"
    return without(out, *{"mano_model": (), "mano_faces_i32": ("_mesh_topo",), "mano_faces": ("_mesh_topo", "_faces_i32")}[variant]), "mano"


def is_first_of_batch(t, faces3):
    return t.data_ptr() == faces3.data_ptr() and torch.equal(t, faces3[0])


@pytest.mark.parametrize("variant", MESH_VARIANTS)
def test_triangle_takes_the_callers_mesh_else_mano(rec, variant):
    ex, full = make_batch()
    out, hand_model = mesh_variant(full, variant)
    run(rec, ex, out, ["triangle"], hand_model=hand_model)
    a = rec.only("mesh_regularizers")
    if variant.startswith("caller"):
        t = rec.only("mesh_topology_of")
        assert (t[0] is out["faces"]) if variant == "caller_2d" else is_first_of_batch(t[0], out["faces"])
        assert t[1] == V and a[0] == ("topology of", t[0]) and a[1] is out["verts"]
    elif variant in ("nimble", "nimble_no_skin_faces", "mano_model"):       # the skin has no 'faces': the MANO mesh is regularised
        assert rec.entries() == ["mesh_regularizers"] and a[0] is full["_mesh_topo"] and a[1] is out["mano_verts"]
    else:
        t = rec.only("mesh_topology_of")
        if variant == "mano_faces_i32":
            assert t[0] is out["_faces_i32"]
        else:
            assert t[0].dtype == torch.int32 and t[0].is_contiguous() and torch.equal(t[0], out["mano_faces"][0].int())
        assert t[1] == V and a[0] == ("topology of", t[0]) and a[1] is out["mano_verts"]
    assert rec.entries()[-1] == "mesh_regularizers" and tuple(a[2:]) == (0.1, 0.0)


@pytest.mark.parametrize("target_key", ["chamfer_points", "verts"])
@pytest.mark.parametrize("variant", MESH_VARIANTS + ["own_points"])
def test_chamfer_takes_its_own_points_else_the_skin_else_mano(rec, variant, target_key):
    ex, full = make_batch()
    if target_key == "chamfer_points":
        ex["chamfer_points"] = torch.rand(B, 7, 3)
    out, hand_model = mesh_variant(full, "caller_2d" if variant == "own_points" else variant)
    if variant == "own_points":
        out["chamfer_points"] = torch.rand(B, 5, 3)
    _, dic, parts = run(rec, ex, out, ["chamfer"], hand_model=hand_model, lambda_chamfer=2.0)
    assert rec.entries() == ["chamfer_distance"]
    a = rec.only("chamfer_distance")
    if variant == "own_points":
        assert a[0] is out["chamfer_points"]
    elif variant.startswith("nimble"):            # the dense skin, root-relative like mano_verts; it needs no faces
        assert torch.equal(a[0], out["verts"] - out["_pred_root"])
    else:                                         # (the caller's verts / faces are the mesh regularisers' and point_mesh's, not chamfer's)
        assert a[0] is out["mano_verts"]
    assert a[1] is ex[target_key] and tuple(a[2:]) == (2.0, 2.0)
    assert list(dic) == ["chamfer"] and value(dic, "chamfer") == 800.0 and parts == [(1, ["chamfer"])]


@pytest.mark.parametrize("target_key", ["chamfer_points", "verts"])
@pytest.mark.parametrize("variant", MESH_VARIANTS)
def test_point_mesh_takes_the_callers_mesh_else_the_skin_else_mano(rec, variant, target_key):
    ex, full = make_batch()
    if target_key == "chamfer_points":
        ex["chamfer_points"] = torch.rand(B, 7, 3)
    out, hand_model = mesh_variant(full, variant)
    _, dic, parts = run(rec, ex, out, ["point_mesh"], hand_model=hand_model, lambda_point_mesh_faces=0.5)
    assert rec.entries() == ["point_mesh_distance"]
    a = rec.only("point_mesh_distance")
    assert a[0] is ex[target_key]
    if variant.startswith("caller"):
        assert a[1] is out["verts"]
        assert (a[2] is out["faces"]) if variant == "caller_2d" else is_first_of_batch(a[2], out["faces"])
    elif variant == "nimble":
        assert torch.equal(a[1], out["verts"] - out["_pred_root"]) and a[2] is out["_skin_faces_i32"]
    elif variant == "mano_faces":
        assert a[1] is out["mano_verts"]
        assert a[2].dtype == torch.int32 and a[2].is_contiguous() and torch.equal(a[2], out["mano_faces"][0].int())
    else:                                         # a skin without its faces falls through to the MANO mesh
        assert a[1] is out["mano_verts"] and a[2] is out["_faces_i32"]
    assert tuple(a[3:]) == (1.0, 0.5)
    assert list(dic) == ["point_mesh"] and value(dic, "point_mesh") == 900.0 and parts == [(1, ["point_mesh"])]


@pytest.mark.parametrize("with_mask", [True, False])
def test_depth_term(rec, with_mask):
    ex, out = make_batch()
    ex = ex if with_mask else without(ex, "segms_gt")
    _, dic, parts = run(rec, ex, without(out, "re_img"), ["depth"], depth_trunc=0.03)
    a = rec.only("depth_loss")
    assert a[0] is out["re_depth"] and a[1] is out["_re_depth_hits"] and a[2] is ex["depths"]
    assert (a[3] is ex["segms_gt"]) if with_mask else a[3] is None
    assert tuple(a[4:]) == (1.0, 0.03)
    assert list(dic) == ["depth"] and value(dic, "depth") == 1000.0 and parts == [(1, ["depth"])]


def test_every_term_at_once_keeps_the_order(rec):
    ex, out = make_batch()
    ex["texture_con"] = torch.tensor([0.5, 0.25])
    names = sorted(ALL_TERMS)                     # the order of the request does not matter
    lf, dic, parts = run(rec, ex, out, names)
    assert rec.entries() == ["geom_losses", "joint_terms", "open2d_terms", "ssim_loss", "photo_losses", "ssim_loss", "perceptual", "lpips",
                             "soft_sil_losses", "mesh_regularizers", "chamfer_distance", "point_mesh_distance", "depth_loss"]
    assert tuple(dic) == ALL_TERMS
    assert parts == [(5, list(GEOM)), (3, list(OPEN2D)), (3, ["texture", "mrgb", "sil"]), (1, ["ssim_tex"]), (2, list(SOFT)), (2, list(MESH)),
                     (1, ["chamfer"]), (1, ["point_mesh"]), (1, ["depth"])]
    assert tuple(rec.only("geom_losses")[8]) == W_GEOM and tuple(rec.only("joint_terms")[5]) == W_JOINT
    assert tuple(rec.only("open2d_terms")[3]) == W_OPEN2D and tuple(rec.only("soft_sil_losses")[2:]) == W_SOFT
    assert tuple(rec.only("mesh_regularizers")[2:]) == W_MESH and tuple(rec.only("photo_losses")[3:]) == W_PHOTO
    assert torch.equal(lf.total(dic, names), torch.stack([dic[k] for k in names]).sum())


def test_the_empty_list(rec):
    ex, out = make_batch()
    lf, dic, parts = run(rec, ex, without(out, "re_img"), [])
    assert dic == {} and parts == [] and rec.calls == []


def test_terms_are_the_31_names():
    assert len(ALL_TERMS) == 31 and len(losses.TERMS) == 31 and set(losses.TERMS) == set(ALL_TERMS)
    for group in (ops.GEOM_TERMS, ops.MESH_REG_TERMS, ops.OPEN2D_TERMS, JOINT, SOFT):
        assert set(group) <= set(losses.TERMS)
    assert (ops.GEOM_TERMS, ops.MESH_REG_TERMS, ops.OPEN2D_TERMS) == (GEOM, MESH, OPEN2D)


def test_the_step_projects_j2d_for_exactly_five_names():
    """(The one test of this file that reads something the term table introduced: before it, traineval kept the five names by hand.)"""
    assert sorted(losses.requested_needing("j2d", losses.TERMS)) == ["bone_direc", "joint_2d", "open_2dj", "open_2dj_de", "open_bone_direc"]
    assert losses.requested_needing("j2d", ["joint_3d", "bone_direc_3d", "sil"]) == []
    assert losses.requested_needing("j2d", ["mpose", "open_2dj_de", "joint_2d"]) == ["open_2dj_de", "joint_2d"]
