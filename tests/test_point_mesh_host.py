"""Host-only checks of the point-to-mesh distance (no kernel runs): the restatement itself (tests/point_mesh_ref.py) against brute force, the
plane distance and torch float64 autograd; the options, the loss name, the Evaluator's keys and the refusal of CPU tensors.

Bounds of the restatement's sanity checks (float64 throughout, coordinates of magnitude <= 1, so extent^2 <= 4):
    d2 <= the squared distance to every point of a 33 x 33 barycentric grid on the triangle, and d2 >= the squared distance to the
    triangle's plane, each with a slack of 1e-14 for the rounding of the two sides (about 50 float64 epsilons);
    the weights are >= 0 and sum to 1 within 1e-15;
    the analytic gradient against autograd of the torch form: 1e-10 relative to the largest component (expected about 1e-13: both are
    float64; autograd also differentiates the closest point, which by the envelope property adds nothing away from region boundaries)."""
import numpy as np
import pytest
import torch

import point_mesh_ref as pr

SLACK = 1e-14


def _seeded(n, seed):
    g = np.random.RandomState(seed)
    tri = (g.rand(n, 3, 3) - 0.5).astype(np.float32)
    # points round each triangle: wide enough that all seven regions occur
    p = (tri.mean(1) + 1.2 * (g.rand(n, 3) - 0.5)).astype(np.float32)
    return tri, p


def test_restatement_against_brute_force_and_the_plane():
    n = 400
    tri, p = _seeded(n, 0)
    td, pd = tri.astype(np.float64), p.astype(np.float64)
    a, ab, ac = td[:, 0], td[:, 1] - td[:, 0], td[:, 2] - td[:, 0]
    w0, w1, w2, d2, reg = pr.closest(pd - a, ab, ac, pr._dot(ab, ab), pr._dot(ab, ac), pr._dot(ac, ac))
    assert sorted(set(reg.astype(int).tolist())) == list(range(7)), "the seeded samples do not reach all seven regions"
    w = np.stack([w0, w1, w2], -1)
    print(f"[point_mesh] restatement: smallest weight {w.min():.3e}, largest |sum - 1| {np.abs(w.sum(-1) - 1).max():.3e} (bound 1e-15)")
    assert (w >= 0).all() and np.abs(w.sum(-1) - 1).max() <= 1e-15
    # the weights reproduce d2 from the corners themselves
    cp = (td * w[:, :, None]).sum(1)
    assert np.abs(((pd - cp) ** 2).sum(-1) - d2).max() <= SLACK
    # no point of a 33 x 33 barycentric grid is closer
    i, j = np.meshgrid(np.arange(33), np.arange(33), indexing="ij")
    keep = i + j <= 32
    gw = np.stack([(32 - i - j)[keep], i[keep], j[keep]], -1) / 32.0                     # [561, 3]
    grid = np.einsum("gk,nkd->ngd", gw, td)                                                # [n, 561, 3]
    dg = ((pd[:, None, :] - grid) ** 2).sum(-1)
    worst = float((d2[:, None] - dg).max())
    print(f"[point_mesh] restatement: largest d2 - (d2 to a grid point) {worst:.3e} (bound {SLACK:.0e})")
    assert worst <= SLACK
    # ... and the plane is no farther
    nrm = np.cross(ab, ac)
    plane = pr._dot(pd - a, nrm) ** 2 / pr._dot(nrm, nrm)
    worst = float((plane - d2).max())
    print(f"[point_mesh] restatement: largest (plane distance)^2 - d2 {worst:.3e} (bound {SLACK:.0e})")
    assert worst <= SLACK
    inside = reg == 6
    assert np.abs(plane[inside] - d2[inside]).max() <= SLACK                              # in the interior the two are one


def test_restatement_handles_degenerate_faces():
    """Zero-area faces in exact arithmetic: the distance to the segment or point, finite, no warning from a division."""
    tri = np.asarray([[[0, 0, 0], [4, 0, 0], [2, 0, 0]], [[0, 0, 0], [0, 0, 0], [0, 4, 0]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]]], np.float64)
    p = np.asarray([[1, 2, 0], [1, 1, 0], [1, 1, 3]], np.float64)
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(all="raise"):
        w0, w1, w2, d2, _ = pr.closest(p - a, ab, ac, pr._dot(ab, ab), pr._dot(ab, ac), pr._dot(ac, ac))
    assert d2.tolist() == [4.0, 1.0, 4.0] and np.isfinite(np.stack([w0, w1, w2])).all()


def test_restatement_gradient_matches_autograd_of_the_torch_form():
    g = torch.Generator().manual_seed(0)
    B, N, V, F = 2, 23, 17, 29
    p32, v32 = torch.rand(B, N, 3, generator=g) - 0.5, torch.rand(B, V, 3, generator=g) - 0.5
    faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F)])
    w, gout = (0.7, 1.3), -1.7
    for weights in (w, (w[0], 0.0), (0.0, w[1])):
        ref = pr.point_mesh(p32.numpy(), v32.numpy(), faces.numpy(), weights[0], weights[1], gout)
        p, v = p32.double().requires_grad_(True), v32.double().requires_grad_(True)
        value = pr.point_mesh_torch(p, v, faces, *weights)
        (value * float(np.float32(gout))).backward()
        ev = abs(float(value.detach()) - ref["value"]) / abs(ref["value"])
        figures = [ev]
        for got, want in ((ref["gp"], p.grad.numpy()), (ref["gv"], v.grad.numpy())):
            assert float(np.abs(want).max()) > 0
            figures.append(float(np.abs(got - want).max()) / float(np.abs(want).max()))
        print(f"[point_mesh] restatement vs autograd, weights {weights}: value {figures[0]:.2e}, gp {figures[1]:.2e}, gv {figures[2]:.2e} "
              f"relative (bound 1e-10)")
        assert max(figures) <= 1e-10, figures


def test_vertex_corner_table():
    faces = np.asarray([[0, 1, 2], [2, 1, 3], [0, 2, 5]], np.int32)
    off, corner = pr.vertex_corner_table(faces, 6)
    assert off.tolist() == [0, 2, 4, 7, 8, 8, 9] and corner.tolist() == [0, 6, 1, 4, 2, 3, 7, 5, 8]


def test_options_default_and_override():
    from hifihr_amd import options
    a = options.make_args()
    assert a.lambda_point_mesh == 1.0 and a.lambda_point_mesh_faces == 0.0 and a.point_mesh_metric is False and "point_mesh" not in a.losses
    b = options.make_args(lambda_point_mesh=250.0, lambda_point_mesh_faces=2.0, point_mesh_metric=True)
    assert b.lambda_point_mesh == 250.0 and b.lambda_point_mesh_faces == 2.0 and b.point_mesh_metric is True
    assert "point_mesh" not in options.baseline_config2_args().losses


def test_the_loss_name_is_known_and_reaches_the_kernels():
    """The name is not ignored: LossFunction goes to ops.point_mesh_distance, which has no CPU path."""
    from hifihr_amd import losses, options
    from hifihr_amd._lib import HifihrError
    assert "point_mesh" in losses.TERMS
    args = options.make_args()
    ex = {"verts": torch.zeros(1, 5, 3)}
    out = {"mano_verts": torch.zeros(1, 4, 3), "_faces_i32": torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)}
    with pytest.raises(HifihrError):
        losses.LossFunction()(ex, out, ["point_mesh"], "FreiHand", args)
    assert losses.LossFunction()(ex, out, [], "FreiHand", args) == {}


def test_ops_refuse_cpu_tensors():
    from hifihr_amd import evaluate, ops
    from hifihr_amd._lib import HifihrError
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for fn in (ops.point_mesh_distance, ops.point_mesh_sums):
        with pytest.raises(HifihrError):
            fn(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3), faces)
    with pytest.raises(HifihrError):
        evaluate.point_to_surface(torch.zeros(1, 5, 3), faces, torch.zeros(1, 4, 3))


def test_evaluator_keyword_and_keys():
    import train_hrnet
    from hifihr_amd import evaluate, options
    assert evaluate.POINT_MESH_KEYS == ("mesh_p2s", "mesh_al_p2s")
    assert not set(evaluate.POINT_MESH_KEYS) & (set(evaluate.BENCHMARK_KEYS) | set(evaluate.CHAMFER_KEYS))
    assert evaluate.Evaluator().point_mesh is False and evaluate.Evaluator(point_mesh=True).point_mesh is True
    assert evaluate.Evaluator(benchmark=True, chamfer=True).point_mesh is False
    assert evaluate.Evaluator().summary() == {} and evaluate.Evaluator(point_mesh=True).summary() == {}
    assert train_hrnet.make_evaluator(options.make_args(), "cpu").point_mesh is False
    assert train_hrnet.make_evaluator(options.make_args(point_mesh_metric=True), "cpu").point_mesh is True
    assert train_hrnet.build_args(train_hrnet.parse([])).point_mesh_metric is False
    report = train_hrnet.benchmark_report({"f_score_5": 0.5, "mesh_chamfer": 1.5e-4, "mesh_p2s": 2.5e-5, "mesh_al_p2s": 5e-6, "pose_3d": 1.0})
    assert report.splitlines() == ["f_score_5: 0.500000", "mesh_chamfer: 1.500000e-04", "mesh_p2s: 2.500000e-05", "mesh_al_p2s: 5.000000e-06"]
    assert train_hrnet.benchmark_report({"f_score_5": 0.5}) == "f_score_5: 0.500000"
