"""Host-only checks of the mesh regularisers' Python surface (no kernel runs): the options, the loss names, the refusal of CPU tensors."""
import pytest
import torch

# the `losses` list of the reference's config/FreiHAND/fully_superv_freihand_shape.json
FULLY_SUPERV_FREIHAND_SHAPE_LOSSES = ["joint_2d", "joint_3d", "bone_direc", "scale", "sil", "triangle"]


def test_options_carry_the_two_weights():
    from hifihr_amd import options
    a = options.make_args()
    assert a.lambda_laplacian == 0.1 and a.lambda_normal_consistency == 0.01
    assert "triangle" not in a.losses and "normal_consistency" not in a.losses
    assert options.make_args(lambda_normal_consistency=0.5).lambda_normal_consistency == 0.5


def test_reference_config_names_no_term_the_loss_function_ignores():
    from hifihr_amd import losses, ops
    assert ops.MESH_REG_TERMS == ("triangle", "normal_consistency")
    assert set(ops.MESH_REG_TERMS) <= set(losses.TERMS)
    assert [k for k in FULLY_SUPERV_FREIHAND_SHAPE_LOSSES if k not in losses.TERMS] == []


@pytest.mark.parametrize("name", ["triangle", "normal_consistency"])
def test_loss_function_reaches_the_kernels_and_refuses_cpu_tensors(name):
    """The name is not ignored: LossFunction goes to ops.mesh_regularizers, which has no CPU path."""
    from hifihr_amd import options
    from hifihr_amd._lib import HifihrError
    from hifihr_amd.losses import LossFunction
    args = options.make_args()
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    for outputs in ({"mano_verts": torch.zeros(1, 4, 3), "_faces_i32": faces}, {"verts": torch.zeros(1, 4, 3), "faces": faces}):
        with pytest.raises(HifihrError):
            LossFunction()({}, outputs, [name], "FreiHand", args)


def test_ops_refuse_cpu_tensors():
    from hifihr_amd import ops
    from hifihr_amd._lib import HifihrError
    with pytest.raises(HifihrError):
        ops.mesh_regularizers(None, torch.zeros(1, 4, 3), 0.1, 0.01)
    with pytest.raises(HifihrError):
        ops.mesh_topology_of(torch.tensor([[0, 1, 2]], dtype=torch.int32), 3)
