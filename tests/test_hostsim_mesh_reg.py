"""The mesh regularisers `triangle` / `normal_consistency` (csrc/mesh_reg.hip: hifihr_mesh_topology_*, hifihr_mesh_reg_fwd / _bwd) on the
host emulator.  The cases are those of tests/test_gpu_mesh_reg.py (tests/mesh_reg_cases.py); the reference is the float64 restatement of
tests/mesh_reg_ref.py."""
import pytest

import kernel_cases as kc
import mesh_reg_cases as mc

_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


def test_known_answers(hostsim_lib):
    mc.known_answers_case(hostsim_lib, "cpu")


def test_topology_counts(hostsim_lib, synth_tables):
    mc.topology_case(hostsim_lib, "cpu", synth_tables)


@pytest.mark.parametrize("case", mc.RANDOM_CASES, ids=_ids)
def test_jittered_grids_match_the_restatement(hostsim_lib, case):
    mc.random_case(hostsim_lib, "cpu", *case)


def test_mano_topology_matches_the_restatement(hostsim_lib, synth_tables):
    mc.mano_case(hostsim_lib, "cpu", synth_tables)


def test_fan_and_book(hostsim_lib):
    mc.fan_case(hostsim_lib, "cpu")


def test_isolated_vertex(hostsim_lib):
    mc.isolated_vertex_case(hostsim_lib, "cpu")


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    mc.refusal_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    mc.random_case(hostsim_lib, "cpu", *mc.RANDOM_CASES[0])
    assert mc.KERNELS <= set(kc.launch_log(hostsim_lib))
