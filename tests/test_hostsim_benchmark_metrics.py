"""The benchmark-metric kernels of csrc/eval.hip (hifihr_point_error_hist, hifihr_fscore_counts) on the host emulator, with what
hifihr_amd.evaluate makes of their counts, plus the host-only front-end checks.  The cases are those of tests/test_gpu_benchmark_metrics.py
(tests/benchmark_cases.py); the references are the float64 restatement of tests/benchmark_ref.py and the reference's own EvalUtil
(tests/golden/benchmark_metrics.npz)."""
import numpy as np
import pytest
import torch

import benchmark_cases as bc
import kernel_cases as kc

_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.mark.parametrize("shape", bc.HIST_SHAPES, ids=_ids)
def test_histogram_counts_equal_the_restatement(hostsim_lib, shape):
    bc.hist_raw_case(hostsim_lib, "cpu", *shape)


def test_histogram_skips_an_invisible_keypoint(hostsim_lib):
    bc.hist_masked_case(hostsim_lib, "cpu")


def test_histogram_counts_exact_hits_in_their_bin(hostsim_lib):
    bc.hist_constructed_case(hostsim_lib, "cpu")


def test_pck_auc_matches_the_reference_evalutil(hostsim_lib, golden_dir):
    bc.hist_fixture_case(hostsim_lib, "cpu", golden_dir)


@pytest.mark.parametrize("shape", bc.FSCORE_SHAPES, ids=_ids)
def test_fscore_counts_equal_the_restatement(hostsim_lib, shape):
    bc.fscore_raw_case(hostsim_lib, "cpu", *shape)


def test_fscore_constructed_cases(hostsim_lib):
    bc.fscore_constructed_case(hostsim_lib, "cpu")


def test_aligned_forms_are_bracketed_by_the_float64_reference(hostsim_lib, golden_dir):
    bc.aligned_case(hostsim_lib, "cpu", golden_dir)


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    bc.refusal_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    bc.hist_constructed_case(hostsim_lib, "cpu")
    bc.fscore_constructed_case(hostsim_lib, "cpu")
    assert {"point_error_hist_kernel", "fscore_counts_kernel"} <= set(kc.launch_log(hostsim_lib))


def test_cpu_tensors_are_refused():
    from hifihr_amd._lib import HifihrError
    from hifihr_amd.evaluate import Evaluator, fscore, pck_auc
    a = torch.zeros(2, 21, 3)
    with pytest.raises(HifihrError):
        pck_auc(a, a)
    with pytest.raises(HifihrError):
        fscore(a, a)
    ev = Evaluator(benchmark=True)
    ev.xyz_pred.append(a)
    with pytest.raises(HifihrError):
        ev.summary(xyz_gt=np.zeros((2, 21, 3), np.float32))


def test_front_end_option():
    import sys
    sys.path.insert(0, kc.REPO)
    import train_hrnet
    from hifihr_amd import options
    from hifihr_amd.evaluate import BENCHMARK_KEYS
    assert options.make_args().benchmark_metrics is True
    assert train_hrnet.make_evaluator(options.make_args(), "cpu").benchmark is True
    assert train_hrnet.make_evaluator(options.make_args(benchmark_metrics=False), "cpu").benchmark is False
    assert train_hrnet.build_args(train_hrnet.parse([])).benchmark_metrics is True
    summary = {k: 0.5 for k in BENCHMARK_KEYS}
    summary["pose_3d"] = 1.0
    lines = train_hrnet.benchmark_report(summary).splitlines()
    assert [ln.split(":")[0] for ln in lines] == list(BENCHMARK_KEYS) and len(BENCHMARK_KEYS) == 12
