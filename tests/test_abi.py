"""The C-ABI library loads and exports every symbol include/hifihr.h declares, and the Python binding takes every signature from that
header (no compute without a GPU)."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_long, c_size_t, c_void_p

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(REPO, "include", "hifihr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hifihr_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported():
    lib_path = os.path.join(REPO, "hifihr_amd", "libhifihr.so")
    if not os.path.exists(lib_path):
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "hifihr_amd", "csrc"), "-j8"], check=True)
    import torch  # noqa: F401  (libamdhip64 is resolved from torch's copy)
    lib = ctypes.CDLL(lib_path)
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/hifihr.h but not exported"
    lib.hifihr_version.restype = ctypes.c_int
    assert lib.hifihr_version() >= 2


def test_python_binding_covers_the_header():
    from hifihr_amd._lib import HifihrLib, LIB_PATH
    lib = HifihrLib(LIB_PATH)
    for n in _declared():
        getattr(lib.c, n)


_FP, _IP, _VP = POINTER(c_float), POINTER(c_int32), c_void_p

# one prototype of each shape the type rules of hifihr_amd/_abi.py tell apart, written out by hand from include/hifihr.h
PINNED = {
    "hifihr_mano_create": (c_int, [POINTER(c_void_p), _FP, _FP, _FP, _FP, _FP, _FP, _FP]),                      # handle **, host float*
    "hifihr_bn_act_fwd": (c_int, [_FP, _FP, _FP, _FP, _FP, c_int, c_long, c_int, c_float, c_float, _FP, _FP, _FP, _FP, _FP, _VP]),   # long, float
    "hifihr_conv2d_bwd_weight_ws": (c_int, [_FP, _FP, _FP, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _VP, c_size_t, _VP]),
    "hifihr_conv2d_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "hifihr_wino_tiles": (c_long, [c_int, c_int, c_int, c_int]),
    "hifihr_mesh_topology_create": (c_void_p, [_IP, c_int, c_int]),                                             # returns a handle
    "hifihr_last_error": (c_char_p, []),
    "hifihr_chamfer_geometry": (None, [_IP, _IP]),                                                              # void, int*
    "hifihr_loss_total_fwd": (c_int, [POINTER(_FP), _IP, c_int, _FP, _VP]),                                     # const float* const*
    "hifihr_linear_fwd_group": (c_int, ["LinearDesc*", c_int, _VP]),                                            # struct pointer (filled in below)
    "hifihr_bgemm_describe": (c_int, [c_int, c_int, c_int, c_int, c_int, c_char_p, c_int]),                     # char*
    "hifihr_chamfer_fwd": (c_int, [_FP, _FP, c_int, c_int, c_int, c_float, c_float, _IP, _IP, _VP, _VP, _VP, _FP, _VP, _VP]),   # double* untyped
    "hifihr_joint_terms_fwd": (c_int, [_FP, _FP, _FP, _FP, c_int, c_int, c_int, _FP, _FP, _VP]),                # host array lam3
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signature(name):
    from hifihr_amd._abi import prototypes
    from hifihr_amd._lib import _LinearDesc
    restype, argtypes = PINNED[name]
    argtypes = [POINTER(_LinearDesc) if t == "LinearDesc*" else t for t in argtypes]
    got = prototypes()[name]
    assert got[0] is restype, (name, got[0])
    assert len(got[1]) == len(argtypes) == len(got[2]), (name, got[2])
    for i, (g, e) in enumerate(zip(got[1], argtypes)):
        assert g is e, (name, i, got[2][i], g, e)


def test_table_covers_the_header_and_is_parsed_once():
    from hifihr_amd._abi import prototypes
    assert sorted(prototypes()) == _declared()
    assert prototypes() is prototypes()


def _bound_from_the_table(lib):
    from hifihr_amd._abi import prototypes
    for name, (restype, argtypes, _) in prototypes().items():
        fn = getattr(lib.c, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name


def test_every_entry_is_bound_from_the_table():
    from hifihr_amd._lib import HifihrLib, LIB_PATH
    _bound_from_the_table(HifihrLib(LIB_PATH))


def test_every_hostsim_entry_is_bound_from_the_table():
    import kernel_cases as kc
    _bound_from_the_table(kc.build_hostsim())


_OK = "int hifihr_ok(const float* x_d, int n, void* stream);\n"


@pytest.mark.parametrize("text,what", [
    (_OK + "int hifihr_scale(float* x_d, double s, void* stream);\n", "a by-value double"),
    (_OK + "int hifihr_walk(const float* x_d, int (*visit)(int), void* stream);\n", "a parameter list the regex cannot close"),
    (_OK + "int hifihr_open(const float* x_d, int n;\n", "a parameter list that never closes"),
    (_OK + "typedef struct hifihr_job { int (*run)(int); int hifihr_foo(int); } hifihr_job;\n", "a name only inside a struct body"),
    (_OK + "#define HIFIHR_CALL(x) hifihr_foo(x)\n", "a name only inside a macro"),
])
def test_parser_is_strict(text, what):
    from hifihr_amd._abi import prototypes
    from hifihr_amd._lib import HifihrError
    assert list(prototypes(_OK)) == ["hifihr_ok"]                    # (the text the cases share is itself accepted)
    with pytest.raises(HifihrError):
        prototypes(text)


def test_missing_header_is_an_error(monkeypatch, tmp_path):
    from hifihr_amd import _abi
    from hifihr_amd._lib import HifihrError
    missing = str(tmp_path / "hifihr.h")
    monkeypatch.setattr(_abi, "HEADER_PATH", missing)
    _abi._header_table.cache_clear()
    try:
        with pytest.raises(HifihrError, match=re.escape(missing)):
            _abi.prototypes()
    finally:
        monkeypatch.undo()
        _abi._header_table.cache_clear()
