"""HifihrLib's marshaller (`_call` / `_run`): what each kind of C parameter accepts, refuses and hands on, on a plan built from a few
lines of header text and a stub in place of the library that records what it receives (no library build; one GPU test for `stream`)."""
import ctypes
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

HEADER = """
typedef struct hifihr_thing hifihr_thing;
const char* hifihr_last_error(void);
int hifihr_mix(const hifihr_thing* h, const float* x_d, const int32_t* idx_d, const void* mask_d, int n, long rows, size_t ws_bytes,
               float eps, float* y_d, void* stream);
int hifihr_host(const float* lam3_host, int n);
int hifihr_sync(void* stream);
size_t hifihr_bytes(int n);
long hifihr_count(int n);
int hifihr_flag(int n);
"""


class _Entry:
    def __init__(self, name, log, result):
        self.name, self.log, self.result = name, log, result

    def __call__(self, *args):
        self.log.append((self.name, args))
        return self.result


def _stub_lib(header=HEADER, **results):
    """-> (a HifihrLib bound to a recording stub, the stub's log of (entry, arguments)); results: entry=value to return (default 0)."""
    from hifihr_amd._abi import prototypes
    from hifihr_amd._lib import HifihrLib
    table, log, stub = prototypes(header), [], type("StubC", (), {})()
    for name in table:
        setattr(stub, name, _Entry(name, log, results.get(name, b"the stub said no" if name == "hifihr_last_error" else 0)))
    lib = HifihrLib.__new__(HifihrLib)
    lib._bind(stub, table)
    return lib, log


def _mix_args(**over):
    a = dict(h=c_void_p(0x1000), x=torch.zeros(2, 3), idx=torch.zeros(4, dtype=torch.int32), mask=torch.zeros(5, dtype=torch.uint8),
             n=3, rows=4, ws_bytes=5, eps=0.5, y=torch.zeros(6))
    a.update(over)
    return list(a.values())


def _address(p):
    return ctypes.cast(p, c_void_p).value


def test_stub_is_bound_like_a_library():
    from hifihr_amd._abi import prototypes
    lib, _ = _stub_lib()
    for name, (restype, argtypes, _) in prototypes(HEADER).items():
        assert getattr(lib.c, name).restype is restype and getattr(lib.c, name).argtypes == argtypes


def test_tensors_arrive_as_their_addresses_and_by_value_arguments_as_plain_values():
    lib, log = _stub_lib()
    args = _mix_args(n=np.int64(3), rows=np.int32(4), ws_bytes=True, eps=np.float32(0.5))
    lib._run("hifihr_mix", *args)
    (name, got), = log
    assert name == "hifihr_mix" and len(got) == 10
    assert got[0] is args[0]                                                      # a handle passes through unchanged
    assert [_address(got[i]) for i in (1, 2, 8)] == [args[i].data_ptr() for i in (1, 2, 8)]
    assert got[1]._type_ is ctypes.c_float and got[2]._type_ is ctypes.c_int32                  # (what ctypes takes for float* / int32_t*)
    assert got[3] == args[3].data_ptr()
    assert [type(v) for v in got[4:8]] == [int, int, int, float] and got[4:8] == (3, 4, 1, 0.5)
    assert got[9] == 0                                                            # CPU tensors only: the default stream


def test_channels_last_dense_is_accepted_for_float_pointers():
    lib, log = _stub_lib()
    x = torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    lib._run("hifihr_mix", *_mix_args(x=x))
    assert _address(log[0][1][1]) == x.data_ptr()


@pytest.mark.parametrize("what,bad", [
    ("x", lambda: torch.zeros(2, 3, dtype=torch.float64)),
    ("x", lambda: torch.zeros(6, dtype=torch.int32)),
    ("x", lambda: torch.zeros(3, 2).t()),                                         # float32, not dense
    ("x", lambda: torch.zeros(2, 3, 4, 5)[:, :, ::2]),
    ("y", lambda: torch.zeros(6, dtype=torch.float64)),
    ("idx", lambda: torch.zeros(4, dtype=torch.int64)),
    ("idx", lambda: torch.zeros(4, dtype=torch.float32)),
    ("idx", lambda: torch.zeros(4, 2, dtype=torch.int32).t()),
    ("mask", lambda: torch.zeros(4, 2, dtype=torch.uint8).t()),                   # void*: any element type, but contiguous
    ("mask", lambda: torch.zeros(8, dtype=torch.float64)[::2]),
])
def test_a_wrong_tensor_raises_before_the_call(what, bad):
    lib, log = _stub_lib()
    with pytest.raises(AssertionError):
        lib._run("hifihr_mix", *_mix_args(**{what: bad()}))
    assert log == []


def test_none_is_null_and_ctypes_values_pass_through():
    lib, log = _stub_lib()
    lib._run("hifihr_mix", *_mix_args(h=None, x=None, idx=None, mask=None, y=None))
    got = log[0][1]
    assert all(got[i] is None for i in (0, 1, 2, 3, 8)) and got[9] == 0           # (ctypes turns None into NULL for every pointer type)
    lam3, addr, n = (ctypes.c_float * 3)(1.0, 2.0, 3.0), c_void_p(0x2000), c_int(0)
    lib._run("hifihr_mix", *_mix_args(x=lam3, mask=addr, h=0x3000, idx=ctypes.byref(n)))
    got = log[1][1]
    assert got[1] is lam3 and got[3] is addr and got[0] == 0x3000 and _address(got[2]) == ctypes.addressof(n)
    lib._run("hifihr_host", lam3, 3)
    assert log[2] == ("hifihr_host", (lam3, 3))                                   # no `stream` parameter: none is added


@pytest.mark.parametrize("drop", [1, -1])
def test_a_wrong_number_of_arguments_names_the_entry_and_its_parameters(drop):
    from hifihr_amd._lib import HifihrError
    lib, log = _stub_lib()
    args = _mix_args()[:-1] if drop == 1 else _mix_args() + [0]
    with pytest.raises(HifihrError) as e:
        lib._run("hifihr_mix", *args)
    assert "hifihr_mix" in str(e.value) and "idx_d" in str(e.value) and "ws_bytes" in str(e.value) and log == []
    with pytest.raises(HifihrError, match="hifihr_host"):
        lib._call("hifihr_host", (ctypes.c_float * 3)(), 3, stream=7)            # an entry without a `stream` parameter takes none


def test_a_status_raises_with_the_entry_name_and_raw_results_are_returned_unchecked():
    from hifihr_amd._lib import HifihrError
    lib, log = _stub_lib(hifihr_mix=3, hifihr_bytes=1 << 40, hifihr_count=-5, hifihr_flag=3)
    with pytest.raises(HifihrError) as e:
        lib._run("hifihr_mix", *_mix_args())
    assert "hifihr_mix" in str(e.value) and "(3)" in str(e.value) and "the stub said no" in str(e.value) and len(log) == 2
    assert lib._call("hifihr_mix", *_mix_args()) == 3
    assert lib._call("hifihr_bytes", 2) == 1 << 40 and lib._call("hifihr_count", np.int64(2)) == -5 and lib._call("hifihr_flag", 2) == 3
    assert log[-1] == ("hifihr_flag", (2,))


def test_stream_is_zero_for_cpu_tensors_and_the_keyword_overrides_it():
    lib, log = _stub_lib()
    lib._run("hifihr_mix", *_mix_args())
    lib._run("hifihr_mix", *_mix_args(), stream=0x4000)
    handle = c_void_p(0x5000)
    lib._run("hifihr_sync", stream=handle)
    lib._run("hifihr_sync")
    lib._run("hifihr_sync", stream=torch.zeros(1))                                # a tensor: its device's current stream
    assert log[0][1][9] == 0 and log[1][1][9] == 0x4000 and log[2][1] == (handle,) and log[2][1][0] is handle and log[3][1] == (0,)
    assert log[4][1][0].value in (0, None)


def test_every_entry_with_a_stream_takes_it_last_and_returns_a_status():
    """The convention `_call` / `_run` rely on: a prototype that breaks it fails here, not in a kernel."""
    from hifihr_amd._abi import prototypes
    streamed = 0
    for name, (restype, argtypes, argnames) in prototypes().items():
        assert "stream" not in argnames[:-1], name
        if argnames[-1:] == ["stream"]:
            assert restype is c_int and argtypes[-1] is c_void_p, name
            streamed += 1
    assert streamed >= 130


@pytest.mark.gpu
def test_stream_is_the_current_stream_of_the_first_cuda_tensor():
    lib, log = _stub_lib()
    x, y = torch.empty(2, 3, device="cuda"), torch.empty(6, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        lib._run("hifihr_mix", *_mix_args(x=x, y=y))
        lib._run("hifihr_mix", *_mix_args(x=None, y=y))                           # a None first: the next CUDA tensor decides
    lib._run("hifihr_mix", *_mix_args(x=x, y=y))
    lib._run("hifihr_mix", *_mix_args(x=x, y=y), stream=0x4000)
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    assert [c[1][9] for c in log] == [side.cuda_stream, side.cuda_stream, torch.cuda.current_stream().cuda_stream, 0x4000]
    assert _address(log[0][1][1]) == x.data_ptr() and log[1][1][1] is None
