"""ctypes binding of libhifihr.so (the C ABI in include/hifihr.h).

`get_lib()` loads the in-tree HIP build and FAILS LOUDLY when it is missing -- there is no CPU or
PyTorch fallback for the hot path.  `HifihrLib` itself only marshals pointers, so the test-suite can also
point it at tests/hostsim/libhifihr_hostsim.so (the same kernel sources compiled against a HIP
execution-model emulator) to exercise the kernels without a GPU; the package never does that.
No signature is written down here: every `argtypes` / `restype` is read from the header (hifihr_amd/_abi.py), and every
call is marshalled from that table (`HifihrLib._call` / `_run`): a wrapper lists the C arguments in header order and nothing else.
"""
from __future__ import annotations

import ctypes
import os
import struct
from ctypes import POINTER, c_double, c_float, c_int, c_int32, c_long, c_size_t, c_void_p

import numpy as np
import torch  # noqa: F401  (must be imported first: the library binds to torch's libamdhip64)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhifihr.so")

_c_float_p = POINTER(c_float)
_c_int_p = POINTER(c_int32)


class _LinearDesc(ctypes.Structure):          # include/hifihr.h: hifihr_linear_desc
    _fields_ = [("x", c_void_p), ("w", c_void_p), ("b", c_void_p), ("y", c_void_p), ("B", c_int), ("I", c_int), ("O", c_int), ("act", c_int),
                ("dy", c_void_p), ("dz_scratch", c_void_p), ("dW_acc", c_void_p), ("db_acc", c_void_p), ("dx", c_void_p)]


class HifihrError(RuntimeError):
    pass


def _check_f32(t):
    dense = t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))
    assert t.dtype == torch.float32 and dense, (t.dtype, t.shape, t.stride())


def _check_i32(t):
    assert t.dtype == torch.int32 and t.is_contiguous()


def _fp(t):
    """Device (or host) pointer of a contiguous fp32 tensor, or NULL for None."""
    if t is None:
        return None
    _check_f32(t)
    return ctypes.cast(t.data_ptr(), _c_float_p)


def _ip(t):
    if t is None:
        return None
    _check_i32(t)
    return ctypes.cast(t.data_ptr(), _c_int_p)


# What `HifihrLib._marshal` gives a pointer parameter for a tensor: the same checks, and for float* / int32_t* a zero-length array at the
# tensor's address, which ctypes takes for a pointer to its element type and builds in a quarter of ctypes.cast's time
_f32_at, _i32_at = (c_float * 0).from_address, (c_int32 * 0).from_address


def _f32_arg(t):
    _check_f32(t)
    return _f32_at(t.data_ptr())


def _i32_arg(t):
    _check_i32(t)
    return _i32_at(t.data_ptr())


def _void_arg(t):
    """Address of a contiguous tensor of any element type, for a parameter the header leaves untyped."""
    assert t.is_contiguous(), (t.dtype, t.shape, t.stride())
    return t.data_ptr()


def _stream_of(t):
    if t is not None and t.is_cuda:
        return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    return c_void_p(0)


# How one C parameter is marshalled, by its ctypes type in the header's table: by value through int / float, a pointer through the
# check a tensor must pass to be given to it (anything but a tensor passes through, and so does every argument of a type that is not
# listed: float**, hifihr_linear_desc*, char*, the handle** of a create call)
_KIND = {c_int: int, c_long: int, c_size_t: int, c_float: float, _c_float_p: _f32_arg, _c_int_p: _i32_arg, c_void_p: _void_arg}
_Tensor = torch.Tensor


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def _host_f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_c_float_p)


def _host_i32(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(_c_int_p)


def _host_f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    return a, a.ctypes.data_as(POINTER(c_double))


def _fp_table(tensors):
    """Host array of the float* of each tensor, for a `float**` parameter."""
    return (_c_float_p * len(tensors))(*[_fp(t) for t in tensors])


def _floats(values, n):
    assert len(values) == n, (len(values), n)
    return (c_float * n)(*[float(v) for v in values])


class HifihrLib:
    def __init__(self, path: str = LIB_PATH):
        if not os.path.exists(path):
            raise HifihrError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C hifihr_amd/csrc`). The HIP extension is mandatory; there is no fallback path.")
        self.path = path
        self._zero_page = set()                # devices whose zero page exists (zero_page_ready)
        self._pair_ok = {}                     # (N, H, W, C, K) -> hifihr_wino4_bwd_gemm_pair_supported
        from ._abi import prototypes           # (imported here: _abi takes HifihrError and _LinearDesc from this module)
        self._bind(ctypes.CDLL(path), prototypes())

    def _bind(self, c, table):
        """Give every entry of `c` the signature `table` (hifihr_amd/_abi.py) holds for it, and build the plan `_marshal` works from:
        entry -> (function, number of parameters before `stream`, (position, tensor check) of each pointer, positions of the by-value
        integers, positions of the by-value floats, whether a trailing `stream` follows, the parameters' names)."""
        self.c, self._plan = c, {}
        for name, (restype, argtypes, argnames) in table.items():    # every signature is include/hifihr.h's own
            fn = getattr(c, name)
            fn.restype, fn.argtypes = restype, argtypes
            n = len(argnames) - (argnames[-1:] == ["stream"])
            kinds = [_KIND.get(t) for t in argtypes[:n]]
            self._plan[name] = (fn, n, tuple((i, k) for i, k in enumerate(kinds) if k not in (int, float, None)),
                                tuple(i for i, k in enumerate(kinds) if k is int), tuple(i for i, k in enumerate(kinds) if k is float),
                                n < len(argnames), tuple(argnames[:n]))

    # ------------------------------------------------------------------
    def check(self, rc: int, what: str):
        if rc != 0:
            raise HifihrError(f"{what} failed ({rc}): {self.c.hifihr_last_error().decode()}")

    def _marshal(self, entry, args, stream):
        """-> (function, C arguments) of one call of `entry`; `args` are its C arguments in header order without the trailing `stream`.
        float* / int32_t*: a tensor passes `_fp`'s / `_ip`'s check; void*: a tensor must be contiguous; None is NULL; ctypes pointers,
        host arrays, handles and addresses pass through; by-value arguments become int / float.  `stream` is the current stream of the
        first CUDA tensor's device (0 without one) unless the caller gives a handle, or a tensor whose device's stream is meant."""
        fn, n, pointers, ints, floats, streamed, names = self._plan[entry]
        if len(args) != n or (stream is not None and not streamed):
            raise HifihrError(f"{entry} takes {n} arguments ({', '.join(names)}){' and a stream' * streamed}, got {len(args)}"
                              f"{'' if stream is None else ' and a stream'}")
        out, dev = list(args), None
        for i, pointer_of in pointers:
            a = out[i]
            if type(a) is _Tensor or isinstance(a, _Tensor):
                if dev is None and a.is_cuda:
                    dev = a.device
                out[i] = pointer_of(a)
        for i in ints:
            if type(out[i]) is not int:
                out[i] = int(out[i])
        for i in floats:
            out[i] = float(out[i])
        if streamed:
            if stream is None:
                stream = 0 if dev is None else torch.cuda.current_stream(dev).cuda_stream
            elif isinstance(stream, _Tensor):
                stream = _stream_of(stream)
            out.append(stream)
        return fn, out

    def _call(self, entry, *args, stream=None):
        """Call `entry` (`_marshal`) and return its raw result."""
        fn, out = self._marshal(entry, args, stream)
        return fn(*out)

    def _run(self, entry, *args, stream=None):
        """Call an entry that returns a status: anything but 0 raises with the entry's name and hifihr_last_error()."""
        fn, out = self._marshal(entry, args, stream)
        rc = fn(*out)
        if rc != 0:
            self.check(rc, entry)

    def version(self):
        return self._call("hifihr_version")

    # ---- MANO --------------------------------------------------------
    def mano_create(self, tables) -> c_void_p:
        h = c_void_p()
        keep = [_host_f32(a) for a in (tables.v_template, tables.shapedirs, tables.posedirs, tables.J_regressor,
                                    tables.weights, tables.hands_components, tables.hands_mean)]
        self._run("hifihr_mano_create", ctypes.byref(h), *[k[1] for k in keep])
        return h

    def mano_destroy(self, h):
        self._call("hifihr_mano_destroy", h)

    def mano_lbs_fwd(self, h, pose, beta, verts, jtr, saved):
        B = pose.shape[0]
        assert pose.shape == (B, 48) and beta.shape == (B, 10) and verts.shape == (B, 778, 3)
        self._run("hifihr_mano_lbs_fwd", h, pose, beta, B, verts, jtr, saved)

    def mano_lbs_bwd(self, h, pose, beta, saved, gverts, gjtr, gpose, gbeta):
        self._run("hifihr_mano_lbs_bwd", h, pose, beta, saved, gverts, gjtr, pose.shape[0], gpose, gbeta)

    def mano_joints_fwd(self, h, verts, root_id, joints_rel, verts_rel, root):
        self._run("hifihr_mano_joints_fwd", h, verts, verts.shape[0], root_id, joints_rel, verts_rel, root)

    def mano_joints_bwd(self, h, gjoints_rel, gverts_rel, groot, root_id, gverts):
        self._run("hifihr_mano_joints_bwd", h, gjoints_rel, gverts_rel, groot, gverts.shape[0], root_id, gverts)

    def mano_full_fwd(self, h, pose, beta, root_id, root_xyz, verts, joints_rel, verts_rel, verts_cam, root, saved):
        """hifihr_mano_full_fwd: the layer, then joint regression + root-relative step + camera-space offset."""
        self._run("hifihr_mano_full_fwd", h, pose, beta, pose.shape[0], root_id, root_xyz, verts, joints_rel, verts_rel, verts_cam, root, saved)

    def mano_full_bwd(self, h, pose, beta, saved, gjoints_rel, gverts_rel, gverts_cam, groot, root_id, gpose, gbeta, gpose_add=None,
                      gbeta_add=None):
        self._run("hifihr_mano_full_bwd", h, pose, beta, saved, gjoints_rel, gverts_rel, gverts_cam, groot, gpose_add, gbeta_add,
                  pose.shape[0], root_id, gpose, gbeta)

    def mano_fit(self, h, pose, beta, root, K, kp2d, conf2d, kp3d, conf3d, prior, lr, iters, weights6, lr_mult4, root_id, trace, grad0, done):
        """hifihr_mano_fit: the whole keypoint fit in one launch; pose [B,48] / beta [B,10] / root [B,3] are updated in place.
        prior = (lo, hi, w) [48] each, or None; lr [iters] on the device (None for iters == 0); trace [B,iters+1,8], done int32 [B]."""
        B = pose.shape[0]
        assert pose.shape == (B, 48) and beta.shape == (B, 10) and root.shape == (B, 3) and K.shape == (B, 3, 3), (pose.shape, K.shape)
        assert kp2d.shape == (B, 21, 2) and conf2d.numel() == B * 21 and trace.shape == (B, iters + 1, 8) and done.shape == (B,)
        assert lr is None or lr.numel() == iters, (iters, None if lr is None else lr.shape)
        for t, numel in ((kp3d, B * 63), (conf3d, B * 21), (grad0, B * 61)) + tuple((p, 48) for p in (prior or ())):
            assert t is None or t.numel() == numel, (t.shape, numel)
        lo, hi, w = prior if prior is not None else (None, None, None)
        self._run("hifihr_mano_fit", h, pose, beta, root, K, kp2d, conf2d, kp3d, conf3d, lo, hi, w, lr, iters, _floats(weights6, 6),
                  _floats(lr_mult4, 4), root_id, B, trace, grad0, done)

    # ---- generic LBS (NIMBLE-shaped layer) -----------------------------
    def lbs_create(self, v_template, shapedirs, j_regressor, weights, parents) -> c_void_p:
        V, J, S = int(v_template.shape[0]), int(weights.shape[1]), int(shapedirs.shape[2])
        assert shapedirs.shape == (V, 3, S) and j_regressor.shape == (J, V) and weights.shape == (V, J) and len(parents) == J
        h = c_void_p()
        keep = [_host_f32(a) for a in (v_template, shapedirs, j_regressor, weights)] + [_host_i32(parents)]
        self._run("hifihr_lbs_create", ctypes.byref(h), V, J, S, *[k[1] for k in keep])
        return h

    def lbs_destroy(self, h):
        self._call("hifihr_lbs_destroy", h)

    def lbs_fwd(self, h, theta, beta, verts, joints):
        self._run("hifihr_lbs_fwd", h, theta, beta, theta.shape[0], verts, joints)

    def lbs_bwd(self, h, theta, beta, gverts, gjoints, scratch, gtheta, gbeta):
        self._run("hifihr_lbs_bwd", h, theta, beta, gverts, gjoints, theta.shape[0], scratch, gtheta, gbeta)

    # ---- convolution (NHWC, f32 MFMA implicit GEMM) --------------------
    # ws: an optional zero-initialised, self-cleaning workspace tensor (any dtype, contiguous)
    def conv2d_workspace_bytes(self, N, H, W, C, K, R, S, stride, pad, bwd_data=False):
        return self._call("hifihr_conv2d_workspace_bytes", N, H, W, C, K, R, S, stride, pad, bool(bwd_data))

    def conv2d_fwd(self, x, w, bias, y, N, H, W, C, K, R, S, stride, pad, ws=None, act=0):
        self._run("hifihr_conv2d_fwd", x, w, bias, act, y, N, H, W, C, K, R, S, stride, pad, ws, _nbytes(ws))

    def bias_relu_bwd(self, dy, y, M, C, g, db_acc):
        self._run("hifihr_bias_relu_bwd", dy, y, M, C, g, db_acc)

    def conv2d_fwd_bnstats(self, x, w, y, stats, N, H, W, C, K, R, S, stride, pad, ws=None):
        self._run("hifihr_conv2d_fwd_bnstats", x, w, y, stats, N, H, W, C, K, R, S, stride, pad, ws, _nbytes(ws))

    def conv2d_fwd_bnstats_pair_supported(self, N, H, W, C, stride, K1, R1, pad1, K2, R2, pad2):
        return bool(self._call("hifihr_conv2d_fwd_bnstats_pair_supported", N, H, W, C, stride, K1, R1, pad1, K2, R2, pad2))

    def conv2d_fwd_bnstats_pair(self, x, w1, y1, stats1, K1, R1, pad1, w2, y2, stats2, K2, R2, pad2, N, H, W, C, stride):
        """two convolutions of the same input (+ their batch-norm statistics) in one launch (include/hifihr.h)"""
        self._run("hifihr_conv2d_fwd_bnstats_pair", x, w1, y1, stats1, K1, R1, pad1, w2, y2, stats2, K2, R2, pad2, N, H, W, C, stride)

    def bn_stats_floats(self, C):
        return self._call("hifihr_bn_stats_floats", C)

    def bn_stats(self, x, M, C, stats):
        self._run("hifihr_bn_stats", x, M, C, stats)

    def bn_act_fwd(self, x, stats, gamma, beta, residual, act, M, C, eps, momentum, y, save_mean, save_invstd, rmean, rvar):
        self._run("hifihr_bn_act_fwd", x, stats, gamma, beta, residual, act, M, C, eps, momentum, y, save_mean, save_invstd, rmean, rvar)

    def bn_act_eval(self, x, rmean, rvar, gamma, beta, residual, act, M, C, eps, y):
        self._run("hifihr_bn_act_eval", x, rmean, rvar, gamma, beta, residual, act, M, C, eps, y)

    def bn_act_bwd(self, dy, y, x, save_mean, save_invstd, gamma, beta, act, M, C, red, dx, dres, dgamma_acc, dbeta_acc):
        self._run("hifihr_bn_act_bwd", dy, y, x, save_mean, save_invstd, gamma, beta, act, M, C, red, dx, dres, dgamma_acc, dbeta_acc)

    def bn_relu_maxpool_supported(self, N, H, W, C):
        return bool(self._call("hifihr_bn_relu_maxpool_supported", N, H, W, C))

    def bn_relu_maxpool_fwd(self, x, stats, gamma, beta, N, H, W, C, eps, momentum, pooled, tap, save_mean, save_invstd, running_mean,
                            running_var):
        self._run("hifihr_bn_relu_maxpool_fwd", x, stats, gamma, beta, N, H, W, C, eps, momentum, pooled, tap, save_mean, save_invstd,
                  running_mean, running_var)

    def bn_relu_maxpool_bwd_y(self, gy, pooled, tap, x, save_mean, save_invstd, gamma, beta, N, H, W, C, red, dx, dgamma_acc, dbeta_acc):
        self._run("hifihr_bn_relu_maxpool_bwd_y", gy, pooled, tap, x, save_mean, save_invstd, gamma, beta, N, H, W, C, red, dx, dgamma_acc,
                  dbeta_acc)

    def bn_relu_maxpool_bwd(self, gy, tap, x, save_mean, save_invstd, gamma, beta, N, H, W, C, red, dx, dgamma_acc, dbeta_acc):
        self._run("hifihr_bn_relu_maxpool_bwd", gy, tap, x, save_mean, save_invstd, gamma, beta, N, H, W, C, red, dx, dgamma_acc, dbeta_acc)

    def conv2d_bwd_weight_c3_supported(self, N, H, W, K, R, S, stride, pad):
        return bool(self._call("hifihr_conv2d_bwd_weight_c3_supported", N, H, W, K, R, S, stride, pad))

    def conv2d_bwd_weight_c3(self, x4, dy, dw3, N, H, W, K, R, S, stride, pad, ws):
        self._run("hifihr_conv2d_bwd_weight_c3", x4, dy, dw3, N, H, W, K, R, S, stride, pad, ws, _nbytes(ws))

    def dwconv2d_fwd(self, x, w, y, N, H, W, C, OH, OW, K, stride, pt, pl, stats=None):
        self._run("hifihr_dwconv2d_fwd", x, w, y, stats, N, H, W, C, OH, OW, K, stride, pt, pl)

    def dwconv2d_fwd_bnswish(self, x, mean, invstd, gamma, beta, w, y, N, H, W, C, OH, OW, K, stride, pt, pl, stats=None):
        self._run("hifihr_dwconv2d_fwd_bnswish", x, mean, invstd, gamma, beta, w, y, stats, N, H, W, C, OH, OW, K, stride, pt, pl)

    def dwconv2d_bwd_weight_bnswish(self, x, mean, invstd, gamma, beta, dy, dw, N, H, W, C, OH, OW, K, stride, pt, pl):
        self._run("hifihr_dwconv2d_bwd_weight_bnswish", x, mean, invstd, gamma, beta, dy, dw, N, H, W, C, OH, OW, K, stride, pt, pl)

    def bn_finalize_fwd(self, stats, M, C, eps, momentum, save_mean, save_invstd, rmean, rvar):
        self._run("hifihr_bn_finalize_fwd", stats, M, C, eps, momentum, save_mean, save_invstd, rmean, rvar)

    def dwconv2d_bwd_data(self, dy, w, dx, N, H, W, C, OH, OW, K, stride, pt, pl):
        self._run("hifihr_dwconv2d_bwd_data", dy, w, dx, N, H, W, C, OH, OW, K, stride, pt, pl)

    def dwconv2d_bwd_weight(self, x, dy, dw, N, H, W, C, OH, OW, K, stride, pt, pl):
        self._run("hifihr_dwconv2d_bwd_weight", x, dy, dw, N, H, W, C, OH, OW, K, stride, pt, pl)

    def light_split_fwd(self, lights, colors, directions):
        self._run("hifihr_light_split_fwd", lights, lights.shape[0], colors, directions)

    def light_split_bwd(self, lights, gcolors, gdirections, glights):
        self._run("hifihr_light_split_bwd", lights, gcolors, gdirections, lights.shape[0], glights)

    def loss_total_fwd(self, parts, counts, total):
        n = len(parts)
        self._run("hifihr_loss_total_fwd", _fp_table(parts), (c_int * n)(*[int(c) for c in counts]), n, total)

    def loss_total_bwd(self, gtotal, grads, counts):
        n = len(grads)
        self._run("hifihr_loss_total_bwd", gtotal, _fp_table(grads), (c_int * n)(*[int(c) for c in counts]), (c_int * n)(*[int(t.numel()) for t in grads]), n)

    def joint_terms_fwd(self, j2d, j2d_gt, joints, joints_gt, mse, lam3, out):
        ref = j2d if j2d is not None else joints
        self._run("hifihr_joint_terms_fwd", j2d, j2d_gt, joints, joints_gt, ref.shape[0], ref.shape[1], mse, _floats(lam3, 3), out)

    def joint_terms_bwd(self, j2d, j2d_gt, joints, joints_gt, mse, lam3, gout, g_j2d, g_joints):
        ref = j2d if j2d is not None else joints
        self._run("hifihr_joint_terms_bwd", j2d, j2d_gt, joints, joints_gt, ref.shape[0], ref.shape[1], mse, _floats(lam3, 3), gout, g_j2d,
                  g_joints)

    def open2d_terms_fwd(self, j2d, open_2dj, open_2dj_con, lam3, out):
        """out[3] = lambda-weighted (open_2dj, open_bone_direc, open_2dj_de); open_2dj_con [B,21] or [B,21,1], contiguous."""
        B, J = j2d.shape[0], j2d.shape[1]
        assert open_2dj.shape == j2d.shape and open_2dj_con.numel() == B * J and open_2dj_con.is_contiguous(), (j2d.shape, open_2dj_con.shape)
        self._run("hifihr_open2d_terms_fwd", j2d, open_2dj, open_2dj_con, B, J, _floats(lam3, 3), out)

    def open2d_terms_bwd(self, j2d, open_2dj, open_2dj_con, lam3, gout, g_j2d):
        B, J = j2d.shape[0], j2d.shape[1]
        assert open_2dj.shape == j2d.shape and open_2dj_con.numel() == B * J and open_2dj_con.is_contiguous(), (j2d.shape, open_2dj_con.shape)
        self._run("hifihr_open2d_terms_bwd", j2d, open_2dj, open_2dj_con, B, J, _floats(lam3, 3), gout, g_j2d)

    def geom_loss_fwd(self, joints, joints_gt, verts, verts_gt, shape, pose, faces, mse, lam, partial, out):
        B, J, V = joints.shape[0], joints.shape[1], verts.shape[1]
        F = 0 if faces is None else faces.shape[0]
        NS = 0 if shape is None else shape.shape[1]
        NP = 0 if pose is None else pose.shape[1]
        self._run("hifihr_geom_loss_fwd", joints, joints_gt, verts, verts_gt, shape, pose, faces, B, J, V, F, NS, NP, mse, _floats(lam, 5),
                  partial, out)

    def geom_loss_bwd(self, joints, joints_gt, verts, verts_gt, shape, pose, faces, vf_off, vf_idx, mse, lam, gout, gj, gv, gshape,
                      gpose):
        B, J, V = joints.shape[0], joints.shape[1], verts.shape[1]
        F = 0 if faces is None else faces.shape[0]
        NS = 0 if shape is None else shape.shape[1]
        NP = 0 if pose is None else pose.shape[1]
        self._run("hifihr_geom_loss_bwd", joints, joints_gt, verts, verts_gt, shape, pose, faces, vf_off, vf_idx, B, J, V, F, NS, NP, mse,
                  _floats(lam, 5), gout, gj, gv, gshape, gpose)

    def photo_loss_partial_floats(self):
        return self._call("hifihr_photo_loss_partial_floats")

    def photo_loss_fwd(self, rgba, imgs, seg, l_tex, l_mrgb, l_sil, re_img_m, mask_rgbs, partial, out):
        B, _, H, W = rgba.shape
        assert seg.dtype == torch.int64 and seg.is_contiguous() and rgba.is_contiguous() and imgs.is_contiguous()
        self._run("hifihr_photo_loss_fwd", rgba, imgs, seg, B, H, W, l_tex, l_mrgb, l_sil, re_img_m, mask_rgbs, partial, out)

    def photo_loss_bwd(self, rgba, re_img_m, mask_rgbs, g_re_img, gout, fwd_out, l_tex, l_mrgb, grad_rgba):
        B, _, H, W = rgba.shape
        self._run("hifihr_photo_loss_bwd", rgba, re_img_m, mask_rgbs, g_re_img, gout, fwd_out, B, H, W, l_tex, l_mrgb, grad_rgba)

    def sil_post(self, rgba, imgs, re_sil, mask_rgbs):
        B, _, H, W = rgba.shape
        assert rgba.is_contiguous() and (imgs is None or imgs.is_contiguous())
        self._run("hifihr_sil_post", rgba, imgs, B, H, W, re_sil, mask_rgbs)

    # ---- Winograd F(2x2, 3x3) ------------------------------------------
    # Winograd: m = output-tile edge (2: F(2x2, 3x3), 16 positions; 4: F(4x4, 3x3), 36 positions); wino_tile() = the library's choice
    def wino_tile(self, N, H, W, C, K):
        return self._call("hifihr_wino_tile", N, H, W, C, K)

    def wino_gemm_workspace_bytes(self, N, H, W, C, K, m=2):
        return self._call("hifihr_wino_gemm_workspace_bytes", N, H, W, C, K, m)

    def wino4_bwd_gemm_pair_supported(self, N, H, W, C, K):
        key = (N, H, W, C, K)
        hit = self._pair_ok.get(key)
        if hit is None:
            hit = self._pair_ok[key] = bool(self._call("hifihr_wino4_bwd_gemm_pair_supported", N, H, W, C, K))
        return hit

    def wino4_bwd_gemm_pair(self, V2, U2, M2, Vx, Yt, dU_parts, N, H, W, C, K, parts):
        """Backward-data and backward-weight products of one F(4x4, 3x3) layer (C -> K channels) in one launch."""
        self._run("hifihr_wino4_bwd_gemm_pair", V2, U2, M2, Vx, Yt, dU_parts, N, H, W, C, K, parts)

    def wino_weight_transform(self, w, U, K, C, flip, m=2):
        self._run("hifihr_wino_weight_transform", w, U, K, C, flip, m)

    def wino_input_transform(self, x, V, N, H, W, C, m=2):
        self._run("hifihr_wino_input_transform", x, V, N, H, W, C, m)

    def zero_page_ready(self, device=None):
        """The 256 zero bytes the halo / Winograd kernels read out-of-image pixels from exist on `device` (allocated at the first call
        OUTSIDE a stream capture; the steppers call this before they capture).  A positive answer is cached per device."""
        idx = torch.cuda.current_device() if device is None else torch.device(device).index
        idx = torch.cuda.current_device() if idx is None else idx
        if idx in self._zero_page:
            return True
        with torch.cuda.device(idx):
            ok = bool(self._call("hifihr_zero_page_ready", stream=torch.cuda.current_stream(idx).cuda_stream))
        if ok:
            self._zero_page.add(idx)
        return ok

    def conv3x3_c64_wino_supported(self, N, H, W, C, K):
        return bool(self._call("hifihr_conv3x3_c64_wino_supported", N, H, W, C, K))

    def conv3x3_c64_wino(self, x, U, bias, relu, y, stats, N, H, W):
        """64 -> 64 channel 3x3 / stride 1 / pad 1 convolution as register-resident Winograd F(2x2, 3x3) (include/hifihr.h)."""
        self._run("hifihr_conv3x3_c64_wino", x, U, bias, bool(relu), y, stats, N, H, W)

    def conv3x3_c64_wino_res(self, x, U, res, y, N, H, W):
        """conv3x3_c64_wino with y = product + res (backward-data + the gradient of the input's other consumer; include/hifihr.h)."""
        self._run("hifihr_conv3x3_c64_wino_res", x, U, res, y, N, H, W)

    def conv3x3_c64_bwd_pair_supported(self, N, H, W):
        return bool(self._call("hifihr_conv3x3_c64_bwd_pair_supported", N, H, W))

    def conv3x3_c64_bwd_pair(self, dy, U_bwd, res, dx, x, dw, N, H, W, ws=None):
        """dx = conv3x3_c64_wino[_res](dy, U_bwd[, res]) and dw += conv2d_bwd_weight(x, dy) in ONE launch + the slab sum (include/hifihr.h)."""
        self._run("hifihr_conv3x3_c64_bwd_pair", dy, U_bwd, res, dx, x, dw, ws, _nbytes(ws), N, H, W)

    def conv3x3_c64_bwd_pair_slabs(self, dy, U_bwd, res, dx, x, slabs, N, H, W):
        """hifihr_conv3x3_c64_bwd_pair without its slab sum: -> number of weight-gradient slabs left in `slabs` (hifihr_conv_halo_wgrad_reduce_multi)."""
        n = c_int32(0)
        self._run("hifihr_conv3x3_c64_bwd_pair_slabs", dy, U_bwd, res, dx, x, slabs, _nbytes(slabs), N, H, W, ctypes.byref(n))
        return n.value

    def conv_halo_wgrad_reduce_multi(self, jobs):
        """jobs: [(slabs tensor, nslab, dw_acc tensor)] -- the slab sums of several 64 -> 64 layers in one launch."""
        raw = b"".join(struct.pack("<QQii", sl.data_ptr(), dw.data_ptr(), int(n), 0) for sl, n, dw in jobs)
        buf = ctypes.create_string_buffer(raw, len(raw))
        self._run("hifihr_conv_halo_wgrad_reduce_multi", ctypes.cast(buf, c_void_p), len(jobs), stream=jobs[0][0])

    def wino_bn_input_supported(self, C, m):
        return bool(self._call("hifihr_wino_bn_input_supported", C, m))

    def wino_bn_input_transform(self, x, stats, gamma, beta, residual, out, V, N, H, W, C, m, eps, momentum, save_mean, save_invstd,
                                running_mean, running_var):
        self._run("hifihr_wino_bn_input_transform", x, stats, gamma, beta, residual, out, V, N, H, W, C, m, eps, momentum, save_mean,
                  save_invstd, running_mean, running_var)

    def wino_output_transform_bnred(self, Mm, x, out, gadd, save_mean, save_invstd, gamma, beta, red, g, N, H, W, C, m):
        self._run("hifihr_wino_output_transform_bnred", Mm, x, out, gadd, save_mean, save_invstd, gamma, beta, red, g, N, H, W, C, m)

    def wino_bn_bwd_dual_transform(self, g, y, save_mean, save_invstd, gamma, red, V, Yt, N, H, W, K, m, dgamma_acc, dbeta_acc):
        self._run("hifihr_wino_bn_bwd_dual_transform", g, y, save_mean, save_invstd, gamma, red, V, Yt, N, H, W, K, m, dgamma_acc, dbeta_acc)

    def bn_bwd_apply(self, g, x, save_mean, save_invstd, gamma, M, C, red, dx, dgamma_acc, dbeta_acc):
        self._run("hifihr_bn_bwd_apply", g, x, save_mean, save_invstd, gamma, M, C, red, dx, dgamma_acc, dbeta_acc)

    def wino_gemm(self, V, U, M, N, H, W, C, K, ws=None, m=2):
        self._run("hifihr_wino_gemm", V, U, M, N, H, W, C, K, m, ws, _nbytes(ws))

    def wino_input_dy_transform(self, dy, V, Yt, N, H, W, K, m=2):
        self._run("hifihr_wino_input_dy_transform", dy, V, Yt, N, H, W, K, m)

    def conv2d_bwd_data_pre(self, dy, wt, dx, N, H, W, C, K, R, S, stride, pad, ws=None):
        self._run("hifihr_conv2d_bwd_data_pre", dy, wt, dx, N, H, W, C, K, R, S, stride, pad, ws, _nbytes(ws))

    def conv2d_bwd_data_pre_res(self, dy, wt, res, dx, N, H, W, C, K, R, S, stride, pad, ws=None):
        """conv2d_bwd_data_pre with dx = product + res (include/hifihr.h)."""
        self._run("hifihr_conv2d_bwd_data_pre_res", dy, wt, res, dx, N, H, W, C, K, R, S, stride, pad, ws, _nbytes(ws))

    def conv2d_bwd_data_pre_plus1x1_supported(self, N, H, W, C, K, R, S, stride, pad):
        return bool(self._call("hifihr_conv2d_bwd_data_pre_plus1x1_supported", N, H, W, C, K, R, S, stride, pad))

    def conv2d_bwd_data_pre_plus1x1(self, dy, wt, dy2, wt2, dx, N, H, W, C, K, R, S, stride, pad):
        """dx = backward-data of the strided convolution (dy, wt) + backward-data of a 1x1 / same stride / pad 0 convolution of the same input
        (dy2 [N][OH][OW][K], wt2 [C][K]) in one launch (include/hifihr.h)."""
        self._run("hifihr_conv2d_bwd_data_pre_plus1x1", dy, wt, dy2, wt2, dx, N, H, W, C, K, R, S, stride, pad)

    def conv2d_bwd_weight_plus1x1_supported(self, N, H, W, C, K, R, S, stride, pad):
        return bool(self._call("hifihr_conv2d_bwd_weight_plus1x1_supported", N, H, W, C, K, R, S, stride, pad))

    def conv2d_bwd_weight_plus1x1(self, x, dy, dw, dy2, dw2, N, H, W, C, K, R, S, stride, pad):
        """dw += weight gradient of the strided convolution, dw2 += that of the 1x1 / same stride / pad 0 convolution of the same input, one launch."""
        self._run("hifihr_conv2d_bwd_weight_plus1x1", x, dy, dw, dy2, dw2, N, H, W, C, K, R, S, stride, pad)

    @staticmethod
    def prep_jobs(jobs, device):
        """[(src tensor, dst tensor, K, C, RS, kind)] -> device table of hifihr_prep_job (two pointers + four ints = 32 bytes)."""
        raw = b"".join(struct.pack("<QQiiii", s.data_ptr(), d.data_ptr(), K, C, RS, kind) for s, d, K, C, RS, kind in jobs)
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)

    def weight_prep(self, table, njobs, blocks_per_job=64):
        self._run("hifihr_weight_prep", table, njobs, blocks_per_job)

    def freihand_batch(self, img_rgbx, mask, Ks, joints, verts, scales, packed, B, out, root_id=None, image_size=None):
        """out: dict with any of imgs, masks, segms_gt, Ks, Ps, joints, verts, j2d_gt, scales, idxs (device tensors, contiguous);
        root_id given: also root_xyz [B,1,3], joints_rel, verts_rel, cam_ndc [B,4] (hifihr_freihand_batch_step)."""
        n, H, W = img_rgbx.shape
        J, V = joints.shape[1], verts.shape[1]
        g = out.get
        for k in ("segms_gt", "idxs"):
            assert g(k) is None or g(k).dtype == torch.int64
        for t in out.values():
            assert t.is_contiguous()
        batch = (img_rgbx, mask, Ks, joints, verts, scales, J, V, packed, B, H, W, g("imgs"), g("masks"), g("segms_gt"), g("Ks"), g("Ps"),
                 g("joints"), g("verts"), g("j2d_gt"), g("scales"), g("idxs"))
        if root_id is None:
            self._run("hifihr_freihand_batch", *batch)
            return
        # + the terms every training iteration derives from the batch: root_xyz, root-relative ground truth, the NDC camera
        self._run("hifihr_freihand_batch_step", *batch, root_id, image_size or H, g("root_xyz"), g("joints_rel"), g("verts_rel"), g("cam_ndc"))

    def freihand_keypoints(self, open_2dj, open_2dj_con, idx, total, j2d_gt, semi_below, out_open_2dj, out_con, out_texture_con):
        """The detections of a batch (hifihr_freihand_keypoints): cache open_2dj [n,21,2] / open_2dj_con [n,21] or [n,21,1], idx int32 [B],
        total [B,3,3]; j2d_gt [B,21,2] with semi_below > 0.  Outputs [B,21,2], [B,21] or [B,21,1], [B]; any may be None."""
        n, B = open_2dj.shape[0], idx.shape[0]
        assert open_2dj.shape[1:] == (21, 2) and open_2dj_con.numel() == n * 21 and total.numel() == 9 * B, (open_2dj.shape, open_2dj_con.shape)
        for t, numel in ((out_open_2dj, B * 42), (out_con, B * 21), (out_texture_con, B), (j2d_gt, B * 42)):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.numel() == numel)
        self._run("hifihr_freihand_keypoints", open_2dj, open_2dj_con, n, idx, total, j2d_gt, semi_below, B, out_open_2dj, out_con,
                  out_texture_con)

    def ho3d_workspace_bytes(self, B, out_size):
        return self._call("hifihr_ho3d_workspace_bytes", B, out_size)

    def ho3d_batch(self, img_rgbx, hand_mask, Ks, uv21, xyz21, packed, B, out_size, ws, out):
        """out: dict with any of img_crop [B,3,S,S], hand_mask_crop [B,1,S,S], K_crop [B,3,3], uv21_crop [B,21,2], xyz21 [B,21,3]."""
        n, FH, FW = img_rgbx.shape
        g = out.get
        for t in out.values():
            assert t.is_contiguous() and t.dtype == torch.float32
        self._run("hifihr_ho3d_batch", img_rgbx, hand_mask, Ks, uv21, xyz21, FH, FW, packed, B, out_size, ws, _nbytes(ws), g("img_crop"),
                  g("hand_mask_crop"), g("K_crop"), g("uv21_crop"), g("xyz21"))

    def ho3d_keypoints(self, open_2dj, open_2dj_con, packed, B, out_size, out_open_2dj, out_con):
        """The detections of an HO-3D batch through its crop window (hifihr_ho3d_keypoints): cache open_2dj [n,21,2] / open_2dj_con [n,21] or
        [n,21,1], packed = hifihr_ho3d_batch's.  Outputs [B,21,2], [B,21] or [B,21,1]; either may be None."""
        n = open_2dj.shape[0]
        assert open_2dj.shape[1:] == (21, 2) and open_2dj_con.numel() == n * 21 and packed.numel() >= 8 * B, (open_2dj.shape, open_2dj_con.shape)
        for t, numel in ((out_open_2dj, B * 42), (out_con, B * 21)):
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.numel() == numel)
        self._run("hifihr_ho3d_keypoints", open_2dj, open_2dj_con, n, packed, B, out_size, out_open_2dj, out_con)

    def ho3d_depth_crop(self, depth_u16, packed, B, out_size, depth_scale, out_depth):
        """The metric depth of an HO-3D batch through its crop box (hifihr_ho3d_depth_crop): cache depth_u16 [n,FH,FW] (uint16, or int16
        holding the same bits), packed = hifihr_ho3d_batch's; out_depth fp32 [B,S,S]."""
        n, FH, FW = depth_u16.shape
        assert depth_u16.element_size() == 2 and not depth_u16.is_floating_point() and packed.numel() >= 8 * B, depth_u16.dtype
        assert out_depth.dtype == torch.float32 and tuple(out_depth.shape) == (B, out_size, out_size)
        self._run("hifihr_ho3d_depth_crop", depth_u16, n, FH, FW, packed, B, out_size, depth_scale, out_depth)

    def depth_points(self, depths, K, mask, draws, origin, points, count, index=None):
        """hifihr_depth_points: depths fp32 [B,H,W], K [B,3,3], mask [B,H,W] float32 / int64 or None, draws [B,P], origin [B,3] or None;
        points fp32 [B,P,3], count int32 [B], index int32 [B,P] or None."""
        B, H, W = depths.shape
        P = draws.shape[1]
        assert tuple(K.shape) == (B, 3, 3) and tuple(draws.shape) == (B, P) and tuple(points.shape) == (B, P, 3) and tuple(count.shape) == (B,)
        assert mask is None or (mask.dtype in (torch.float32, torch.int64) and mask.numel() == B * H * W), None if mask is None else (mask.dtype, mask.shape)
        assert origin is None or origin.numel() == B * 3
        assert index is None or tuple(index.shape) == (B, P)
        self._run("hifihr_depth_points", depths, K, mask, int(mask is not None and mask.dtype == torch.int64), draws, origin, B, H, W, P, points,
                  count, index)

    def freihand_augment(self, img_rgbx, mask, idx, coef_fix, out_img, out_mask):
        """img_rgbx int32/uint8x4 [n,H,W], mask uint8 [n,H,W] (either None with its output), idx int32 [B], coef_fix int32 [B,6]."""
        ref = img_rgbx if img_rgbx is not None else mask
        self._run("hifihr_freihand_augment", img_rgbx, mask, idx, coef_fix, idx.shape[0], ref.shape[1], ref.shape[2], out_img, out_mask)

    def procrustes_error(self, pred, gt, aligned, err_sum):
        self._run("hifihr_procrustes_error", pred, gt, pred.shape[0], pred.shape[1], aligned, err_sum)

    def point_error_hist(self, pred, gt, vis, thresholds, hist, sum_d):
        """pred / gt fp32 [n,K,3], vis uint8 [n,K] or None, thresholds: T host float64 values; hist int32 [K,T+1], sum_d float64 [K]."""
        (thr, thr_p), n, K = _host_f64(thresholds), pred.shape[0], pred.shape[1]
        assert vis is None or (vis.dtype == torch.uint8 and vis.is_contiguous() and tuple(vis.shape) == (n, K))
        assert sum_d.dtype == torch.float64 and sum_d.is_contiguous() and tuple(hist.shape) == (K, len(thr) + 1) and tuple(sum_d.shape) == (K,)
        self._run("hifihr_point_error_hist", pred, gt, vis, n, K, thr_p, len(thr), hist, sum_d)

    def fscore_counts(self, pred, gt, thresholds, counts):
        """pred fp32 [B,Np,3], gt fp32 [B,Ng,3], thresholds: T host float64 values; counts int32 [B,2,T]."""
        (thr, thr_p), B = _host_f64(thresholds), pred.shape[0]
        assert gt.shape[0] == B and tuple(counts.shape) == (B, 2, len(thr))
        self._run("hifihr_fscore_counts", pred, gt, B, pred.shape[1], gt.shape[1], thr_p, len(thr), counts)

    def wino_output_transform(self, M, y, stats, N, H, W, K, bias=None, act=0, m=2, mask=None):
        if mask is not None:
            assert stats is None and bias is None and not act and m == 4
            self._run("hifihr_wino_output_transform_mask", M, y, mask, N, H, W, K, m)
        elif bias is not None or act:
            assert stats is None
            self._run("hifihr_wino_output_transform_act", M, y, bias, act, N, H, W, K, m)
        else:
            self._run("hifihr_wino_output_transform", M, y, stats, N, H, W, K, m)

    def wino_dy_transform(self, dy, Y, N, H, W, K, m=2):
        self._run("hifihr_wino_dy_transform", dy, Y, N, H, W, K, m)

    def wino_wgrad_gemm(self, V, Y, dU_zeroed, N, H, W, C, K):
        self._run("hifihr_wino_wgrad_gemm", V, Y, dU_zeroed, N, H, W, C, K)

    def wino_dw_transform(self, dU, dw_acc, K, C, clear=True):
        self._run("hifihr_wino_dw_transform", dU, dw_acc, K, C, bool(clear))

    def bgemm_nt_workspace_bytes(self, M, N, K, batch):
        return self._call("hifihr_bgemm_nt_workspace_bytes", M, N, K, batch)

    def bgemm_nt(self, A, B, C, M, N, K, batch, ws=None):
        self._run("hifihr_bgemm_nt", A, B, C, M, N, K, batch, ws, _nbytes(ws))

    # ---- RCCL wrapper (csrc/comm.hip); torch.distributed drives the exchange in this package, these bindings serve tests / other hosts
    def _comm(self, entry, *args):
        if self._call(entry, *args) != 0:
            raise HifihrError(f"{entry}: " + (self.c.hifihr_comm_last_error() or b"").decode())

    def comm_unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        self._comm("hifihr_comm_get_unique_id", buf)
        return buf.raw

    def comm_init(self, rank, world, uid: bytes):
        h = c_void_p()
        self._comm("hifihr_comm_init", ctypes.byref(h), rank, world, ctypes.create_string_buffer(uid, 128))
        return h

    def comm_allreduce(self, h, buf):
        self._comm("hifihr_comm_allreduce_f32", h, buf, buf.numel())

    def comm_broadcast(self, h, buf, root=0):
        self._comm("hifihr_comm_broadcast_f32", h, buf, buf.numel(), root)

    def comm_destroy(self, h):
        self._call("hifihr_comm_destroy", h)

    def conv2d_describe(self, N, H, W, C, K, R, S, stride, pad, direction):
        """direction: 0 / False forward, 1 / True backward-data, 2 backward-weight."""
        buf = ctypes.create_string_buffer(64)
        self._run("hifihr_conv2d_describe", N, H, W, C, K, R, S, stride, pad, direction, buf, 64)
        return buf.value.decode()

    def bgemm_describe(self, tn, M, N, K, batch=16):
        buf = ctypes.create_string_buffer(96)
        self._run("hifihr_bgemm_describe", bool(tn), M, N, K, batch, buf, 96)
        return buf.value.decode()

    def bgemm_tn_parts(self, M, N, T, batch):
        return self._call("hifihr_bgemm_tn_parts", M, N, T, batch)

    def bgemm_tn_coherent(self, M, N, T, batch):
        return self._call("hifihr_bgemm_tn_coherent", M, N, T, batch)

    def bgemm_tn(self, A, B, Cparts, M, N, T, batch, parts):
        self._run("hifihr_bgemm_tn", A, B, Cparts, M, N, T, batch, parts)

    def wino_wgrad_parts(self, N, H, W, C, K, m=2):
        return self._call("hifihr_wino_wgrad_parts", N, H, W, C, K, m)

    def wino_wgrad_gemm_parts(self, V, Y, dU_parts, N, H, W, C, K, parts, m=2):
        self._run("hifihr_wino_wgrad_gemm_parts", V, Y, dU_parts, N, H, W, C, K, parts, m)

    def wino4_dw_transform_multi(self, jobs):
        """jobs: [(dU_parts tensor, parts, dw_acc tensor, K, C)] -- the F(4x4) weight-gradient transforms of several layers in one launch
        (hifihr_wino4_dw_transform_multi: a host array of hifihr_wino_dw_job, 32 bytes each, passed in the kernel arguments)."""
        raw = b"".join(struct.pack("<QQiiii", du.data_ptr(), dw.data_ptr(), int(parts), int(K), int(C), 0) for du, parts, dw, K, C in jobs)
        buf = ctypes.create_string_buffer(raw, len(raw))
        self._run("hifihr_wino4_dw_transform_multi", ctypes.cast(buf, c_void_p), len(jobs), stream=jobs[0][0])

    def wino_dw_transform_parts(self, dU_parts, parts, dw_acc, K, C, m=2):
        self._run("hifihr_wino_dw_transform_parts", dU_parts, parts, dw_acc, K, C, m)

    def weight_transpose(self, w, wt, K, RS, C):
        self._run("hifihr_weight_transpose", w, wt, K, RS, C)

    def se_pool(self, x, B, HW, C, mean_zeroed):
        self._run("hifihr_se_pool", x, B, HW, C, mean_zeroed)

    def se_scale(self, x, gate, add, add_scale, B, HW, C, y):
        self._run("hifihr_se_scale", x, gate, add, add_scale, B, HW, C, y)

    def drop_connect_add(self, x, skip, u, keep, B, per_sample, out):
        self._run("hifihr_drop_connect_add", x, skip, u, keep, B, per_sample, out)

    def wino_tiles(self, N, H, W, m):
        return self._call("hifihr_wino_tiles", N, H, W, m)

    def wino_tiles_computed(self, N, H, W, m):
        return self._call("hifihr_wino_tiles_computed", N, H, W, m)

    def se_mlp_supported(self, C, SQ):
        return bool(self._call("hifihr_se_mlp_supported", C, SQ))

    def se_mlp_fwd(self, mean_acc, w1, b1, w2t, b2, B, C, SQ, mean, z1, h1, gate):
        self._run("hifihr_se_mlp_fwd", mean_acc, w1, b1, w2t, b2, B, C, SQ, mean, z1, h1, gate)

    def se_mlp_bwd(self, dgate_acc, gate, z1, h1, mean, w1, w2t, B, C, SQ, dz2, dz1, dmean, dw1, db1, dw2, db2):
        self._run("hifihr_se_mlp_bwd", dgate_acc, gate, z1, h1, mean, w1, w2t, B, C, SQ, dz2, dz1, dmean, dw1, db1, dw2, db2)

    def se_bwd_gate(self, dy, x, B, HW, C, dgate_zeroed):
        self._run("hifihr_se_bwd_gate", dy, x, B, HW, C, dgate_zeroed)

    def linear_fwd(self, x, w, b, act, y, bn=None, z=None):
        """bn: None or (gamma, beta, eps, momentum, running_mean, running_var, z, save_mean, save_invstd); z: pre-activation
        buffer for act 2 (swish) without batch-norm."""
        B, I = x.shape
        O = w.shape[0]
        gamma, beta, eps, mom, rm, rv, z_bn, sm, si = bn if bn is not None else (None, None, 0.0, 0.0, None, None, None, None, None)
        z = z_bn if bn is not None else z
        self._run("hifihr_linear_fwd", x, w, b, B, I, O, act, gamma, beta, eps, mom, rm, rv, y, z, sm, si)

    def linear_bwd(self, dy, y, x, w, act, dz, dW_acc, db_acc, dx, bn=None, z=None):
        """bn: None or (gamma, z, save_mean, save_invstd, dgamma_acc, dbeta_acc); z: pre-activation of an act-2 layer."""
        B, I = x.shape
        O = w.shape[0]
        gamma, z_bn, sm, si, dg, dbt = bn if bn is not None else (None,) * 6
        z = z_bn if bn is not None else z
        self._run("hifihr_linear_bwd", dy, y, x, w, B, I, O, act, gamma, z, sm, si, dz, dW_acc, db_acc, dg, dbt, dx)

    @staticmethod
    def _descs(members):
        """members: list of dicts with tensors x, w, b, y and act (+ dy, dz, dW, db, dx for the backward) -> ctypes array."""
        arr = (_LinearDesc * len(members))()
        p = lambda t: None if t is None else t.data_ptr()
        for d, m in zip(arr, members):
            d.x, d.w, d.b, d.y = p(m["x"]), p(m["w"]), p(m.get("b")), p(m["y"])
            d.B, d.I, d.O, d.act = m["x"].shape[0], m["x"].shape[1], m["w"].shape[0], int(m["act"])
            d.dy, d.dz_scratch, d.dW_acc, d.db_acc, d.dx = p(m.get("dy")), p(m.get("dz")), p(m.get("dW")), p(m.get("db")), p(m.get("dx"))
        return arr

    def linear_fwd_group(self, members):
        self._run("hifihr_linear_fwd_group", self._descs(members), len(members), stream=members[0]["x"])

    def linear_bwd_group(self, members):
        self._run("hifihr_linear_bwd_group", self._descs(members), len(members), stream=members[0]["x"])

    def mmpool_fwd(self, x, p, B, HW, C, y, argmax, xmax, xavg):
        self._run("hifihr_mmpool_fwd", x, p, B, HW, C, y, argmax, xmax, xavg)

    def mmpool_bwd(self, gy, p, argmax, xmax, xavg, B, HW, C, dx, dp_acc):
        self._run("hifihr_mmpool_bwd", gy, p, argmax, xmax, xavg, B, HW, C, dx, dp_acc)

    def maxpool2d_fwd(self, x, N, H, W, C, k, s, p, y, tap):
        assert tap.dtype == torch.uint8
        self._run("hifihr_maxpool2d_fwd", x, N, H, W, C, k, s, p, y, tap)

    def maxpool2d_fwd_flat(self, x, N, H, W, C, k, s, p, y_flat, tap):
        """maxpool2d_fwd with the output as the [N, C * OH * OW] matrix of `y.view(N, -1)` (NCHW order; include/hifihr.h)."""
        self._run("hifihr_maxpool2d_fwd_flat", x, N, H, W, C, k, s, p, y_flat, tap)

    def maxpool2d_bwd_flat(self, gy_flat, tap, N, H, W, C, k, s, p, dx):
        self._run("hifihr_maxpool2d_bwd_flat", gy_flat, tap, N, H, W, C, k, s, p, dx)

    def maxpool2d_bwd(self, gy, tap, N, H, W, C, k, s, p, dx, relu_y=None):
        if relu_y is not None:
            self._run("hifihr_maxpool2d_bwd_relu", gy, tap, relu_y, N, H, W, C, k, s, p, dx)
        else:
            self._run("hifihr_maxpool2d_bwd", gy, tap, N, H, W, C, k, s, p, dx)

    def conv2d_bwd_data(self, dy, w, dx, scratch, N, H, W, C, K, R, S, stride, pad, ws=None):
        self._run("hifihr_conv2d_bwd_data", dy, w, dx, scratch, N, H, W, C, K, R, S, stride, pad, ws, _nbytes(ws))

    def conv2d_wgrad_workspace_bytes(self, N, H, W, C, K, R, S, stride, pad):
        return self._call("hifihr_conv2d_wgrad_workspace_bytes", N, H, W, C, K, R, S, stride, pad)

    def conv2d_bwd_weight(self, x, dy, dw, N, H, W, C, K, R, S, stride, pad, ws=None):
        self._run("hifihr_conv2d_bwd_weight_ws", x, dy, dw, N, H, W, C, K, R, S, stride, pad, ws, _nbytes(ws))

    def image_to_nhwc4(self, images, out):
        B, _, H, W = images.shape
        self._run("hifihr_image_to_nhwc4", images, out, B, H, W)

    def image_to_nhwc4_padded(self, images, out, pad4, normalize):
        """pad4 = (left, right, top, bottom) like F.pad."""
        B, _, H, W = images.shape
        pl, pr, pt, pb = pad4
        self._run("hifihr_image_to_nhwc4_padded", images, out, B, H, W, pt, pl, pb, pr, bool(normalize))

    # ---- LPIPS (csrc/lpips.hip) -----------------------------------------
    def image_scale_to_nhwc4(self, images, out, shift3, scale3):
        """out[B, H, W, 4] = ((images - shift[c]) / scale[c], 0); shift3 / scale3: three Python floats each (the package's ScalingLayer)."""
        B, _, H, W = images.shape
        self._run("hifihr_image_scale_to_nhwc4", images, out, B, H, W, _floats(shift3, 3), _floats(scale3, 3))

    def maxpool2d_fwd_notap(self, x, N, H, W, C, k, s, p, y):
        self._run("hifihr_maxpool2d_fwd_notap", x, N, H, W, C, k, s, p, y)

    def lpips_tap_max_channels(self):
        return self._call("hifihr_lpips_tap_max_channels")

    def lpips_tap_partial_floats(self, B):
        return self._call("hifihr_lpips_tap_partial_floats", B)

    def lpips_tap(self, f0, f1, w, B, HW, C, partial, val, accumulate=False):
        """val[b] (+)= mean over pixels of sum_c w_c (n0_c - n1_c)^2 on two channels-last maps [B][HW][C] (include/hifihr.h)."""
        self._run("hifihr_lpips_tap", f0, f1, w, B, HW, C, bool(accumulate), partial, val)

    def lpips_tap_bwd(self, f0, f1, w, gval, B, HW, C, gf0, accumulate=False, relu=False):
        """gf0[b] (+)= gval[b] / HW * d tap / d f0 on two channels-last maps [B][HW][C]; f1 is the target (include/hifihr.h).
        relu: f0 is a ReLU's output and the stored sum is multiplied by [f0 > 0] (hifihr_lpips_tap_bwd_relu)."""
        self._run("hifihr_lpips_tap_bwd_relu" if relu else "hifihr_lpips_tap_bwd", f0, f1, w, gval, B, HW, C, bool(accumulate), gf0)

    def lpips_maxpool_fwd(self, x, N, H, W, C, y):
        """nn.MaxPool2d(3, 2): x[N, H, W, C] -> y[N, OH, OW, C]; tapless (the backward recomputes the winners from x)."""
        self._run("hifihr_lpips_maxpool_fwd", x, N, H, W, C, y)

    def lpips_maxpool_bwd(self, gy, x, N, H, W, C, dx):
        """dx[N, H, W, C] (overwritten) from gy[N, OH, OW, C] and the pool's saved input x: a gather, first maximum wins."""
        self._run("hifihr_lpips_maxpool_bwd", gy, x, N, H, W, C, dx)

    def image_scale_to_nhwc4_bwd(self, g4, gimg, scale3):
        """gimg[B, 3, H, W] = g4[B, H, W, :3] / scale[c]: the backward of image_scale_to_nhwc4."""
        B, _, H, W = gimg.shape
        self._run("hifihr_image_scale_to_nhwc4_bwd", g4, gimg, B, H, W, _floats(scale3, 3))

    # ---- SSIM ----------------------------------------------------------
    def ssim_partial_count(self, planes, H, W):
        return self._call("hifihr_ssim_partial_count", planes, H, W)

    def ssim_fwd(self, window, img1, img2, partial, dA, dB, dC):
        planes, H, W = img1.shape[0] * img1.shape[1], img1.shape[2], img1.shape[3]
        self._run("hifihr_ssim_fwd", window, img1, img2, planes, H, W, partial, dA, dB, dC)

    def ssim_finish(self, partial, scale, offset, out):
        self._run("hifihr_ssim_finish", partial, partial.numel(), scale, offset, out)

    def ssim_bwd_scaled(self, window, img1, img2, dA, dB, dC, grad_out, out_scale, gimg1):
        planes, H, W = img1.shape[0] * img1.shape[1], img1.shape[2], img1.shape[3]
        self._run("hifihr_ssim_bwd_scaled", window, img1, img2, dA, dB, dC, grad_out, out_scale, planes, H, W, gimg1)

    def ssim_bwd(self, window, img1, img2, dA, dB, dC, grad_out, gimg1):
        planes, H, W = img1.shape[0] * img1.shape[1], img1.shape[2], img1.shape[3]
        self._run("hifihr_ssim_bwd", window, img1, img2, dA, dB, dC, grad_out, planes, H, W, gimg1)

    # ---- optimizer ---------------------------------------------------
    def adam_step(self, p, g, m, v, grad_scale, lr, beta1, beta2, eps, weight_decay, step):
        n = p.numel()
        assert g.numel() == n and m.numel() == n and v.numel() == n
        self._run("hifihr_adam_step", p, g, m, v, n, grad_scale, lr, beta1, beta2, eps, weight_decay, step)

    def adam_state_bytes(self):
        return self._call("hifihr_adam_state_bytes")

    @staticmethod
    def adam_state_image(lr, beta1, beta2, step):
        """The 48 bytes of hifihr_adam_step_counted's state (include/hifihr.h) as a uint8 CPU tensor:
        f64 lr, beta1, beta2, beta1^step, beta2^step, i32 step, i32 0."""
        b1, b2 = float(beta1), float(beta2)
        return torch.frombuffer(bytearray(struct.pack("<dddddii", float(lr), b1, b2, b1 ** int(step), b2 ** int(step), int(step), 0)),
                                dtype=torch.uint8).clone()

    def adam_step_counted(self, p, g, m, v, grad_scale, eps, weight_decay, state):
        assert state.dtype == torch.uint8 and state.numel() == self.adam_state_bytes() and state.device == p.device
        self._run("hifihr_adam_step_counted", p, g, m, v, p.numel(), grad_scale, eps, weight_decay, state)

    def adam_step_dyn(self, p, g, m, v, grad_scale, beta1, beta2, eps, weight_decay, dyn):
        self._run("hifihr_adam_step_dyn", p, g, m, v, p.numel(), grad_scale, beta1, beta2, eps, weight_decay, dyn)

    # ---- gradient guard (include/hifihr.h: hifihr_grad_norm / hifihr_adam_step_guarded) ----
    def grad_guard_bytes(self):
        return self._call("hifihr_grad_guard_bytes")

    def grad_norm_workspace_bytes(self, n):
        return self._call("hifihr_grad_norm_workspace_bytes", n)

    def grad_guard_alloc(self, n, device):
        """(guard block, workspace) for a flat gradient of n floats: uint8 tensors, the guard block zeroed once as the header asks."""
        guard = torch.zeros(self.grad_guard_bytes(), dtype=torch.uint8, device=device)
        ws = torch.zeros(self.grad_norm_workspace_bytes(n), dtype=torch.uint8, device=device)
        return guard, ws

    def grad_norm(self, g, grad_scale, max_norm, guard, ws):
        n = g.numel()
        assert guard.dtype == torch.uint8 and guard.numel() == self.grad_guard_bytes() and guard.device == g.device
        assert ws.dtype == torch.uint8 and ws.numel() >= self.grad_norm_workspace_bytes(n) and ws.device == g.device
        self._run("hifihr_grad_norm", g, n, grad_scale, max_norm, guard, ws)

    def adam_step_guarded(self, p, g, m, v, grad_scale, lr, beta1, beta2, eps, weight_decay, step, state, guard):
        """state None: the host-scalar form (lr, betas, step as hifihr_adam_step); a state tensor: the counted form (they are ignored)."""
        n = p.numel()
        assert g.numel() == n and m.numel() == n and v.numel() == n
        assert guard.dtype == torch.uint8 and guard.numel() == self.grad_guard_bytes() and guard.device == p.device
        if state is not None:
            assert state.dtype == torch.uint8 and state.numel() == self.adam_state_bytes() and state.device == p.device
        self._run("hifihr_adam_step_guarded", p, g, m, v, n, grad_scale, lr, beta1, beta2, eps, weight_decay, step, state, guard)

    @staticmethod
    def grad_guard_unpack(raw):
        """The 32 bytes of the guard block (include/hifihr.h) as a dict: norm, clip_coef, finite, steps, clipped, skipped."""
        norm, coef, finite, steps, clipped, skipped, _ = struct.unpack("<dfiiiii", bytes(raw))
        return {"norm": norm, "clip_coef": coef, "finite": bool(finite), "steps": steps, "clipped": clipped, "skipped": skipped}

    # ---- renderer ----------------------------------------------------
    def renderer_create(self, faces, V, image_size=224, aa=3, ambient=(0.5, 0.5, 0.5), mat_diffuse=(0.8, 0.8, 0.8),
                        specular=(0.04, 0.04, 0.04), shininess=30.0, background=(1.0, 1.0, 1.0)) -> c_void_p:
        f, f_p = _host_i32(faces)
        h = c_void_p()
        a, m, s, b = (_host_f32(x) for x in (ambient, mat_diffuse, specular, background))
        self._run("hifihr_renderer_create", ctypes.byref(h), f_p, V, f.shape[0], image_size, aa, a[1], m[1], s[1], shininess, b[1])
        return h

    def texture_pca_fwd(self, coef, basis, mean, out):
        B, K = coef.shape
        self._run("hifihr_texture_pca_fwd", coef, basis, mean, B, K, basis.shape[1], out)

    def texture_pca_bwd(self, gtex, basis, dcoef_zeroed):
        B, K = dcoef_zeroed.shape
        self._run("hifihr_texture_pca_bwd", gtex, basis, B, K, basis.shape[1], dcoef_zeroed)

    def renderer_set_light_mode(self, h, point_lights):
        self._run("hifihr_renderer_set_light_mode", h, bool(point_lights))

    def renderer_destroy(self, h):
        self._call("hifihr_renderer_destroy", h)

    def render_workspace_bytes(self, h, B) -> int:
        return self._call("hifihr_render_workspace_bytes", h, B)

    def render_fwd(self, h, verts, vcolors, cam, light_color, light_dir, rgba, face_id, ws):
        self._run("hifihr_render_fwd", h, verts, vcolors, vcolors.dim() == 3, cam, light_color, light_dir, verts.shape[0], rgba, face_id, ws)

    def renderer_set_uv(self, h, faces_uvs, verts_uvs):
        (fu, fu_p), (vu, vu_p) = _host_i32(faces_uvs), _host_f32(verts_uvs)
        self._run("hifihr_renderer_set_uv", h, fu_p, vu_p, vu.shape[0])

    def render_uv_scratch_bytes(self, h, B):
        return self._call("hifihr_render_uv_scratch_bytes", h, B)

    def render_fwd_uv(self, h, verts, maps, cam, light_color, light_dir, rgba, face_id, texels, ws):
        B, TH, TW = maps.shape[0], maps.shape[1], maps.shape[2]
        self._run("hifihr_render_fwd_uv", h, verts, maps, TH, TW, cam, light_color, light_dir, B, rgba, face_id, texels, ws)

    def render_bwd_uv(self, h, verts, maps, cam, light_color, light_dir, face_id, grad_rgba, texels, gtexels, gverts, gmaps, glc, gld, ws):
        B, TH, TW = maps.shape[0], maps.shape[1], maps.shape[2]
        self._run("hifihr_render_bwd_uv", h, verts, maps, TH, TW, cam, light_color, light_dir, face_id, grad_rgba, B, texels, gtexels, gverts,
                  gmaps, glc, gld, ws)

    def render_bwd(self, h, verts, cam, light_color, light_dir, face_id, grad_rgba, gverts, gvcolors, glc, gld, ws):
        self._run("hifihr_render_bwd", h, verts, cam, light_color, light_dir, face_id, grad_rgba, verts.shape[0], gverts, gvcolors, glc, gld, ws)

    # ---- soft silhouette (csrc/soft_sil.hip) ------------------------------
    def soft_sil_workspace_bytes(self, h, B) -> int:
        return self._call("hifihr_soft_sil_workspace_bytes", h, B)

    def soft_sil_fwd(self, h, verts, cam, sigma, blur_radius, alpha, neglog, ws):
        self._run("hifihr_soft_sil_fwd", h, verts, cam, verts.shape[0], sigma, blur_radius, alpha, neglog, ws)

    def soft_sil_bwd(self, h, verts, cam, neglog, galpha, sigma, blur_radius, gverts, ws):
        self._run("hifihr_soft_sil_bwd", h, verts, cam, neglog, galpha, verts.shape[0], sigma, blur_radius, gverts, ws)

    @staticmethod
    def _mask_kind(mask):
        """The mask_i64 flag of a float32 or int64 mask tensor."""
        assert mask.dtype in (torch.float32, torch.int64), mask.dtype
        return mask.dtype == torch.int64

    def soft_sil_loss_fwd(self, alpha, mask, lam_sil, lam_iou, sums, out):
        """alpha [B, ...]; mask of the same element count, float32 or int64; sums float64 [B, 3]; out float32 [2] (include/hifihr.h)."""
        B = alpha.shape[0]
        assert sums.dtype == torch.float64 and mask.numel() == alpha.numel()
        self._run("hifihr_soft_sil_loss_fwd", alpha, mask, self._mask_kind(mask), B, alpha.numel() // max(B, 1), lam_sil, lam_iou, sums, out)

    def soft_sil_loss_bwd(self, alpha, mask, sums, gout, lam_sil, lam_iou, galpha):
        B = alpha.shape[0]
        self._run("hifihr_soft_sil_loss_bwd", alpha, mask, self._mask_kind(mask), sums, gout, B, alpha.numel() // max(B, 1), lam_sil, lam_iou,
                  galpha)

    # ---- depth map and depth loss (csrc/depth.hip) -------------------------
    def render_depth_workspace_bytes(self, h, B) -> int:
        return self._call("hifihr_render_depth_workspace_bytes", h, B)

    def render_depth_fwd(self, h, verts, cam, face_id, depth, hits):
        """face_id int32 [B, S, S] as render_fwd wrote it for the same verts and cam; depth float32 [B, ..., H, H], hits int32 [B, H, H]."""
        self._run("hifihr_render_depth_fwd", h, verts, cam, face_id, verts.shape[0], depth, hits)

    def render_depth_bwd(self, h, verts, cam, face_id, gdepth, hits, gverts, ws):
        self._run("hifihr_render_depth_bwd", h, verts, cam, face_id, gdepth, hits, verts.shape[0], gverts, ws)

    def _depth_mask_kind(self, mask, n):
        if mask is None:
            return 0
        assert mask.numel() == n, (mask.shape, n)
        return self._mask_kind(mask)

    def depth_loss_fwd(self, depth, hits, target, mask, lam, trunc, sums, out):
        """depth [B, ...]; hits int32 and target float32 of the same element count; mask None, float32 or int64; sums float64 [B, 2];
        out float32 [1] (include/hifihr.h "Depth map")."""
        B = depth.shape[0]
        assert sums.dtype == torch.float64
        assert hits.numel() == depth.numel() and target.numel() == depth.numel(), (depth.shape, hits.shape, target.shape)
        self._run("hifihr_depth_loss_fwd", depth, hits, target, mask, self._depth_mask_kind(mask, depth.numel()), B, depth.numel() // max(B, 1),
                  lam, trunc, sums, out)

    def depth_loss_bwd(self, depth, hits, target, mask, sums, gout, lam, trunc, gdepth):
        B = depth.shape[0]
        self._run("hifihr_depth_loss_bwd", depth, hits, target, mask, self._depth_mask_kind(mask, depth.numel()), sums, gout, B,
                  depth.numel() // max(B, 1), lam, trunc, gdepth)

    # ---- mesh regularisers (csrc/mesh_reg.hip) ----------------------------
    def mesh_topology_create(self, faces, V) -> c_void_p:
        """faces [F, 3] (host); raises when the library refuses them (include/hifihr.h "Mesh regularisers")."""
        f, f_p = _host_i32(faces)
        assert f.ndim == 2 and f.shape[1] == 3, f.shape
        h = self._call("hifihr_mesh_topology_create", f_p, f.shape[0], V)
        if not h:
            raise HifihrError(f"hifihr_mesh_topology_create failed: {self.c.hifihr_last_error().decode()}")
        return c_void_p(h)

    def mesh_topology_destroy(self, h):
        self._call("hifihr_mesh_topology_destroy", h)

    def mesh_topology_counts(self, h):
        """-> (V, E, Q)"""
        v, e, q = c_int32(), c_int32(), c_int32()
        self._run("hifihr_mesh_topology_counts", h, ctypes.byref(v), ctypes.byref(e), ctypes.byref(q))
        return v.value, e.value, q.value

    def mesh_reg_partial_floats(self, h, B) -> int:
        return self._call("hifihr_mesh_reg_partial_floats", h, B)

    def mesh_reg_fwd(self, h, verts, lam_lap, lam_nc, unit, partial, out):
        """verts, unit [B, V, 3]; partial [mesh_reg_partial_floats(h, B)]; out [2]"""
        self._run("hifihr_mesh_reg_fwd", h, verts, verts.shape[0], lam_lap, lam_nc, unit, partial, out)

    def mesh_reg_bwd(self, h, verts, unit, gout, lam_lap, lam_nc, gverts):
        self._run("hifihr_mesh_reg_bwd", h, verts, unit, gout, verts.shape[0], lam_lap, lam_nc, gverts)

    # ---- Chamfer distance (csrc/chamfer.hip) ------------------------------
    def chamfer_geometry(self):
        """-> (queries per workgroup, searched points per LDS pass)"""
        q, t = c_int32(), c_int32()
        self._call("hifihr_chamfer_geometry", ctypes.byref(q), ctypes.byref(t))
        return q.value, t.value

    def chamfer_workspace_bytes(self, B, N, M) -> int:
        return self._call("hifihr_chamfer_workspace_bytes", B, N, M)

    def chamfer_fwd(self, x, y, w_xy, w_yx, idx_xy, idx_yx, min_xy, min_yx, sums, out, ws):
        """x [B, N, 3], y [B, M, 3]; idx_* int32 and min_* float64 [B, N] / [B, M]; sums float64 [B, 2]; out [1]; ws: a byte tensor of
        chamfer_workspace_bytes(B, N, M)"""
        B, N, M = x.shape[0], x.shape[1], y.shape[1]
        assert min_xy.dtype == torch.float64 and min_yx.dtype == torch.float64 and sums.dtype == torch.float64
        assert _nbytes(ws) >= self.chamfer_workspace_bytes(B, N, M)
        self._run("hifihr_chamfer_fwd", x, y, B, N, M, w_xy, w_yx, idx_xy, idx_yx, min_xy, min_yx, sums, out, ws)

    def chamfer_bwd(self, x, y, idx_xy, idx_yx, gout, w_xy, w_yx, gx, gy):
        """gx [B, N, 3] / gy [B, M, 3] or None: the set is skipped; gout [1] on the device"""
        self._run("hifihr_chamfer_bwd", x, y, idx_xy, idx_yx, gout, x.shape[0], x.shape[1], y.shape[1], w_xy, w_yx, gx, gy)

    # ---- point-to-mesh distance (csrc/point_mesh.hip) ------------------------
    def point_mesh_geometry(self):
        """-> (points per workgroup, face records per LDS pass, faces per workgroup, points per LDS pass)"""
        g = [c_int32() for _ in range(4)]
        self._call("hifihr_point_mesh_geometry", *[ctypes.byref(x) for x in g])
        return tuple(x.value for x in g)

    def point_mesh_workspace_bytes(self, B, N, V, F) -> int:
        return self._call("hifihr_point_mesh_workspace_bytes", B, N, V, F)

    def point_mesh_fwd(self, p, v, faces, w_pf, w_fp, idx_pf, bary_pf, min_pf, idx_fp, bary_fp, min_fp, sums, out, ws):
        """p [B, N, 3], v [B, V, 3], faces int32 [F, 3]; idx_* int32 [B, N] / [B, F], bary_* float64 [B, N, 3] / [B, F, 3], min_* float64;
        sums float64 [B, 2]; out [1]; ws: point_mesh_workspace_bytes(B, N, V, F) bytes"""
        B, N, V, F = p.shape[0], p.shape[1], v.shape[1], faces.shape[0]
        assert all(t.dtype == torch.float64 for t in (bary_pf, min_pf, bary_fp, min_fp, sums))
        assert v.shape[0] == B and _nbytes(ws) >= self.point_mesh_workspace_bytes(B, N, V, F)
        self._run("hifihr_point_mesh_fwd", p, v, faces, B, N, V, F, w_pf, w_fp, idx_pf, bary_pf, min_pf, idx_fp, bary_fp, min_fp, sums, out, ws)

    def point_mesh_bwd(self, p, v, faces, idx_pf, bary_pf, idx_fp, bary_fp, gout, v2c_off, v2c_corner, w_pf, w_fp, gp, gv, ws):
        """gp [B, N, 3] / gv [B, V, 3] or None: that gradient is skipped; gout [1] on the device; v2c_off int32 [V + 1], v2c_corner int32
        [3 F]: the vertex -> corner table (ops.point_mesh_tables_of)"""
        B, N, V, F = p.shape[0], p.shape[1], v.shape[1], faces.shape[0]
        assert bary_pf.dtype == torch.float64 and bary_fp.dtype == torch.float64 and v2c_off.numel() == V + 1 and v2c_corner.numel() == 3 * F
        assert _nbytes(ws) >= self.point_mesh_workspace_bytes(B, N, V, F)
        self._run("hifihr_point_mesh_bwd", p, v, faces, idx_pf, bary_pf, idx_fp, bary_fp, gout, v2c_off, v2c_corner, B, N, V, F, w_pf, w_fp,
                  gp, gv, ws)


_LIB = None


def get_lib() -> HifihrLib:
    """The product library (HIP, in-tree).  Raises HifihrError when it has not been built."""
    global _LIB
    if _LIB is None:
        _LIB = HifihrLib(LIB_PATH)
    return _LIB


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HifihrError("hifihr_amd ops run on the GPU only (HIP kernels); got a CPU tensor. "
                              "There is no CPU fallback: use oracle/ only from tests.")
