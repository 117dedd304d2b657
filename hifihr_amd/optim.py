"""Flat parameter / gradient buffers and the fused Adam step.

MI355X-first layout: all trainable parameters of the model live in ONE contiguous fp32 buffer and all their
gradients in another (parameters and .grad are views), so that
  * zero_grad is one memset, the optimizer step is one HBM-bound kernel launch (hifihr_adam_step), and
  * the data-parallel all-reduce runs on contiguous slices of the gradient buffer with no packing copies
    (hifihr_amd/dist.py).
Semantics: torch.optim.Adam as configured at reference train_hrnet.py:546-551.
"""
from __future__ import annotations

import torch

from ._lib import get_lib, require_cuda


class FlatParams:
    """Re-homes module parameters into a flat buffer (registration order) and pins their .grad to views of a
    flat gradient buffer."""

    def __init__(self, module: torch.nn.Module, align: int = 64):
        named = [(n, p) for n, p in module.named_parameters() if p.requires_grad]
        self.params = [p for _, p in named]
        self.names = [n for n, _ in named]
        dev = self.params[0].device
        self.offsets = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + align - 1) // align * align        # keep every tensor 256-byte aligned
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            p.data = self._view(self.flat, p, o, init=p.data)
            p.grad = self._view(self.grad, p, o)
            p._hifihr_direct_grad = True          # kernels may accumulate straight into this (pre-zeroed) buffer

    @staticmethod
    def _view(buf, p, o, init=None):
        """A view of buf[o:o+n] with p's logical shape; conv weights kept in channels_last (physical [K][R][S][C]) stay so."""
        n = p.numel()
        seg = buf[o:o + n]
        if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous():
            K, C, R, S = p.shape
            v = seg.view(K, R, S, C).permute(0, 3, 1, 2)
        else:
            v = seg.view(p.shape)
        if init is not None:
            v.copy_(init)
        return v

    def check_trainable(self):
        """A parameter frozen AFTER it was re-homed here cannot be honoured: its slice of the flat buffers still gets the one Adam launch,
        and the moments it has collected keep moving it even with a zero gradient.  Host-side, before any launch of a step: ValueError
        naming the parameters (freeze with checkpoint.freeze_model_modules BEFORE building FlatParams, or rebuild FlatParams / FusedAdam)."""
        late = [n for n, p in zip(self.names, self.params) if not p.requires_grad]
        if late:
            raise ValueError(f"requires_grad was turned off on {len(late)} parameter(s) that already live in a FlatParams ({', '.join(late[:8])}"
                             f"{', ...' if len(late) > 8 else ''}): the fused Adam step would still move them.  Freeze before FlatParams is built, "
                             f"or rebuild FlatParams and FusedAdam")

    def zero_grad(self):
        self.grad.zero_()
        for p, o in zip(self.params, self.offsets):                # re-pin (a None grad would detach the view)
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self._view(self.grad, p, o)

    def param_count(self):
        return sum(p.numel() for p in self.params)


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics on a FlatParams (one kernel launch per step).  Subclasses Optimizer so that
    torch.optim.lr_scheduler.MultiStepLR (train_hrnet.py:551) drives param_groups[0]['lr'] unchanged."""

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_grad_norm=None):
        """max_grad_norm (None = off: exactly the unguarded launches): a float > 0 turns the gradient guard on -- step() first takes the
        global L2 norm of grad_scale * flat.grad on the device (hifihr_grad_norm), then runs the Adam launch that reads the clip
        coefficient min(1, max_grad_norm / (norm + 1e-6)) and the finite flag from device memory (hifihr_adam_step_guarded).  A gradient
        with a NaN / inf in it leaves parameters and moments untouched; the step still counts (include/hifihr.h).  float('inf') = guard
        only.  Nothing is read back, so a captured step keeps replaying; grad_stats() reads the block for a log line."""
        if max_grad_norm is not None:
            ok = isinstance(max_grad_norm, (int, float)) and not isinstance(max_grad_norm, bool) and max_grad_norm > 0     # (NaN fails >)
            if not ok:
                raise ValueError(f"max_grad_norm must be None (off) or a number > 0 (inf = guard only), got {max_grad_norm!r}")
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        self.flatp = flat
        super().__init__([flat.flat], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self._step_count = 0
        self.grad_scale = grad_scale
        self._lib = None
        # graph mode: the step counter and the learning rate live in device memory (hifihr_adam_step_counted: the kernel derives the bias
        # corrections and advances the counter itself), uploaded by prepare_step() only when the host's view of them changed -- a scheduler
        # step, a restored checkpoint.
        self.graph_mode = False
        self._state = None                  # device image of (lr, betas, step)
        self._state_sig = None              # (lr, betas, completed steps) the device holds
        self._prepared = False              # prepare_step() ran and the launch / replay it announced has not been noted yet
        # gradient guard: the 32-byte block and the norm pass's workspace, allocated ONCE -- captured graphs have their addresses baked in.
        # The counters in the block are not persisted (state_dict() and the .t7 files do not change).
        self._guard = self._guard_ws = None
        if max_grad_norm is not None:
            self._lib = get_lib()
            self._guard, self._guard_ws = self._lib.grad_guard_alloc(flat.flat.numel(), flat.flat.device)

    @property
    def step_count(self):
        return self._step_count

    @step_count.setter
    def step_count(self, value):
        # (a restored snapshot / checkpoint: the device's counter is refreshed by the next prepare_step)
        self._step_count = int(value)
        self._state_sig = None
        self._prepared = False

    def enable_graph_mode(self):
        """The device-side state is allocated ONCE per optimizer: a graph captured after an earlier enable_graph_mode() has the
        buffers' addresses baked in, and a second call (a re-capture after a lambda schedule fired) must not free them under it."""
        self.graph_mode = True
        self._prepared = False
        self._state_sig = None
        require_cuda(self.flatp.flat)
        if self._lib is None:
            self._lib = get_lib()
        if self._state is None:
            self._state = torch.zeros(self._lib.adam_state_bytes(), dtype=torch.uint8, device=self.flatp.flat.device)

    def disable_graph_mode(self):
        """Back to the eager step (scalars passed by value, step counter advanced by step())."""
        self.graph_mode = False
        self._prepared = False
        self._state_sig = None              # whatever the device counter holds is re-uploaded if graph mode comes back

    def note_step_done(self):
        """The launch / replay announced by the last prepare_step() has been enqueued (GraphedTrainStep.__call__ after graph.replay(),
        step() for an eager launch in graph mode).  A prepare_step() that finds the previous one un-noted -- the replay never ran:
        an exception, a caller that prepared twice -- takes its count back and re-uploads the device state, so the host counter
        (bias correction, state_dict()['step']) stays the number of steps that were actually enqueued."""
        self._prepared = False

    def prepare_step(self):
        """Graph mode: advance the step counter; call before each replay.  The device advances its own counter, so the state image
        (lr, betas, completed steps) is uploaded only when what the device holds is not what this step needs."""
        g = self.param_groups[0]
        if self._prepared:                  # the step announced last time was never enqueued
            self._step_count -= 1
            self._state_sig = None
        self._prepared = True
        self._step_count += 1
        b1, b2 = g["betas"]
        want = (float(g["lr"]), float(b1), float(b2), self._step_count - 1)
        if self._state_sig != want:
            self._state.copy_(self._lib.adam_state_image(*want))        # (pageable source: a blocking, stream-ordered copy; rare)
        self._state_sig = (want[0], want[1], want[2], self._step_count)     # after the replay that follows

    def zero_grad(self, set_to_none: bool = False):
        self.flatp.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        if self._lib is None:
            self._lib = get_lib()
        require_cuda(self.flatp.flat)
        g = self.param_groups[0]
        if self.graph_mode:
            capturing = self.flatp.flat.is_cuda and torch.cuda.is_current_stream_capturing()
            if not capturing:               # an eager launch in graph mode (the warm-up steps): it consumes its prepare_step()
                if not self._prepared:
                    raise RuntimeError("FusedAdam.step() in graph mode without prepare_step(): the device-side step counter / the uploaded "
                                       "bias corrections would be those of the previous step")
                self._prepared = False
            if self.max_grad_norm is not None:
                self._lib.grad_norm(self.flatp.grad, self.grad_scale, self.max_grad_norm, self._guard, self._guard_ws)
                self._lib.adam_step_guarded(self.flatp.flat, self.flatp.grad, self.exp_avg, self.exp_avg_sq, self.grad_scale, 0.0, 0.0, 0.0,
                                            g["eps"], g["weight_decay"], 0, self._state, self._guard)
                return
            self._lib.adam_step_counted(self.flatp.flat, self.flatp.grad, self.exp_avg, self.exp_avg_sq, self.grad_scale, g["eps"],
                                        g["weight_decay"], self._state)
            return
        self._step_count += 1
        from .ops import PROFILE
        if self.max_grad_norm is not None:
            def guarded():
                self._lib.grad_norm(self.flatp.grad, self.grad_scale, self.max_grad_norm, self._guard, self._guard_ws)
                self._lib.adam_step_guarded(self.flatp.flat, self.flatp.grad, self.exp_avg, self.exp_avg_sq, self.grad_scale, g["lr"],
                                            g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.step_count, None, self._guard)
            PROFILE.bracket("adam", guarded)
            return
        PROFILE.bracket("adam", lambda: self._lib.adam_step(self.flatp.flat, self.flatp.grad, self.exp_avg, self.exp_avg_sq,
                                                            self.grad_scale, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                                                            g["weight_decay"], self.step_count))

    def grad_stats(self):
        """The guard block as a dict -- norm, clip_coef, finite (of the last step), steps, clipped, skipped (since construction): one
        32-byte copy that SYNCHRONISES, meant for a log line.  None when the guard is off."""
        if self._guard is None:
            return None
        return self._lib.grad_guard_unpack(self._guard.cpu().numpy().tobytes())

    def guard_snapshot(self):
        """The guard block for a later guard_restore() (the warm-up of a captured step must not show in a run's counters)."""
        return None if self._guard is None else self._guard.clone()

    def guard_restore(self, snap):
        if snap is not None:
            self._guard.copy_(snap)

    def state_dict(self):
        return {"step": self.step_count, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
