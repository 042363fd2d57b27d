"""The reference's three optimizers (main.py:182-191: adam, sgd, adamax) with the gradient clip folded into their step -- the
optimizer side of the training path on the HIP kernels.

`ClipAdam` IS a torch.optim.Adam (same constructor arguments, param groups, `state_dict()` layout: per-parameter `step`,
`exp_avg`, `exp_avg_sq`), so checkpoints, LR schedulers and resume code see nothing new.  What changes is how a step is taken
on the GPU: `clip_and_step(max_norm, inv_world)` does `nn.utils.clip_grad_norm_` + `optimizer.step()` of the reference's
trainer (trainer.py:116-122) in three launches of csrc/optim.hip (norm partials, coefficient + step counters, one pass over
p / g / m / v) with nothing read back by the host -- the library path takes a norm reduction per gradient bucket, a multiply
over every gradient and the fused Adam's own pass.  `step()` alone is the unclipped update on the same kernel.

`ClipSGD` IS a torch.optim.SGD (state `momentum_buffer`; dampening 0, no Nesterov) and `ClipAdamax` a torch.optim.Adamax (state
`step`, `exp_avg`, `exp_inf`) in the same way: the same first two launches, their own update kernel in the third
(cvc_sgd_clip_step, cvc_adamax_clip_step of include/cvc_hip_blocks.h).  What is not the update rule -- the segment and chunk
tables keyed on the tensors' addresses, the in-place rewrite of lr / weight_decay, the tables a rebuild retires, clip_and_step's
arguments, last_norm -- is `_ClipStep`, shared by the three.

Weight averaging: `attach_ema(decay, warmup)` keeps an exponential moving average of every stepped parameter, updated INSIDE the
update launch from the new value still in registers (the `_ema` entries of include/cvc_hip_blocks.h); `averaged()` exchanges the
averages with the parameters' own storage and back.  The shadows are not optimizer state: `state_dict()` stays torch's.

Parameters whose .grad is None are skipped, as the torch optimizers skip them (no state, no step count, no weight decay).
amsgrad / nesterov / dampening / maximize / differentiable are not taken: the reference never sets them (main.py:171-191)."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import hip

_SEG_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("step", "<u8"), ("n", "<i8"), ("lr", "<f4"), ("wd", "<f4")])
_CHUNK_DT = np.dtype([("seg", "<i4"), ("pad", "<i4"), ("start", "<i8")])


def _refuse(name, kw, keys):
    for k in keys:
        if kw.pop(k, False):
            raise ValueError(f"{name}: {k} is not supported")


class _ClipStep:
    """What the three optimizers share.  A subclass gives
         _rule()            the scalars every param group must share (a tuple; raises ValueError when the groups differ)
         _state(p, group)   (m, v, step) of one parameter with a gradient: its state tensors, created on first use; None = the rule
                            has no such operand
         _launch(...)       the C entry's return code"""

    def _init_clip(self):
        self._table = None          # (key, device segment table, chunk table, scratch, norm_coef, nseg, nchunk, *rule)
        self._seg_host = None       # host copy of the segment table (lr / weight_decay are rewritten in place when they change)
        self._retired = []          # tables replaced by a rebuild: kept alive, a captured HIP graph may still replay on them
        self.last_norm: Optional[torch.Tensor] = None       # device scalar: norm of the (averaged) gradient of the last clipped step
        # ---- weight averaging (attach_ema): off = None, and nothing below this line is touched by a step
        self._ema = None            # (decay, warmup)
        self._ema_shadow = {}       # parameter -> its average (NOT in self.state: state_dict() stays torch's layout)
        self._ema_state = None      # device float32[2]: [averaged steps so far, d_eff of the current step] (the kernels keep it)
        self._ema_updates0 = 0.0    # the count _ema_state starts from (load_ema_state_dict before the first step)
        self._ema_ptrs = None       # device array of the step table's shadow addresses, built and retired with the table
        self._swap = None           # (key, segment table, chunk table, shadow addresses, nseg, nchunk) of swap_ema

    def _device_step(self, st, p):
        """the state's `step` as a float32 scalar on the parameter's device (a state_dict loaded from a CPU-step checkpoint is moved)"""
        if not (st["step"].is_cuda and st["step"].dtype == torch.float32):
            st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32, device=p.device)
        return st["step"]

    def _build_table(self):
        name = type(self).__name__
        segs, key = [], []
        rule = self._rule()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.is_contiguous()
                        and p.grad.dtype == torch.float32):
                    raise RuntimeError(f"{name}: contiguous float32 GPU parameters and gradients only (no CPU fallback)")
                m, v, step = self._state(p, group)
                segs.append((p, p.grad, m, v, step, float(group["lr"]), float(group["weight_decay"])))
                key.append((p.data_ptr(), p.grad.data_ptr()) + tuple(0 if t is None else t.data_ptr() for t in (m, v, step)))
                if self._ema is not None:
                    key[-1] += (self._shadow(p).data_ptr(),)
        if not segs:
            return None
        key = (tuple(key),) + rule
        if self._table is not None and self._table[0] == key:
            # same tensors: only the learning rates / weight decays may have moved (a scheduler).  They live in the device table,
            # rewritten IN PLACE so that a captured graph replaying this table honours them
            lr_wd = np.array([(s_[5], s_[6]) for s_ in segs], dtype=np.float32)
            if not (np.array_equal(self._seg_host["lr"], lr_wd[:, 0]) and np.array_equal(self._seg_host["wd"], lr_wd[:, 1])):
                self._seg_host["lr"], self._seg_host["wd"] = lr_wd[:, 0], lr_wd[:, 1]
                self._table[1].copy_(torch.from_numpy(self._seg_host.view(np.uint8).copy()).pin_memory(), non_blocking=False)
            return self._table
        dev = segs[0][0].device
        chunk = int(hip.lib().cvc_optim_chunk_elems())
        # the two tables as numpy records with the C structs' layout (cvc_optim_seg: 5 pointers, int64, 2 floats; cvc_optim_chunk)
        seg_np = np.zeros(len(segs), dtype=_SEG_DT)
        assert seg_np.itemsize == C.sizeof(hip.OptimSeg) and _CHUNK_DT.itemsize == C.sizeof(hip.OptimChunk)
        for i, (p, g, m, v, step, lr, wd) in enumerate(segs):
            for t in (g, m, v):            # (the kernels index every operand with the parameter's element count)
                if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()):
                    raise RuntimeError(f"{name}: contiguous float32 GPU parameters and gradients only (no CPU fallback)")
            seg_np[i] = (p.data_ptr(), g.data_ptr()) + tuple(0 if t is None else t.data_ptr() for t in (m, v, step)) + (p.numel(), lr, wd)
        counts = np.array([(p.numel() + chunk - 1) // chunk for p, *_ in segs], dtype=np.int64)
        chunk_np = np.zeros(int(counts.sum()), dtype=_CHUNK_DT)
        chunk_np["seg"] = np.repeat(np.arange(len(segs), dtype=np.int32), counts)
        first = np.concatenate(([0], np.cumsum(counts)[:-1]))
        chunk_np["start"] = (np.arange(len(chunk_np), dtype=np.int64) - np.repeat(first, counts)) * chunk
        seg_t = torch.from_numpy(seg_np.view(np.uint8)).to(dev)
        chunk_t = torch.from_numpy(chunk_np.view(np.uint8)).to(dev)
        partial = torch.empty(len(chunk_np), dtype=torch.float32, device=dev)
        norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)
        if self._table is not None:
            self._retired.append(self._table)
            if self._ema_ptrs is not None:
                self._retired.append(self._ema_ptrs)
        self._ema_ptrs = None
        if self._ema is not None:
            self._ema_ptrs = torch.tensor([self._ema_shadow[p].data_ptr() for p, *_ in segs], dtype=torch.int64).to(dev)
            if self._ema_state is None:
                self._ema_state = torch.tensor([self._ema_updates0, 0.0], dtype=torch.float32).to(dev)
        self._seg_host = seg_np
        self._table = (key, seg_t, chunk_t, partial, norm_coef, len(segs), len(chunk_np)) + rule
        return self._table

    def sync_hyperparameters(self):
        """Push the param groups' current lr / weight_decay into the device table (in place).  Eager steps do this on their own;
        call it before replaying a HIP graph that captured clip_and_step (Trainer.train_step_graphed does)."""
        if self._table is not None:
            self._build_table()

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def clip_and_step(self, max_norm: float, inv_world: float = 1.0, write_grad: bool = True, zero_grad: bool = False,
                      skip: Optional[torch.Tensor] = None):
        """clip_grad_norm_(all parameters, max_norm) then step(), on the device.  inv_world = 1 / ranks when the gradients are sums
        over ranks (cvc.distributed.GradReducer.finalize(average=False)).  zero_grad: leave every gradient this step consumed
        ZERO (the next step's zero_grad() folded into the pass; instead of the clipped gradient write_grad leaves).  Returns the
        norm as a device scalar.  skip: a device int32 word (cvc.hip.step_status); non-zero when the pass executes = the step is void,
        nothing but the gradients' zeroing happens (see include/cvc_hip.h)."""
        if skip is not None and not (skip.is_cuda and skip.dtype == torch.int32 and skip.numel() >= 1):
            raise TypeError(f"{type(self).__name__}.clip_and_step: skip must be an int32 tensor on the GPU")
        t = self._build_table()
        if t is None:
            return None
        _key, seg_t, chunk_t, partial, norm_coef, nseg, nchunk = t[:7]
        entry, rule_args = self._launch(t)
        ema_args = ()
        if self._ema is not None:
            entry += "_ema"
            ema_args = (self._ema_ptrs.data_ptr(), self._ema_state.data_ptr(), self._ema[0], int(self._ema[1]))
        hip._check(getattr(hip.lib(), entry)(seg_t.data_ptr(), nseg, chunk_t.data_ptr(), nchunk, float(max_norm), float(inv_world),
                                             *rule_args, 2 if zero_grad else (1 if write_grad else 0), partial.data_ptr(),
                                             norm_coef.data_ptr(), skip.data_ptr() if skip is not None else None, *ema_args,
                                             hip._stream()),
                   entry)
        self.last_norm = norm_coef[0]
        return self.last_norm

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.clip_and_step(0.0, 1.0, write_grad=False)
        return loss

    # ------------------------------------------------------------------ weight averaging
    @property
    def ema_active(self) -> bool:
        return self._ema is not None

    def attach_ema(self, decay: float, warmup: bool = False):
        """Keep e = e + (p_new - e) (1 - d_eff) of every stepped parameter from the next step on, inside the update launch.
        d_eff = decay, or min(decay, (1 + n) / (10 + n)) over the n averaged steps so far under `warmup`.  A parameter's shadow is a
        copy of its value when it first enters the step table.  Attach before a step is captured into a graph."""
        name = type(self).__name__
        decay = float(decay)
        if not 0.0 <= decay < 1.0:                   # (NaN fails both comparisons)
            raise ValueError(f"{name}.attach_ema: decay must lie in [0, 1), got {decay}")
        for group in self.param_groups:
            for p in group["params"]:
                if not (p.is_cuda and p.dtype == torch.float32):
                    raise RuntimeError(f"{name}.attach_ema: the average is kept by the HIP step, float32 GPU parameters only "
                                       "(no CPU fallback)")
        self._ema = (decay, bool(warmup))

    def detach_ema(self):
        """Stop averaging and forget the shadows (a graph captured while attached keeps replaying on them: they stay alive)."""
        if self._ema is not None:
            self._retired.append((dict(self._ema_shadow), self._ema_state, self._swap))
        self._ema, self._ema_state, self._ema_updates0, self._swap = None, None, 0.0, None
        self._ema_shadow = {}

    def _shadow(self, p):
        e = self._ema_shadow.get(p)
        if e is None:
            e = self._ema_shadow[p] = p.detach().clone(memory_format=torch.contiguous_format)
        return e

    @property
    def ema_updates(self) -> int:
        """averaged (non-void) steps so far: one host read of the device's counter"""
        return int(self._ema_updates0 if self._ema_state is None else float(self._ema_state[0]))

    def _swap_table(self):
        """segment / chunk tables over EVERY shadowed parameter, with or without a gradient at the moment (p and n alone are read)"""
        ps = [p for group in self.param_groups for p in group["params"] if p in self._ema_shadow]
        if not ps:
            return None
        key = tuple((p.data_ptr(), self._ema_shadow[p].data_ptr()) for p in ps)
        if self._swap is not None and self._swap[0] == key:
            return self._swap
        for p in ps:
            e = self._ema_shadow[p]
            if not (p.is_contiguous() and e.is_cuda and e.dtype == torch.float32 and e.is_contiguous() and e.numel() == p.numel()):
                raise RuntimeError(f"{type(self).__name__}: contiguous float32 GPU parameters and shadows only (no CPU fallback)")
        dev = ps[0].device
        chunk = int(hip.lib().cvc_optim_chunk_elems())
        seg_np = np.zeros(len(ps), dtype=_SEG_DT)
        seg_np["p"], seg_np["n"] = [p.data_ptr() for p in ps], [p.numel() for p in ps]
        counts = (seg_np["n"] + chunk - 1) // chunk
        chunk_np = np.zeros(int(counts.sum()), dtype=_CHUNK_DT)
        chunk_np["seg"] = np.repeat(np.arange(len(ps), dtype=np.int32), counts)
        first = np.concatenate(([0], np.cumsum(counts)[:-1]))
        chunk_np["start"] = (np.arange(len(chunk_np), dtype=np.int64) - np.repeat(first, counts)) * chunk
        if self._swap is not None:
            self._retired.append(self._swap)
        self._swap = (key, torch.from_numpy(seg_np.view(np.uint8)).to(dev), torch.from_numpy(chunk_np.view(np.uint8)).to(dev),
                      torch.tensor([e for _p, e in key], dtype=torch.int64).to(dev), len(ps), len(chunk_np))
        return self._swap

    @torch.no_grad()
    def swap_ema(self):
        """p <-> e of every shadowed parameter, in the parameters' own storage (one launch; twice is the identity).  Whoever caches
        anything derived from the weights is told by the caller (Trainer.averaged_weights)."""
        if self._ema is None:
            raise RuntimeError(f"{type(self).__name__}.swap_ema: no average is attached (attach_ema)")
        t = self._swap_table()
        if t is None:
            return
        _key, seg_t, chunk_t, ptrs, nseg, nchunk = t
        hip._check(hip.lib().cvc_ema_swap(seg_t.data_ptr(), nseg, chunk_t.data_ptr(), nchunk, ptrs.data_ptr(), hip._stream()), "cvc_ema_swap")

    @contextlib.contextmanager
    def averaged(self):
        """the averaged weights in the parameters' storage while the block runs; the live ones come back bit for bit"""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def ema_state_dict(self, model) -> dict:
        """model.state_dict() with every shadowed parameter replaced by its average (copies; buffers and shadow-less parameters are
        the live model's), plus `updates`, the averaged steps so far"""
        if self._ema is None:
            raise RuntimeError(f"{type(self).__name__}.ema_state_dict: no average is attached (attach_ema)")
        sd = {}
        for name, t in model.state_dict(keep_vars=True).items():
            e = self._ema_shadow.get(t) if isinstance(t, torch.nn.Parameter) else None
            sd[name] = (t if e is None else e.view_as(t)).detach().clone()
        assert "updates" not in sd
        sd["updates"] = self.ema_updates
        return sd

    @torch.no_grad()
    def load_ema_state_dict(self, model, sd):
        """the inverse of ema_state_dict: every parameter of this optimizer named in `sd` gets that value as its shadow (created
        where there is none yet), the counter gets `updates`"""
        if self._ema is None:
            raise RuntimeError(f"{type(self).__name__}.load_ema_state_dict: no average is attached (attach_ema)")
        mine = {p for group in self.param_groups for p in group["params"]}
        for name, p in model.named_parameters():
            if p not in mine or name not in sd:
                continue
            v = sd[name]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"load_ema_state_dict: {name} has shape {tuple(v.shape)}, the parameter {tuple(p.shape)}")
            self._shadow(p).view_as(p).copy_(v)
        self._ema_updates0 = float(sd.get("updates", 0))
        if self._ema_state is not None:
            self._ema_state.copy_(torch.tensor([self._ema_updates0, 0.0]))

    def _shared(self, what, pick):
        """the one value of pick(group) over the param groups"""
        vals = {pick(g) for g in self.param_groups}
        if len(vals) != 1:
            raise ValueError(f"{type(self).__name__}: all param groups must share {what} (they do in the reference, main.py:171-191)")
        return vals.pop()


class ClipAdam(_ClipStep, torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **kw):
        _refuse("ClipAdam", kw, ("amsgrad", "maximize", "differentiable"))
        kw.pop("fused", None); kw.pop("foreach", None); kw.pop("capturable", None)
        # capturable=True: the step counters are float32 tensors on the parameters' device, which is what the kernel increments
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True, foreach=False, fused=False)
        self._init_clip()

    # ------------------------------------------------------------------ state, exactly as torch.optim.Adam lays it out
    def _ensure_state(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _rule(self):
        return self._shared("betas and eps", lambda g: (tuple(float(x) for x in g["betas"]), float(g["eps"])))

    def _state(self, p, group):
        st = self._ensure_state(p)
        return st["exp_avg"], st["exp_avg_sq"], self._device_step(st, p)

    def _launch(self, t):
        betas, eps = t[7:]
        return "cvc_adam_clip_step", (betas[0], betas[1], eps)


class ClipSGD(_ClipStep, torch.optim.SGD):
    """torch.optim.SGD(momentum=...) behind the clip: dampening 0, no Nesterov (what the reference builds, main.py:183)."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, **kw):
        _refuse("ClipSGD", kw, ("maximize", "differentiable"))
        if nesterov:
            raise ValueError("ClipSGD: nesterov is not supported")
        if dampening != 0:
            raise ValueError("ClipSGD: dampening is not supported")
        kw.pop("fused", None); kw.pop("foreach", None)
        if kw:
            raise TypeError(f"ClipSGD: unexpected arguments {sorted(kw)}")
        super().__init__(params, lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=False, foreach=False, fused=False)
        self._init_clip()

    def _rule(self):
        for g in self.param_groups:
            if g.get("nesterov") or g.get("dampening", 0) != 0 or g.get("maximize"):
                raise ValueError("ClipSGD: nesterov / dampening / maximize are not supported")
        mom = self._shared("momentum", lambda g: float(g["momentum"]))
        if not 0.0 <= mom < 1.0:
            raise ValueError(f"ClipSGD: momentum must lie in [0, 1), got {mom}")
        return (mom,)

    def _state(self, p, group):
        if group["momentum"] == 0:
            return None, None, None                      # no buffer, as torch keeps none
        st = self.state[p]
        if st.get("momentum_buffer") is None:            # first use, or a state saved before torch's first step (its buffer is None):
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)     # buf = mom 0 + ge is torch's first step
        return st["momentum_buffer"], None, None

    def _launch(self, t):
        return "cvc_sgd_clip_step", (t[7],)


class ClipAdamax(_ClipStep, torch.optim.Adamax):
    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **kw):
        _refuse("ClipAdamax", kw, ("maximize", "differentiable"))
        kw.pop("foreach", None); kw.pop("capturable", None)
        if kw:
            raise TypeError(f"ClipAdamax: unexpected arguments {sorted(kw)}")
        # capturable=True: the step counters are float32 tensors on the parameters' device, which is what the kernel increments
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False, capturable=True)
        self._init_clip()

    def _rule(self):
        betas, eps = self._shared("betas and eps", lambda g: (tuple(float(x) for x in g["betas"]), float(g["eps"])))
        if any(g.get("maximize") for g in self.param_groups):
            raise ValueError("ClipAdamax: maximize is not supported")
        return betas, eps

    def _state(self, p, group):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_inf"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st["exp_avg"], st["exp_inf"], self._device_step(st, p)

    def _launch(self, t):
        betas, eps = t[7:]
        return "cvc_adamax_clip_step", (betas[0], betas[1], eps)
