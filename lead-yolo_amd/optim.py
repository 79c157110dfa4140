"""Fused optimiser steps: gradient-norm clipping + the update rule over the reference's three parameter groups +
zero_grad + ModelEMA update as a few launches over a device-resident table of tensors, instead of ~50 foreach launches plus a
Python loop over 319 state tensors (reference train.py:330-341; utils/torch_utils.py:318-346, 404-432).

`FusedSGD` (SGD-nesterov, csrc/ly_optim.hip), `FusedAdam` / `FusedAdamW` (csrc/ly_adam.hip) are `torch.optim.Optimizer`s:
`param_groups` (lr / weight_decay / momentum or betas read every step, so LR schedulers and the reference's warm-up loop work
unchanged), `state[p]` in torch's keys (checkpoints interchange with torch.optim.SGD / Adam / AdamW), `step()`.
Learning rates, the EMA decay ramp and the step counters live in a small device array: the step has no host-dependent kernel
argument and can be captured into a hipGraph together with forward and backward (train.GraphedTrainStep)."""
import ctypes

import torch

from . import capi

CHUNK = 4096                 # elements per block, = LY_OPT_CHUNK in csrc/ly_optim.hip and LY_ADAM_CHUNK in csrc/ly_adam.hip


def _pairable(p):
    """p and its `_ly_grad_pair` partner can share one gradient allocation (and do not yet): same-shape contiguous fp32 weights whose
    gradients are unset or plain tensors this optimiser may replace (not views of somebody's bucket)"""
    q = getattr(p, "_ly_grad_pair", None)
    if q is None or not q.requires_grad or q.shape != p.shape or q.device != p.device or q.dtype != torch.float32 or not q.is_contiguous():
        return False
    for t in (p, q):
        g = t.grad
        if g is not None and (g.dtype != torch.float32 or g.shape != t.shape or g._base is not None):
            return False
    return True


def _is_tap_major(g, p):
    """g is a view of p's shape [co, ci, kh, kw] over storage laid out [co][kh][kw][ci]"""
    if g is None or g.dim() != 4 or tuple(g.shape) != tuple(p.shape) or g.is_contiguous():
        return False
    co, ci, kh, kw = p.shape
    return tuple(g.stride()) == (kh * kw * ci, 1, kw * ci, ci)


def _owned(p):
    """the optimiser may choose the gradient's storage: there is none yet, or it is a plain tensor of its own (not a slice of a
    larger buffer such as a ddp.GradReducer bucket)"""
    g = p.grad
    return g is None or _is_tap_major(g, p) or (g.is_contiguous() and g.untyped_storage().nbytes() == g.numel() * g.element_size())


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: a device-resident table of (parameter, gradient, state, EMA) entries built on the first step,
    persistent gradient storage handed to the backward kernels (ops.GradSink; tap-major k x k weight gradients, C3_CA's stacked cv1 / cv2
    pair), the EMA fold (`attach_ema`), step-dependent scalars in the device array `hyper` (`_sync_hyper` writes what the host schedule
    changed), and the zero_grad protocol.  Subclasses name their per-parameter state tensors (`_state_keys`), their table entry and
    their launch."""
    _state_keys = ()             # per-parameter state tensors the table points at
    _struct = None               # ctypes entry type of the table

    def __init__(self, params, defaults, max_norm):
        super().__init__(params, defaults)
        self.max_norm = max_norm
        self._ema = None
        self._table = None
        self._grad_ptrs = None
        self._mask = None               # requires_grad of every parameter when the table was built (_flags)
        self.grad_norm = None           # device scalar: pre-clip global gradient norm of the last step
        self._zeroed = False
        self._sink = None               # the ops.GradSink this optimiser installed; _writes_at_step: its write counter when step() last zeroed the storage
        self._writes_at_step = -1
        self.grad_scale = 1.0           # gradients are read as g * grad_scale: 1 / world_size when the buckets are all-reduced as SUMs

    # ---- EMA -----------------------------------------------------------------------------------------------------
    def attach_ema(self, ema, model):
        """fold `ema.update(model)` (utils/torch_utils.py:418-427) into the step: every floating entry of the model's state_dict"""
        self._ema = (ema, model)
        self._table = None
        return self

    # ---- table ---------------------------------------------------------------------------------------------------
    def _ema_pairs(self):
        """-> ({parameter data_ptr: EMA tensor}, [(buffer, EMA tensor)] for the floating state entries that are not parameters)"""
        ema_of, extra = {}, []
        if self._ema is not None:
            ema, model = self._ema
            msd, esd = model.state_dict(), ema.ema.state_dict()
            pid = {p.data_ptr(): p for g in self.param_groups for p in g["params"]}
            for k, v in esd.items():
                if not v.dtype.is_floating_point:
                    continue
                src = msd[k]
                if v.dtype != torch.float32 or src.dtype != torch.float32 or not v.is_contiguous() or not src.is_contiguous():
                    raise NotImplementedError(f"{type(self).__name__} EMA: {k} must be contiguous float32 on both sides")
                if src.data_ptr() in pid and pid[src.data_ptr()].requires_grad:
                    ema_of[src.data_ptr()] = v
                else:
                    extra.append((src, v))      # buffers, and frozen parameters: ModelEMA.update averages every floating state entry
        return ema_of, extra

    def _flags(self):
        """requires_grad of every parameter, in group order: the table, the gradient storage and the sink hold the trainable ones only"""
        return tuple(p.requires_grad for g in self.param_groups for p in g["params"])

    def _grad_storage(self, p):
        """give p its persistent gradient storage -> (taps, cin) of the table entry (taps > 1: tap-major)"""
        taps, cin = 1, 0
        if getattr(p, "_ly_tap_major", False) and p.dim() == 4 and p.shape[2] * p.shape[3] > 1 and _owned(p):
            # k x k convolution weight: gradient storage [cout][kh][kw][cin] (ly_wgrad adds with contiguous atomics), exposed
            # to torch as a permuted VIEW of the parameter's shape; the update kernel maps indices (entry taps / cin)
            co, ci, kh, kw = p.shape
            taps, cin = kh * kw, ci
            if not _is_tap_major(p.grad, p):
                store = torch.zeros((co, kh, kw, ci), dtype=torch.float32, device=p.device)
                view = store.permute(0, 3, 1, 2)
                if p.grad is not None:
                    view.copy_(p.grad)
                p.grad = view
        elif _pairable(p):
            # two weights whose gradients ONE ly_wgrad launch can write as a stacked [2*cout, cin] matrix (C3_CA's cv1 / cv2:
            # grad.ConvBnActPair): adjacent halves of one allocation
            q = p._ly_grad_pair
            both = torch.zeros((2,) + tuple(p.shape), dtype=torch.float32, device=p.device)
            for half, t in zip(both, (p, q)):
                if t.grad is not None:
                    half.copy_(t.grad)
                t.grad = half
        elif p.grad is None:
            p.grad = torch.zeros_like(p)              # persistent gradient storage: autograd accumulates in place
        elif not p.grad.is_contiguous() and not _is_tap_major(p.grad, p):
            p.grad = p.grad.contiguous()
        if _is_tap_major(p.grad, p) and taps == 1:
            co, ci, kh, kw = p.shape
            taps, cin = kh * kw, ci
        if p.grad.dtype != torch.float32 or not (p.grad.is_contiguous() or taps > 1):
            raise NotImplementedError(f"{type(self).__name__} needs float32 gradients, contiguous or tap-major")
        return taps, cin

    def _build(self):
        name = type(self).__name__
        if len(self.param_groups) > 3:
            raise NotImplementedError(f"{name} carries three learning rates (the reference's bias / weight / norm groups)")
        self._begin_build()
        dev = None
        entries, sizes, keep = [], [], []
        ema_of, extra = self._ema_pairs()
        mine = self._sink.targets if self._sink is not None else {}
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if not p.requires_grad:
                    # frozen (the reference's --freeze): no entry, so no update, no decay, no momentum.  Frozen since the last table: the
                    # storage this optimiser gave it goes, as the reference's zero_grad() leaves None for a parameter without gradient
                    if p.grad is not None and mine.get(id(p)) is p.grad:
                        p.grad = None
                    self._frozen(p)
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise NotImplementedError(f"{name} needs contiguous float32 CUDA parameters (fp32 master weights)")
                dev = p.device
                taps, cin = self._grad_storage(p)
                e = ema_of.get(p.data_ptr())
                entry, state = self._param_entry(p, group, gi, taps, cin, e)
                entries.append(entry)
                sizes.append(p.numel())
                keep += [p.grad, *state, e]
                self._check_group(group)
        for src, v in extra:
            entries.append(self._buffer_entry(src, v))
            sizes.append(src.numel())
            keep += [src, v]
        if not entries:
            # every parameter frozen (and no EMA): a table without entries, and step() launches nothing
            dev = next((p.device for g in self.param_groups for p in g["params"]), None)
            if dev is None:
                raise ValueError(f"{name}: no parameters")
        arr = (self._struct * len(entries))(*[self._struct(*e) for e in entries])
        raw = torch.frombuffer(bytearray(bytes(arr) or b"\0"), dtype=torch.uint8).clone()
        blk_t, blk_o = [], []
        for i, n in enumerate(sizes):
            for off in range(0, n, CHUNK):
                blk_t.append(i)
                blk_o.append(off)
        ema_obj = self._ema[0] if self._ema else None
        hyper = self._hyper_init(ema_obj)
        self._table = dict(tab=raw.to(dev), blk_t=torch.tensor(blk_t, dtype=torch.int32, device=dev), blk_o=torch.tensor(blk_o, dtype=torch.int64, device=dev),
                           n_blocks=len(blk_t), ws=torch.zeros(1, dtype=torch.float64, device=dev), hyper=torch.tensor(hyper, dtype=torch.float32, device=dev),
                           keep=keep, lrs=None)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._grad_ptrs = [(p, p.grad.data_ptr(), tuple(self.state[p][k].data_ptr() for k in self._state_keys), float(g["weight_decay"]))
                           for g in self.param_groups for p in g["params"] if p.requires_grad]
        self._mask = self._flags()
        self._zeroed = False
        # the backward kernels may now add weight / BatchNorm gradients straight into this storage (ops.GradSink): no fresh
        # gradient tensors, no zero fills, no AccumulateGrad launches
        from . import ops
        sink = ops.GradSink()
        sink.targets = {id(p): p.grad for g in self.param_groups for p in g["params"] if p.requires_grad}
        ops.SINK = sink
        self._sink = sink

    def _begin_build(self):
        pass

    def _frozen(self, p):
        """_build met a parameter that does not require grad"""

    def _sync_hyper(self):
        """learning rates (and the other host-set scalars) follow param_groups — schedulers / warm-up write them; one small H2D copy per
        range only when they change"""
        t = self._table
        slots = self._hyper_slots()
        key = tuple(v for _, vals in slots for v in vals)
        if key != t["lrs"]:
            for start, vals in slots:
                t["hyper"][start:start + len(vals)].copy_(torch.tensor(vals, dtype=torch.float32), non_blocking=True)
            t["lrs"] = key

    def device_state(self):
        """every device tensor a step of this optimiser changes: the per-parameter state tensors, then `hyper`, the norm accumulator and
        grad_norm (train.GraphedTrainStep's exchange probe replays real steps and puts these back)"""
        ts = [st[k] for g in self.param_groups for p in g["params"] for st in (self.state.get(p, {}),) for k in self._state_keys
              if st.get(k) is not None]
        t = self._table
        return ts + [t["hyper"], t["ws"], self.grad_norm]

    # ---- the step --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        name = type(self).__name__
        if closure is not None:
            raise NotImplementedError(f"{name}.step does not take a closure")
        capturing = torch.cuda.is_current_stream_capturing()
        if self._table is None:
            if capturing:
                raise RuntimeError(f"{name}: run one eager step before capturing (the tensor table is built on the first step)")
            self._build()
        if self._flags() != self._mask:                    # parameters were frozen or unfrozen since the table was built
            if capturing:
                raise RuntimeError(f"{name}: requires_grad of its parameters changed since the last step: run one eager step before capturing "
                                   "(the tensor table is rebuilt there)")
            self._build()
        elif not capturing:
            wds = {id(p): float(g["weight_decay"]) for g in self.param_groups for p in g["params"]}
            for p, ptr, sptrs, wd in self._grad_ptrs:      # gradients, state tensors and decays must still be what the table says
                st = self.state[p]
                if (p.grad is None or p.grad.data_ptr() != ptr or wds.get(id(p)) != wd
                        or any(st.get(k) is None or st[k].data_ptr() != q for k, q in zip(self._state_keys, sptrs))):
                    self._build()
                    break
        if not capturing:
            self._sync_hyper()
        if self._table["n_blocks"]:
            self._launch(self._table)
        from . import pack
        pack.touch_weights()              # parameters changed through raw pointers: packed-weight images and caches must refresh
        if self._ema is not None and not capturing:
            self._ema[0].updates += 1
        self._zeroed = True
        self._writes_at_step = self._sink.writes if self._sink is not None else -1

    def load_state_dict(self, state_dict):
        """loaded state tensors are new tensors: the device table must be rebuilt around them"""
        super().load_state_dict(state_dict)
        self._table = None

    def mark_dirty(self):
        """a backward wrote gradients behind this object's back (a replayed graph: train.GraphedTrainStep)"""
        self._zeroed = False

    def mark_stepped(self):
        """a replayed optimiser graph has just consumed and zeroed the gradients"""
        self._zeroed = True
        self._writes_at_step = self._sink.writes if self._sink is not None else -1

    def _clean(self):
        """the storage is exactly as step() left it: zeroed, and no backward kernel has been handed a target since (the sink counts them;
        a backward that went through autograd's AccumulateGrad instead — sink replaced or `.grad` re-assigned — counts as dirty too)"""
        from . import ops
        return self._zeroed and self._sink is not None and ops.SINK is self._sink and self._sink.writes == self._writes_at_step

    def zero_grad(self, set_to_none=False):
        """Gradients stay allocated (the table, the backward kernels and a captured graph point at them) and step() leaves them zeroed,
        so the reference loop's `optimizer.step(); optimizer.zero_grad()` costs nothing.  Whenever a backward may have run since the last
        step() — a skipped / NaN step whose gradients are to be discarded, an abandoned micro-batch — it zeroes the persistent storage in
        place (one foreach launch)."""
        if self._table is None:
            super().zero_grad(set_to_none=False)
        elif not self._clean():
            grads = [p.grad for g in self.param_groups for p in g["params"] if p.requires_grad and p.grad is not None]
            if grads:
                torch._foreach_zero_(grads)
            self._zeroed = True
            self._writes_at_step = self._sink.writes if self._sink is not None else -1

    fused = True


class FusedSGD(_FusedOptimizer):
    _state_keys = ("momentum_buffer",)
    _struct = capi.LyOptTensor

    def __init__(self, params, lr=0.01, momentum=0.937, weight_decay=0.0, nesterov=True, max_norm=10.0):
        if not nesterov or momentum <= 0:
            raise NotImplementedError("FusedSGD implements the LEAD-YOLO recipe: SGD with momentum and nesterov=True")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True), max_norm)

    def _param_entry(self, p, group, gi, taps, cin, e):
        # a fresh momentum buffer is all zeros, and mom*0 + g is torch's first-step rule (buf = g): no first-step flag is needed, so a table
        # rebuilt after load_state_dict (some buffers loaded, some new) never overwrites loaded buffers
        st = self.state[p]
        if "momentum_buffer" not in st or st["momentum_buffer"] is None:
            st["momentum_buffer"] = torch.zeros_like(p)
        buf = st["momentum_buffer"]
        return ((p.data_ptr(), p.grad.data_ptr(), buf.data_ptr(), e.data_ptr() if e is not None else 0, p.numel(),
                 float(group["weight_decay"]), gi, taps, cin), (buf,))

    def _buffer_entry(self, src, v):
        return (src.data_ptr(), 0, 0, v.data_ptr(), src.numel(), 0.0, -1, 1, 0)

    def _check_group(self, group):
        if group["momentum"] != self.param_groups[0]["momentum"]:
            raise NotImplementedError("FusedSGD uses one momentum for all groups")

    def _hyper_init(self, ema_obj):
        return [0.0, 0.0, 0.0, float(self.param_groups[0]["momentum"]), float(self.max_norm or 0.0),
                float(ema_obj.decay_base) if ema_obj is not None else -1.0, float(ema_obj.tau) if ema_obj is not None else 1.0,
                float(ema_obj.updates) if ema_obj is not None else 0.0, 0.0, float(self.grad_scale)]

    def _hyper_slots(self):
        # momentum: the warm-up ramps it (train.py:303-311)
        return [(0, tuple(float(g["lr"]) for g in self.param_groups)), (3, (float(self.param_groups[0]["momentum"]), float(self.max_norm or 0.0))),
                (9, (float(self.grad_scale),))]

    def _launch(self, t):
        capi.check(capi.lib().ly_optim_step(capi.ptr(t["tab"]), capi.ptr(t["blk_t"]), capi.ptr(t["blk_o"]), t["n_blocks"], capi.ptr(t["ws"]),
                                            capi.ptr(t["hyper"]), capi.ptr(self.grad_norm), capi.stream_ptr()), "ly_optim_step")


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam (foreach update, amsgrad / maximize / capturable off) + clip_grad_norm_ + zero_grad (+ ModelEMA.update) in three
    launches of csrc/ly_adam.hip.  `state[p]` holds `exp_avg` / `exp_avg_sq`; the step count is ONE device counter T (hyper[11]) and
    a per-parameter offset step0 (parameter p has taken T - step0 steps), so a captured step needs no host value.  state_dict() /
    load_state_dict() interchange with torch.optim.Adam (`step` as a float32 CPU tensor per parameter)."""
    _state_keys = ("exp_avg", "exp_avg_sq")
    _struct = capi.LyAdamTensor
    decoupled = False            # FusedAdamW: decoupled weight decay

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=10.0, amsgrad=False, maximize=False,
                 capturable=False):
        if amsgrad or maximize or capturable:
            raise NotImplementedError(f"{type(self).__name__} implements Adam without amsgrad, maximize and capturable")
        # the flags torch.optim.Adam keeps per group: a state_dict of this object loads into torch's class and updates alike
        super().__init__(params, dict(lr=lr, betas=tuple(float(b) for b in betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=self.decoupled), max_norm)
        self._T = 0                     # T before the first table is built / after load_state_dict
        self._T_dev = None              # `hyper` of the last table built: its [11] is T from then on (also after attach_ema drops the table)
        self._step0 = {}                # parameter -> value of T when its state was created (its step count is T - step0)
        self._frozen_at = {}            # parameter with state, frozen now -> T when a table was first built without it

    def _steps_taken(self):
        """T (a host sync once a table has been built)"""
        return int(self._T_dev[11].item()) if self._T_dev is not None else self._T

    def _begin_build(self):
        self._T = self._steps_taken()

    def _frozen(self, p):
        if p in self._step0:
            self._frozen_at.setdefault(p, self._T)

    def _param_entry(self, p, group, gi, taps, cin, e):
        st = self.state[p]
        if p in self._frozen_at:                           # unfrozen again: the steps taken without it do not count (torch counts per parameter)
            self._step0[p] = self._step0.get(p, self._T) + self._T - self._frozen_at.pop(p)
        if st.get("exp_avg") is None or st.get("exp_avg_sq") is None:
            st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
            self._step0[p] = self._T                   # no state yet: its first update is torch's step 1
        m, v = st["exp_avg"], st["exp_avg_sq"]
        return ((p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if e is not None else 0, p.numel(),
                 float(group["weight_decay"]), gi, taps, cin, self._step0.get(p, self._T)), (m, v))

    def _buffer_entry(self, src, v):
        return (src.data_ptr(), 0, 0, 0, v.data_ptr(), src.numel(), 0.0, -1, 1, 0, 0)

    def _check_group(self, group):
        g0 = self.param_groups[0]
        if tuple(group["betas"]) != tuple(g0["betas"]) or group["eps"] != g0["eps"]:
            raise NotImplementedError(f"{type(self).__name__} uses one (betas, eps) for all groups")
        if group.get("amsgrad") or group.get("maximize") or group.get("capturable"):
            raise NotImplementedError(f"{type(self).__name__} implements Adam without amsgrad, maximize and capturable")

    def _hyper_init(self, ema_obj):
        b1, b2 = self.param_groups[0]["betas"]
        return [0.0, 0.0, 0.0, float(b1), float(b2), float(self.param_groups[0]["eps"]), float(self.max_norm or 0.0),
                float(ema_obj.decay_base) if ema_obj is not None else -1.0, float(ema_obj.tau) if ema_obj is not None else 1.0,
                float(ema_obj.updates) if ema_obj is not None else 0.0, float(self.grad_scale), float(self._T)]

    def _hyper_slots(self):
        for g in self.param_groups:
            self._check_group(g)
        g0 = self.param_groups[0]
        b1, b2 = g0["betas"]
        return [(0, tuple(float(g["lr"]) for g in self.param_groups)), (3, (float(b1), float(b2), float(g0["eps"]), float(self.max_norm or 0.0))),
                (10, (float(self.grad_scale),))]

    def _build(self):
        super()._build()
        self._T_dev = self._table["hyper"]

    def _launch(self, t):
        capi.check(capi.lib().ly_adam_step(capi.ptr(t["tab"]), capi.ptr(t["blk_t"]), capi.ptr(t["blk_o"]), t["n_blocks"], capi.ptr(t["ws"]),
                                           capi.ptr(t["hyper"]), int(self.decoupled), capi.ptr(self.grad_norm), capi.stream_ptr()), "ly_adam_step")

    def state_dict(self):
        """torch.optim.Adam's form: per parameter exp_avg, exp_avg_sq and `step` (float32 CPU tensor, T - step0)"""
        if torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.state_dict reads the step counter from the device: not while a graph is being captured")
        sd = super().state_dict()
        T = self._steps_taken()
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for p, i in zip(g["params"], sg["params"]):
                if i in sd["state"]:
                    sd["state"][i]["step"] = torch.tensor(float(self._frozen_at.get(p, T) - self._step0.get(p, T)), dtype=torch.float32)
        return sd

    def load_state_dict(self, state_dict):
        """a torch.optim.Adam / AdamW (or FusedAdam / FusedAdamW) state dict: T = the largest loaded step, step0 = T - step per parameter;
        parameters without a loaded entry start at step 1 on the next update"""
        super().load_state_dict(state_dict)
        steps = {p: int(float(st.pop("step"))) for p, st in self.state.items() if "step" in st}
        self._T, self._T_dev = max(steps.values(), default=0), None
        self._step0 = {p: self._T - s for p, s in steps.items()}
        self._frozen_at = {}
        for g in self.param_groups:
            g["decoupled_weight_decay"] = self.decoupled   # the update rule is this class's
            self._check_group(g)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW: FusedAdam with decoupled weight decay (p *= 1 - lr * wd before the update)"""
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=10.0, amsgrad=False, maximize=False,
                 capturable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm, amsgrad=amsgrad, maximize=maximize,
                         capturable=capturable)
