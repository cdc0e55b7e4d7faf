"""Fused optimizers over the ParamArena flat buffers (one kernel launch per step for the whole
model) with torch.optim semantics, plus a launch-free ``clip_grad_norm_``.

Replaces ``optim.SGD(momentum=0.9, weight_decay=1e-5)`` (/root/reference/pytorch/resnet/main.py:114),
``optim.Adam`` (/root/reference/pytorch/unet/train.py:160-161) and
``torch.nn.utils.clip_grad_norm_`` (train.py:194).  When the parameters are not backed by a
single arena the optimizers fall back to one kernel per parameter tensor.

``LARS`` and ``LAMB`` add layer-wise trust ratios for a large global batch: two chunk-indexed passes
over the flat buffers plus one finishing block (csrc/kernels/optim_layerwise.hip), with the step
count, the learning-rate schedule and the skip decision on the device.

``WeightEMA`` (optim/ema.py) averages the master weights and the BatchNorm statistics after each
applied update: one launch over the arena's two flat buffers, its counters on the device as well.
"""
from __future__ import annotations

import torch

from ..ops.backend import make_backend
from ..utils.arena import arena_of
from ..utils.profiler import range as trace_range


def _single_arena(params):
    ars = {id(arena_of(p)) for p in params}
    if len(ars) != 1:
        return None
    a = arena_of(params[0])
    if a is None or len(params) != len(a.params):
        return None
    return a


class _FusedBase(torch.optim.Optimizer):
    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        allp = [p for g in self.param_groups for p in g["params"]]
        self._arena = _single_arena(allp) if len(self.param_groups) == 1 else None
        dev = allp[0].device
        self._be = self._arena.backend if self._arena is not None else make_backend(dev)
        self._step_count = 0

    def zero_grad(self, set_to_none: bool = True):
        self._resolve_arena()
        if self._arena is not None:
            self._arena.zero_grad()   # grads are views of the flat buffer: one memset
        else:
            super().zero_grad(set_to_none=set_to_none)

    def _resolve_arena(self):
        # the engine builds its arena lazily (first forward / DDP construction), possibly after the
        # optimizer was created: pick it up as soon as it exists
        if (self._arena is None or not self._arena.valid()) and len(self.param_groups) == 1:
            a = _single_arena(self.param_groups[0]["params"])
            if a is not None:
                self._arena = a
                self._be = a.backend

    def _groups(self):
        """Yield (group, p, g, state-key-prefix) as flat (arena) or per-tensor views."""
        self._resolve_arena()
        if self._arena is not None:
            g = self.param_groups[0]
            yield g, self._arena.flat, self._arena.grad, "__flat__"
        else:
            for g in self.param_groups:
                for p in g["params"]:
                    if p.grad is None:
                        continue
                    if not (p.is_contiguous() and p.grad.is_contiguous()):
                        raise RuntimeError("fused optimizer fallback needs contiguous params/grads")
                    yield g, p.data.view(-1), p.grad.view(-1), p

    def _buf(self, key, name, like):
        st = self.state[key] if not isinstance(key, str) else self.state.setdefault(key, {})
        if name not in st:
            st[name] = torch.zeros_like(like)
        return st[name]


class SGD(_FusedBase):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov))
        self.skip_flag = None   # optional device scalar: non-zero -> skip the update on every rank

    @torch.no_grad()
    def step(self, closure=None):
        with trace_range("dlmpi.sgd_step"):
            return self._step(closure)

    def _step(self, closure):
        loss = closure() if closure is not None else None
        for g, p, gr, key in self._groups():
            first = "momentum_buffer" not in (self.state[key] if not isinstance(key, str) else
                                              self.state.get(key, {}))
            m = self._buf(key, "momentum_buffer", p) if g["momentum"] != 0 else p
            self._be.sgd(p, gr, m, g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"],
                         first, self.skip_flag)
        if self._arena is not None:
            self._arena.mark_updated()
        self._step_count += 1
        return loss


class Adam(_FusedBase):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.decoupled = decoupled
        self.clip = None   # device [coef, nonfinite] from clip_grad_norm_ (applied & used to skip)
        self._clip_handoff = False   # clip_grad_norm_ left the in-place scaling to this step (see there)

    @torch.no_grad()
    def step(self, closure=None):
        with trace_range("dlmpi.adam_step"):
            return self._step(closure)

    def _step(self, closure):
        loss = closure() if closure is not None else None
        self._step_count += 1
        t = self._step_count
        for g, p, gr, key in self._groups():
            b1, b2 = g["betas"]
            m = self._buf(key, "exp_avg", p)
            v = self._buf(key, "exp_avg_sq", p)
            # the step count lives on the device: the kernel uses step + 1 and advances it only when
            # the update is applied (a collective NaN/Inf skip leaves it unchanged), so a captured
            # step replayed from a hipGraph keeps correct bias corrections
            st = self.state[key] if not isinstance(key, str) else self.state.setdefault(key, {})
            if "step" not in st:
                st["step"] = torch.zeros(1, dtype=torch.float32, device=p.device)
            self._be.adam(p, gr, m, v, g["lr"], b1, b2, g["eps"], g["weight_decay"], self.decoupled,
                          1 - b1 ** t, 1 - b2 ** t, self.clip, st["step"], clip_writeback=self._clip_handoff)
        if self._clip_handoff:   # a handed-off coefficient is used once
            self.clip = None
            self._clip_handoff = False
        if self._arena is not None:
            self._arena.mark_updated()
        return loss


class AdamW(Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, lr, betas, eps, weight_decay, decoupled=True)


_SCHEDULE_KINDS = {"constant": 0, "cosine": 1, "poly": 2}
_TAB = 8   # header floats of the layer-wise table: lr, bc1, bc2, skip, grad norm, first, next bc1, next bc2


def _parse_schedule(schedule):
    """schedule dict -> (kind, warmup_steps, total_steps, min_lr, power); None = constant, no warm-up."""
    s = dict(schedule or {})
    kind = s.pop("kind", "constant")
    if kind not in _SCHEDULE_KINDS:
        raise ValueError(f"schedule kind {kind!r}: one of {sorted(_SCHEDULE_KINDS)}")
    warm, total = int(s.pop("warmup_steps", 0)), int(s.pop("total_steps", 0))
    min_lr, power = float(s.pop("min_lr", 0.0)), float(s.pop("power", 2.0))
    if s:
        raise ValueError(f"unknown schedule keys {sorted(s)}")
    if warm < 0 or (kind != "constant" and total <= 0):
        raise ValueError("schedule: warmup_steps >= 0, and total_steps > 0 for a decaying schedule")
    return (_SCHEDULE_KINDS[kind], float(warm), float(total), min_lr, power)


class _Plan:
    """The layer-wise tables of one pair of flat buffers: the arena's, or one tensor's (fallback)."""

    def __init__(self, seg, pairs, exclude, device, dtype, arena=None):
        self.seg, self.arena = seg, arena
        self.flag_words = []
        for name, q in pairs:
            ex = (q.dim() <= 1) if exclude == "1d" else bool(exclude(name, q)) if exclude is not None else False
            self.flag_words.append(3 if ex else 0)   # bit 0: no weight decay, bit 1: no adaptation
        self.flags = torch.tensor(self.flag_words, dtype=torch.int32).to(device)
        self.tab = torch.zeros(_TAB + len(pairs), dtype=dtype, device=device)
        self.tab[_TAB:] = 1.0
        self.partial = torch.zeros(2 * seg.nchunks, dtype=torch.float32, device=device)
        self.primed = False   # LAMB: tab[6..7] hold the next update's bias corrections (set on first use)
        inv = [0] * len(pairs)   # position in the table of each parameter in the caller's order
        for pos, i in enumerate(seg.order):
            inv[i] = pos
        self.inv = torch.tensor(inv, dtype=torch.int64).to(device)


class _LayerwiseBase(_FusedBase):
    """Shared by LARS and LAMB: per-tensor trust ratios from chunk-indexed kernels, and the step
    count, learning-rate schedule and skip decision on the device.

    ``exclude``: which parameters get neither weight decay nor a trust ratio (ratio 1): ``"1d"``
    (default: every parameter with at most one dimension -- BatchNorm weights and all biases), a
    callable ``(name, param) -> bool``, or ``None`` for none.

    ``schedule``: ``dict(kind="constant"|"cosine"|"poly", warmup_steps=W, total_steps=T, min_lr=0.0,
    power=2.0)``.  With s the number of updates applied so far: s < W gives lr = base (s + 1) / W;
    otherwise q = min(1, (s - W) / max(1, T - W)) and lr = min_lr + (base - min_lr) (1 + cos(pi q)) / 2
    (cosine), min_lr + (base - min_lr) (1 - q)^power (poly) or base (constant).  It is evaluated on the
    device from the device step count, so a step replayed from a hipGraph follows it; the base is
    ``param_groups[0]["lr"]`` as read when ``step()`` is called, so changing it after a capture has
    no effect on replays (as for SGD's lr).  A skipped update changes nothing: not the parameters,
    the state, the step count or the schedule."""

    def __init__(self, params, defaults, exclude, schedule):
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("layer-wise optimizers take one param group (exclusions go through exclude=)")
        if not (exclude is None or exclude == "1d" or callable(exclude)):
            raise ValueError('exclude: "1d", a callable (name, param) -> bool, or None')
        self._exclude = exclude
        self._schedule = _parse_schedule(schedule)
        self._plans = {}

    def _plan(self, key, p):
        """Tables for one group of ``_groups()`` (built and copied to the device on first use: the
        first, eager, step -- never inside a capture)."""
        if isinstance(key, str):
            a = self._arena
            pl = self._plans.get(key)
            if pl is None or pl.arena is not a:
                seg = a.segments()
                pl = self._plans[key] = _Plan(seg, [(a.names[i], a.params[i]) for i in seg.order], self._exclude,
                                              p.device, p.dtype, arena=a)
            return pl
        pl = self._plans.get(id(key))
        if pl is None or pl.seg.numels[0] != p.numel() or pl.tab.device != p.device:
            from ..utils.arena import Segments

            k = next(i for i, q in enumerate(self.param_groups[0]["params"]) if q is key)
            seg = Segments([0], [p.numel()], [1 if key.dim() <= 1 else 0], p.device)
            pl = self._plans[id(key)] = _Plan(seg, [(f"param{k}", key)], self._exclude, p.device, p.dtype)
        return pl

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}   # the tables follow the loaded step count

    def _state_of(self, key, p):
        st = self.state[key] if not isinstance(key, str) else self.state.setdefault(key, {})
        if "step" not in st:   # updates applied so far, on the device (advanced by the kernels)
            st["step"] = torch.zeros(1, dtype=torch.float32, device=p.device)
        return st

    def _active_plans(self):
        if self._arena is not None and "__flat__" in self._plans:
            return [self._plans["__flat__"]]
        return [self._plans[id(q)] for q in self.param_groups[0]["params"] if id(q) in self._plans]

    def trust_ratios(self):
        """Device [T] tensor: the trust ratio each parameter got in the last applied step (1 for
        excluded ones), in arena parameter order (``arena.params`` / ``arena.names``; without an
        arena, the order of the param group)."""
        pls = self._active_plans()
        if not pls:
            return None
        if len(pls) == 1 and pls[0].arena is not None:
            return pls[0].tab[_TAB:][pls[0].inv]
        return torch.cat([pl.tab[_TAB:] for pl in pls])

    @property
    def current_lr(self):
        """Device [1] tensor: the learning rate of the last applied update."""
        pls = self._active_plans()
        return pls[0].tab[0:1] if pls else None


class LARS(_LayerwiseBase):
    """SGD with momentum and layer-wise trust ratios (You et al. 2017) for large global batches.
    For tensor i: r_i = trust_coefficient |w_i| / (|g_i| + wd_i |w_i| + eps) when the tensor is
    adapted and both norms are positive, else 1; d = r_i (g + wd_i w); m = d on the first applied
    update, else momentum m + d; w -= lr_t (d + momentum m if nesterov else m).  Two passes over
    the flat buffers plus one finishing block, whatever the number of tensors.

    ``skip_flag`` (device scalar, non-zero = skip) as for SGD; an update whose global gradient norm
    is not finite is skipped as well.  ``grad_norm``: that norm, a device scalar."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, nesterov=False, trust_coefficient=1e-3, eps=1e-9,
                 exclude="1d", schedule=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                                      trust_coefficient=trust_coefficient, eps=eps), exclude, schedule)
        self.skip_flag = None

    @property
    def grad_norm(self):
        pls = self._active_plans()
        if not pls:
            return None
        if len(pls) == 1:
            return pls[0].tab[4]
        return torch.stack([pl.tab[4] for pl in pls]).double().pow(2).sum().sqrt().to(pls[0].tab.dtype)

    @torch.no_grad()
    def step(self, closure=None):
        with trace_range("dlmpi.lars_step"):
            loss = closure() if closure is not None else None
            for g, p, gr, key in self._groups():
                st = self._state_of(key, p)
                m = self._buf(key, "momentum_buffer", p) if g["momentum"] != 0 else p
                self._be.lars(p, gr, m, self._plan(key, p), st["step"], self.skip_flag, g["lr"], g["momentum"],
                              g["weight_decay"], g["nesterov"], g["trust_coefficient"], g["eps"], self._schedule)
            if self._arena is not None:
                self._arena.mark_updated()
            self._step_count += 1
            return loss


class LAMB(_LayerwiseBase):
    """Adam with layer-wise trust ratios (You et al. 2020).  m and v follow Adam's recurrences;
    u = m_hat / (sqrt(v_hat) + eps) + wd_i w; r_i = |w_i| / |u_i| when the tensor is adapted and both
    norms are positive, else 1; w -= lr_t r_i u.  u is formed twice and never stored: two passes over
    the flat buffers plus one finishing block.

    ``clip``: device (scale, skip) as for Adam.  ``clip_grad_norm_(..., optimizer=lamb)`` scales the
    gradients in place and hands over (1, skip), so a non-finite gradient norm skips the update."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, exclude="1d", schedule=None):
        if not eps > 0:
            raise ValueError("LAMB: eps > 0")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), exclude, schedule)
        self.clip = None

    @torch.no_grad()
    def step(self, closure=None):
        with trace_range("dlmpi.lamb_step"):
            loss = closure() if closure is not None else None
            for g, p, gr, key in self._groups():
                st = self._state_of(key, p)
                m = self._buf(key, "exp_avg", p)
                v = self._buf(key, "exp_avg_sq", p)
                b1, b2 = g["betas"]
                self._be.lamb(p, gr, m, v, self._plan(key, p), st["step"], self.clip, g["lr"], b1, b2, g["eps"],
                              g["weight_decay"], self._schedule)
            if self._arena is not None:
                self._arena.mark_updated()
            self._step_count += 1
            return loss


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, optimizer=None):
    """L2 gradient clipping without a host synchronisation.  Returns the total norm as a device
    tensor.  With ``optimizer`` (our Adam) the clip coefficient is also handed to it so a
    non-finite norm skips the update (the same decision on every rank, because gradients are
    identical after the all-reduce).  With ``optimizer`` and arena-backed parameters (norm_type 2)
    the in-place scaling of the gradients is left to that optimizer's next ``step()``: its kernel
    stores g * coef back while it reads g (one pass over the gradients less, the same products:
    bit-identical update and gradients), so until ``step()`` the gradients are still unscaled.

    ``norm_type`` 2 runs the fused single-pass kernel; any other p (including ``inf``) is the
    torch.nn.utils.clip_grad_norm_ contract computed with device-side torch reductions (still no
    host synchronisation, still capturable)."""
    params = [p for p in parameters if p.grad is not None] if not isinstance(parameters, torch.Tensor) \
        else [parameters]
    a = _single_arena(params)
    dev = params[0].device
    be = a.backend if a is not None else make_backend(dev)
    norm = torch.empty(1, dtype=torch.float32, device=dev)
    # [scale, nonfinite, 1, nonfinite]: the last pair is the optimizer's (scale, skip) once the
    # gradients are scaled in place (written by the same kernel: no copy or fill per step)
    coef = torch.empty(4, dtype=torch.float32, device=dev)
    if float(norm_type) != 2.0:
        grads = [a.grad] if a is not None else [p.grad.reshape(-1) for p in params]
        p = float(norm_type)
        if p == float("inf"):
            n = torch.stack([g.float().abs().max() for g in grads]).max()
        else:
            n = torch.stack([g.double().abs().pow(p).sum() for g in grads]).sum().pow(1.0 / p).float()
        norm.copy_(n.reshape(1))
        coef[0] = torch.clamp(max_norm / (n + 1e-6), max=1.0)
        coef[1] = (~torch.isfinite(n)).float()
        coef[2] = 1.0
        coef[3] = coef[1]
        for g in grads:
            g.mul_(coef[0].to(g.dtype))
    elif a is not None:
        be.grad_norm(a.grad, float(max_norm), norm, coef)
        if optimizer is not None and hasattr(optimizer, "_clip_handoff") and \
                (optimizer._resolve_arena() or getattr(optimizer, "_arena", None) is a):
            optimizer.clip = coef[0:2]   # (scale, skip): applied and stored back by the optimizer's step
            optimizer._clip_handoff = True
            return norm[0]
        be.scale_(a.grad, coef)
    else:
        flat = torch.cat([p.grad.reshape(-1).float() for p in params])
        be.grad_norm(flat, float(max_norm), norm, coef)
        for p in params:
            be.scale_(p.grad.view(-1), coef)
    if optimizer is not None and hasattr(optimizer, "clip"):
        optimizer.clip = coef[2:4]   # grads already scaled in place: scale 1, keep the skip flag
    return norm[0]


from .ema import WeightEMA  # noqa: E402  (after the optimizers it refers to)
