"""Weight EMA: an exponential moving average of the master weights and the BatchNorm running
statistics, kept on the device, for evaluation and checkpoints (torchvision's ``--model-ema``,
timm's ``ModelEmaV2``).

With the model in one ParamArena the average is one streaming pass over two flat buffers
(``arena.flat`` and ``arena.fbuf``, csrc/kernels/ema.hip); otherwise one launch per tensor with
the same results.  The counters, the warm-up and the "was the optimizer update applied?" decision
live in one device vector (``state``, fp32 [8]), so ``update()`` inside a step captured into a
hipGraph keeps working under replay and a skipped optimizer step leaves the average untouched:

    applied = the optimizer's update was not skipped
    fire    = applied and (n + 1) % every == 0          n: applied optimizer updates seen so far
    d_t     = min(decay, (1 + s) / (10 + s)) if warmup else decay      s: EMA updates so far
    e      += (1 - d_t) * (w - e)                        on fire, for every weight and float buffer

``state`` = [n, s, optimizer step counter last seen, 1 - d_t of the last update, 1 if the last
call updated, 0, 0, 0].
"""
from __future__ import annotations

import contextlib

import torch

from ..ops.backend import make_backend
from ..utils.arena import arena_of
from ..utils.profiler import range as trace_range

_STATE = 8


def _flat1d(t):
    """The memory of a dense tensor as a 1-D view (arena parameters are dense but permuted)."""
    if t.is_contiguous():
        return t.view(-1)
    acc = 1
    for size, stride in sorted(zip(t.shape, t.stride()), key=lambda d: d[1]):
        if size != 1 and stride != acc:
            raise RuntimeError("WeightEMA needs dense parameters and buffers")
        acc *= size
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


class WeightEMA:
    """``WeightEMA(model, decay=0.9999, warmup=True, every=1, optimizer=None)``; ``model`` is the
    DDP wrapper or the bare module.  The average starts as a copy of the weights and float buffers
    at construction; ``update()`` goes after ``optimizer.step()``.

    ``optimizer`` tells how a skipped update is detected: our ``SGD`` by its ``skip_flag`` (read at
    each ``update()``), ``Adam`` / ``AdamW`` / ``LARS`` / ``LAMB`` by their device step counter,
    which advances on applied updates only (clip hand-off, non-finite norms and ``skip_flag``
    alike); ``None`` counts every ``update()`` call as applied.  A skipped step changes nothing:
    not the average, not ``n``, not ``s``.  ``num_batches_tracked`` is not averaged.  Every rank
    holds the same weights after the all-reduce, hence the same average: no collective."""

    fused = True   # False: one launch per tensor even with an arena (A/B, tests)

    def __init__(self, model, decay=0.9999, warmup=True, every=1, optimizer=None):
        from . import _FusedBase

        decay, every = float(decay), int(every)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"WeightEMA: decay must be in [0, 1), got {decay}")
        if every < 1:
            raise ValueError(f"WeightEMA: every must be >= 1, got {every}")
        if optimizer is not None and not isinstance(optimizer, _FusedBase):
            raise TypeError("WeightEMA: optimizer must be one of this package's (SGD, Adam, AdamW, LARS, LAMB)")
        self.decay, self.warmup, self.every = decay, bool(warmup), every
        self.optimizer = optimizer
        named = list(model.named_parameters())
        strip = all(n.startswith("module.") for n, _ in named)
        cut = len("module.") if strip else 0
        self.param_names = [n[cut:] for n, _ in named]
        self._params = [p for _, p in named]
        if not self._params:
            raise ValueError("WeightEMA: the model has no parameters")
        # float buffers, read through their owners: building an arena re-points them
        self.buffer_names, self._owners = [], []
        seen = set()
        for mn, m in model.named_modules():
            for bn, b in m._buffers.items():
                if b is None or not b.is_floating_point() or id(b) in seen:
                    continue
                seen.add(id(b))
                full = (mn + "." if mn else "") + bn
                self.buffer_names.append(full[cut:] if full.startswith("module.") else full)
                self._owners.append((m, bn))
        p0 = self._params[0]
        self.device = p0.device
        self.state = torch.zeros(_STATE, dtype=torch.float32, device=self.device)
        self._arena = self._be = None
        self._bound = False
        self._inside = False
        with torch.no_grad():
            self._rehome([p.detach().clone() for p in self._params], [b.detach().clone() for b in self._buffers()])
        c = self._counter()
        if c is not None:   # the optimizer has stepped before: its count so far is "seen" (device copy, no sync)
            self.state[2:3].copy_(c.reshape(-1)[0:1])

    # ------------------------------------------------------------------ storage
    def _buffers(self):
        return [m._buffers[bn] for m, bn in self._owners]

    def _strides(self):
        return [t.stride() for t in [p.data for p in self._params] + self._buffers()]

    def _find_arena(self):
        """The arena that holds exactly this model's parameters and float buffers, else None."""
        from . import _single_arena

        a = _single_arena(self._params) if self.fused else None
        if a is None:
            return None
        bufs = self._buffers()
        if sum(b.numel() for b in bufs) != a.fbuf_total:
            return None
        base, es = a.fbuf.data_ptr(), a.fbuf.element_size()
        for b in bufs:
            off = b.data_ptr() - base
            if b.dtype != a.fbuf.dtype or not b.is_contiguous() or off < 0 or off % es or \
                    off // es + b.numel() > a.fbuf_total:
                return None
        return a

    def _rehome(self, pvals, bvals):
        """Storage for the average next to the model's present storage, filled with the given values:
        with an arena two flat buffers in its layout (the padding between tensors zero, and it stays
        zero: lerp(0, 0)), else one tensor per parameter / buffer in that tensor's own strides."""
        a = self._find_arena()
        bufs = self._buffers()
        if a is not None:
            self._flat = torch.zeros_like(a.flat)
            self._pe = [self._flat.as_strided(tuple(p.shape), p.data.stride(), a.offsets[a.index[id(p)]])
                        for p in self._params]
            nb = a.fbuf_total
            self._fbuf = torch.zeros(nb, dtype=a.fbuf.dtype, device=a.fbuf.device) if nb else None
            base, es = a.fbuf.data_ptr(), a.fbuf.element_size()
            self._bufe = [self._fbuf[(b.data_ptr() - base) // es:][:b.numel()].view(b.shape) for b in bufs]
            self._live_fbuf = a.fbuf[:nb] if nb else None
            self._be = a.backend if a.backend is not None else make_backend(self.device, a.flat.dtype)
        else:
            self._flat = self._fbuf = self._live_fbuf = None
            self._pe = [torch.empty_like(p.data) for p in self._params]
            self._bufe = [torch.empty_like(b) for b in bufs]
            fa = arena_of(self._params[0])
            self._be = fa.backend if fa is not None and fa.backend is not None else \
                make_backend(self.device, self._params[0].dtype)
        for e, v in zip(self._pe + self._bufe, list(pvals) + list(bvals)):
            e.copy_(v)
        self._arena = a
        self._bound_bufs = [b.data_ptr() for b in bufs]
        self._bound_strides = self._strides()
        self._bound = True

    def _bind(self):
        """Follow the model's storage: the engine builds its arena lazily (first forward / DDP
        construction), possibly after this object was created."""
        a = self._arena
        if a is not None:
            if a.valid() and self._bound_bufs == [b.data_ptr() for b in self._buffers()]:
                return
        elif self._find_arena() is None and self._bound_strides == self._strides():
            return   # (a foreign arena re-homes the parameters in its own memory order: follow their strides)
        with torch.no_grad():
            self._rehome([e.clone() for e in self._pe], [e.clone() for e in self._bufe])

    def _pairs(self):
        """(average, live) 1-D views, one pair per tensor (the per-tensor path)."""
        live = [p.data for p in self._params] + self._buffers()
        return [(_flat1d(e), _flat1d(w)) for e, w in zip(self._pe + self._bufe, live) if w.numel()]

    def _fence(self):
        a = self._arena if self._arena is not None else arena_of(self._params[0])
        if a is not None:
            a.wait_buffers()   # joins an in-flight DDP broadcast of the BN statistics (normally done already)
        return a

    # ------------------------------------------------------------------ the optimizer's verdict
    def _counter(self):
        """The optimizer's device count of applied updates (None: it has none, or none yet)."""
        from . import SGD

        opt = self.optimizer
        if opt is None or isinstance(opt, SGD):
            return None
        st = opt.state.get("__flat__")
        if st is not None and "step" in st:
            return st["step"]
        for g in opt.param_groups:
            for p in g["params"]:
                st = opt.state.get(p)
                if st is not None and "step" in st:
                    return st["step"]   # (per-tensor optimizer state: the counters advance together)
        return None

    def _signals(self):
        from . import SGD

        opt = self.optimizer
        if opt is None:
            return None, None
        if isinstance(opt, SGD):
            return opt.skip_flag, None
        c = self._counter()
        if c is None:
            raise RuntimeError("WeightEMA.update() goes after optimizer.step(): the optimizer has no step counter yet")
        return None, c

    # ------------------------------------------------------------------ public interface
    @torch.no_grad()
    def update(self):
        """After ``optimizer.step()``.  Capturable: no host synchronisation, and on the native path no
        kernel but ours."""
        with trace_range("dlmpi.ema_update"):
            if self._inside:
                raise RuntimeError("WeightEMA.update() inside applied(): the model holds the averaged weights")
            self._bind()
            a = self._fence()
            skip, counter = self._signals()
            args = (self.state, skip, counter, self.every, self.warmup, self.decay)
            if self._arena is not None:
                self._be.ema_update(self._flat, a.flat, self._fbuf, self._live_fbuf, *args)
            else:
                pairs = self._pairs()
                for k, (e, w) in enumerate(pairs):   # every launch decides from the same state; the last advances it
                    self._be.ema_update(e, w, None, None, *args, advance=k == len(pairs) - 1)

    def _swap(self):
        a = self._fence()
        if self._arena is not None:
            self._be.ema_swap(a.flat, self._flat, self._live_fbuf, self._fbuf)
        else:
            for e, w in self._pairs():
                self._be.ema_swap(w, e)
        if a is not None:
            a.mark_updated()   # the compute copies are recast from what the masters hold now

    @contextlib.contextmanager
    def applied(self):
        """The model runs (and ``state_dict()``s) with the averaged weights and BN statistics inside;
        on exit the training weights are back bit for bit.  Not inside a hipGraph capture."""
        if self._inside:
            raise RuntimeError("WeightEMA.applied() re-entered")
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightEMA.applied() inside a graph capture")
        with torch.no_grad():
            self._bind()
            self._swap()
        self._inside = True
        try:
            yield self
        finally:
            self._inside = False
            with torch.no_grad():
                self._swap()

    @torch.no_grad()
    def copy_to(self, model):
        """One way, for export: the averaged weights and float buffers into ``model`` (by name)."""
        if self._inside:
            raise RuntimeError("WeightEMA.copy_to() inside applied()")
        own = self._named()
        tgt = dict(model.named_parameters())
        tgt.update({n: b for n, b in model.named_buffers() if b.is_floating_point()})
        if tgt and all(n.startswith("module.") for n in tgt):
            tgt = {n[len("module."):]: t for n, t in tgt.items()}
        missing = [n for n in own if n not in tgt]
        if missing:
            raise KeyError(f"WeightEMA.copy_to: the model lacks {missing[:3]}")
        for n, e in own.items():
            tgt[n].data.copy_(e)
        a = arena_of(next(iter(model.parameters())))
        if a is not None:
            a.mark_updated()

    def _named(self):
        d = dict(zip(self.param_names, self._pe))
        d.update(zip(self.buffer_names, self._bufe))
        return d

    @property
    def num_updates(self):
        """Device scalar (a view of ``state``): EMA updates applied."""
        return self.state[1]

    @property
    def current_decay(self):
        """Device scalar: d_t of the last EMA update applied, 1 - state[3] (1 before the first)."""
        return 1.0 - self.state[3]

    def state_dict(self):
        """Tensors in the parameters' logical shapes under their names without the ``module.`` prefix
        (not arena order: the state survives a change of the arena layout); plain tensors and
        numbers, so it loads with ``weights_only=True``."""
        if self._inside:
            raise RuntimeError("WeightEMA.state_dict() inside applied(): the model holds the average there")

        def c(t):
            return t.detach().clone(memory_format=torch.contiguous_format)

        return {"params": {n: c(e) for n, e in zip(self.param_names, self._pe)},
                "buffers": {n: c(e) for n, e in zip(self.buffer_names, self._bufe)},
                "state": self.state.clone(), "decay": self.decay, "warmup": self.warmup, "every": self.every}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """After the optimizer's ``load_state_dict``: the state vector is restored whole, so the step
        counter it last saw is the restored optimizer's."""
        if self._inside:
            raise RuntimeError("WeightEMA.load_state_dict() inside applied()")
        self._bind()
        for names, mine, theirs in ((self.param_names, self._pe, sd["params"]),
                                    (self.buffer_names, self._bufe, sd["buffers"])):
            if set(names) != set(theirs):
                raise KeyError(f"WeightEMA.load_state_dict: names differ: {sorted(set(names) ^ set(theirs))[:4]}")
            for n, e in zip(names, mine):
                if tuple(theirs[n].shape) != tuple(e.shape):
                    raise ValueError(f"WeightEMA.load_state_dict: shape of {n}")
                e.copy_(theirs[n])
        self.state.copy_(sd["state"])
        self.decay, self.warmup, self.every = float(sd["decay"]), bool(sd["warmup"]), int(sd["every"])
