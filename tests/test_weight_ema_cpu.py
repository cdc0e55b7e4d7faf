"""optim.WeightEMA on the reference backend with fp64 weights: the closed form of the recurrence, skipped optimizer
steps, applied(), the state_dict round trip, the per-tensor path against the arena path, and the refusals.

The state vector: [n, s, counter seen, omd, fired, 0, 0, 0].  A skipped call writes only state[4] = 0 ("the last
call did not update"); the counters and omd (state[:4]) stay bit for bit."""
import io

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ema_ref as R
from deeplearning_mpi_amd import optim
from deeplearning_mpi_amd.models import resnet18
from deeplearning_mpi_amd.ops import cross_entropy

F64 = torch.float64


class Toy(nn.Module):
    """Two convolutions and a BatchNorm, plain torch: no arena, so the per-tensor path."""

    def __init__(self):
        super().__init__()
        self.c1 = nn.Conv2d(3, 5, 3, padding=1)
        self.bn = nn.BatchNorm2d(5)
        self.c2 = nn.Conv2d(5, 4, 1)

    def forward(self, x):
        return self.c2(F.relu(self.bn(self.c1(x)))).mean((2, 3))


def _toy():
    torch.manual_seed(3)
    return Toy().double(), F.cross_entropy, 4


def _r18():
    torch.manual_seed(4)
    return resnet18(num_classes=10).double(), cross_entropy, 10


MODELS = {"toy": _toy, "resnet18": _r18}


def _batches(K, n, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 3, 32, 32, generator=g, dtype=F64), torch.randint(K, (2,), generator=g)) for _ in range(n)]


def _train_step(model, loss_fn, opt, batch, ema, poison=None, clip=False):
    opt.zero_grad()
    loss_fn(model(batch[0]), batch[1]).backward()
    if poison is not None:
        with torch.no_grad():
            next(p for p in model.parameters() if p.grad is not None and p.dim() == 1).grad[0] = poison
    if clip:
        optim.clip_grad_norm_(model.parameters(), 1.0, optimizer=opt)
    opt.step()
    ema.update()


def _values(model):
    """name -> fp64 clone of every parameter and float buffer (logical shapes)."""
    d = {n: p.detach().clone() for n, p in model.named_parameters()}
    d.update({n: b.detach().clone() for n, b in model.named_buffers() if b.is_floating_point()})
    return d


def _ema_values(ema):
    sd = ema.state_dict()
    return {**sd["params"], **sd["buffers"]}


def _biteq(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_closed_form_over_five_steps(name, warmup, every):
    model, loss_fn, K = MODELS[name]()
    opt = optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    ema = optim.WeightEMA(model, decay=0.9, warmup=warmup, every=every, optimizer=opt)
    e0 = _values(model)
    assert _biteq(e0, _ema_values(ema))          # starts as a copy of the weights and float buffers
    assert not any("num_batches_tracked" in k for k in e0)
    ws, omds = [], []
    for t, b in enumerate(_batches(K, 5)):
        _train_step(model, loss_fn, opt, b, ema)
        assert (ema._arena is not None) == (name == "resnet18")
        if (t + 1) % every == 0:
            ws.append(_values(model))
            omds.append(1.0 - R.decay_at(len(omds), 0.9, warmup))
    st = ema.state.tolist()
    assert st[0] == 5 and st[1] == len(ws) == 5 // every and float(ema.num_updates) == len(ws)
    assert st[4] == float(5 % every == 0)
    assert abs(float(ema.current_decay) - (1.0 - omds[-1])) < 1e-7
    got = _ema_values(ema)
    for k in e0:
        want = R.closed_form(e0[k], [w[k] for w in ws], omds)
        assert float((got[k] - want).abs().max()) <= 1e-12, k
    if ema._arena is not None:                     # the padding between the tensors stays zero
        a = ema._arena
        used = torch.zeros(a.total, dtype=torch.bool)
        for p, off in zip(a.params, a.offsets):
            used[off:off + p.numel()] = True
        assert bool((ema._flat[~used] == 0).all())


def _skip_case(kind):
    model, loss_fn, K = _r18()
    if kind == "sgd":
        opt = optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
        return model, loss_fn, K, opt, dict(), dict()
    if kind == "adam":
        opt = optim.Adam(model.parameters(), lr=1e-3)
        return model, loss_fn, K, opt, dict(clip=True), dict(clip=True, poison=float("nan"))
    opt = optim.LARS(model.parameters(), lr=1e-2)
    return model, loss_fn, K, opt, dict(), dict(poison=float("inf"))


@pytest.mark.parametrize("kind", ["sgd", "adam", "lars"])
def test_skipped_step_changes_nothing(kind):
    model, loss_fn, K, opt, good, bad = _skip_case(kind)
    ema = optim.WeightEMA(model, decay=0.9, warmup=True, every=1, optimizer=opt)
    b = _batches(K, 3)
    _train_step(model, loss_fn, opt, b[0], ema, **good)
    e1, s1, w1 = _ema_values(ema), ema.state.clone(), _values(model)
    assert s1.tolist()[:2] == [1, 1] and s1[4] == 1
    if kind == "sgd":
        opt.skip_flag = torch.ones(1)
    _train_step(model, loss_fn, opt, b[1], ema, **bad)
    w2 = _values(model)
    assert all(torch.equal(w1[k], w2[k]) for k in dict(model.named_parameters()))   # the optimizer did skip
    assert _biteq(e1, _ema_values(ema))
    assert torch.equal(s1[:4], ema.state[:4]) and ema.state[4] == 0 and not ema.state[5:].any()
    if kind == "sgd":
        opt.skip_flag = torch.zeros(1)
    _train_step(model, loss_fn, opt, b[2], ema, **good)
    # the next applied step continues from the state of before the skipped one: update number 2, s = 1
    w3 = _values(model)
    names = sorted(e1)
    want, st, omd = R.update([e1[k] for k in names], [w3[k] for k in names], s1.tolist()[:2] + [-1.0] + [0.0] * 5,
                             None, None, 1, True, 0.9)
    got = _ema_values(ema)
    assert ema.state.tolist()[:2] == [2, 2] == st[:2] and ema.state[4] == 1
    assert abs(float(ema.state[3]) - omd) < 1e-7 and omd == 1.0 - 2.0 / 11.0
    for k, wv in zip(names, want):
        assert float((got[k] - wv).abs().max()) <= 1e-12, k
    if kind != "sgd":
        assert float(ema.state[2]) == 2.0 == float(opt.state["__flat__"]["step"])


def test_counter_of_an_optimizer_that_has_stepped_is_seen_at_construction():
    model, loss_fn, K, opt, good, bad = _skip_case("adam")
    b = _batches(K, 2)
    scratch = optim.WeightEMA(model, optimizer=opt)
    _train_step(model, loss_fn, opt, b[0], scratch, **good)
    ema = optim.WeightEMA(model, decay=0.5, warmup=False, optimizer=opt)
    assert ema.state.tolist()[:3] == [0, 0, 1]
    e0 = _ema_values(ema)
    _train_step(model, loss_fn, opt, b[1], ema, **bad)        # skipped: the counter stays at 1
    assert _biteq(e0, _ema_values(ema)) and ema.state.tolist()[:3] == [0, 0, 1]


def test_applied_swaps_in_and_restores_bit_for_bit():
    model, loss_fn, K = _r18()
    opt = optim.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    ema = optim.WeightEMA(model, decay=0.5, warmup=False, optimizer=opt)
    b = _batches(K, 3)
    for t in range(2):
        _train_step(model, loss_fn, opt, b[t], ema)
    before, avg = _values(model), _ema_values(ema)
    nbt = {n: v.clone() for n, v in model.named_buffers() if not v.is_floating_point()}
    model.eval()
    with torch.no_grad():
        out = model(b[2][0]).clone()
        with ema.applied():
            inside = model.state_dict()
            assert all(torch.equal(inside[k], avg[k]) for k in avg)
            assert all(torch.equal(inside[k], nbt[k]) for k in nbt)       # num_batches_tracked is left alone
            out_ema = model(b[2][0]).clone()
            with pytest.raises(RuntimeError, match="re-entered"):
                with ema.applied():
                    pass
            with pytest.raises(RuntimeError):
                ema.update()
        assert _biteq(before, _values(model)) and _biteq(avg, _ema_values(ema))
        assert torch.equal(out, model(b[2][0]))                            # the compute copies were recast
    assert not torch.equal(out, out_ema)
    model.train()
    # one way: into a fresh model
    other, _, _ = _r18()
    ema.copy_to(other)
    assert all(torch.equal(v, avg[k]) for k, v in _values(other).items())


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_state_dict_round_trip_continues_bit_for_bit(kind):
    def fresh():
        model, loss_fn, K, opt, good, _ = _skip_case(kind)
        with torch.no_grad():
            model(torch.zeros(2, 3, 32, 32, dtype=F64))      # builds the arena before the optimizer looks for it
        return model, loss_fn, opt, good

    b = _batches(10, 5)
    model, loss_fn, opt, good = fresh()
    ema = optim.WeightEMA(model, decay=0.9, warmup=True, every=2, optimizer=opt)
    for t in range(2):
        _train_step(model, loss_fn, opt, b[t], ema, **good)
    f = io.BytesIO()
    torch.save({"model": model.state_dict(), "optimizer": opt.state_dict(), "ema": ema.state_dict()}, f)
    for t in range(2, 5):
        _train_step(model, loss_fn, opt, b[t], ema, **good)

    f.seek(0)
    ck = torch.load(f, weights_only=True)
    sd = ck["ema"]
    assert set(sd) == {"params", "buffers", "state", "decay", "warmup", "every"}
    assert sd["state"].dtype == torch.float32 and sd["state"].shape == (8,)
    assert set(sd["params"]) == {n for n, _ in model.named_parameters()}
    assert all(sd["params"][n].shape == p.shape and sd["params"][n].is_contiguous() for n, p in model.named_parameters())
    model2, _, opt2, _ = fresh()
    model2.load_state_dict(ck["model"])
    model2.arena.mark_updated()
    opt2.load_state_dict(ck["optimizer"])
    ema2 = optim.WeightEMA(model2, decay=0.5, warmup=False, every=1, optimizer=opt2)
    ema2.load_state_dict(sd)                                   # after the optimizer's
    assert (ema2.decay, ema2.warmup, ema2.every) == (0.9, True, 2)
    for t in range(2, 5):
        _train_step(model2, loss_fn, opt2, b[t], ema2, **good)
    assert _biteq(_values(model), _values(model2))
    assert _biteq(_ema_values(ema), _ema_values(ema2)) and torch.equal(ema.state, ema2.state)
    assert ema.state.tolist()[:2] == [5, 2]


def test_ddp_wrapper_names_carry_no_module_prefix():
    class Wrap(nn.Module):
        def __init__(self, m):
            super().__init__()
            self.module = m

    model, _, _ = _toy()
    ema = optim.WeightEMA(Wrap(model), decay=0.9)
    assert set(_ema_values(ema)) == set(_values(model))


def test_arena_path_and_per_tensor_path_are_bit_equal():
    model, loss_fn, K = _r18()
    opt = optim.Adam(model.parameters(), lr=1e-3)
    a = optim.WeightEMA(model, decay=0.9, every=2, optimizer=opt)
    f = optim.WeightEMA(model, decay=0.9, every=2, optimizer=opt)
    f.fused = False
    for t, b in enumerate(_batches(K, 4)):
        _train_step(model, loss_fn, opt, b, a, clip=True, poison=float("nan") if t == 1 else None)
        f.update()
    assert a._arena is not None and f._arena is None and a._flat is not None and f._flat is None
    assert _biteq(_ema_values(a), _ema_values(f)) and torch.equal(a.state, f.state)
    assert a.state.tolist()[:3] == [3, 1, 3]
    before = _values(model)
    with f.applied():
        assert all(torch.equal(v, _values(model)[k]) for k, v in _ema_values(a).items())
    assert _biteq(before, _values(model))


def test_arena_built_after_construction_is_picked_up():
    model, loss_fn, K = _r18()
    opt = optim.SGD(model.parameters(), lr=1e-3)
    ema = optim.WeightEMA(model, decay=0.5, warmup=False, optimizer=opt)   # no arena yet: one tensor each
    assert ema._arena is None
    e0 = _ema_values(ema)
    b = _batches(K, 1)[0]
    _train_step(model, loss_fn, opt, b, ema)
    assert ema._arena is model.arena
    w = _values(model)
    got = _ema_values(ema)
    for k in e0:
        assert float((got[k] - (e0[k] + 0.5 * (w[k] - e0[k]))).abs().max()) <= 1e-12, k


def test_refusals():
    model, _, _ = _toy()
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            optim.WeightEMA(model, decay=bad)
    with pytest.raises(ValueError, match="every"):
        optim.WeightEMA(model, every=0)
    with pytest.raises(TypeError):
        optim.WeightEMA(model, optimizer=torch.optim.SGD(model.parameters(), lr=0.1))
    ema = optim.WeightEMA(model, decay=0.0)
    with ema.applied():
        with pytest.raises(RuntimeError, match="re-entered"):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError):
            ema.state_dict()
    from deeplearning_mpi_amd.ops.backend import RefBackend

    be, e, w, st = RefBackend(), torch.zeros(4), torch.ones(4), torch.zeros(8)
    with pytest.raises(RuntimeError, match="decay"):
        be.ema_update(e, w, None, None, st, None, None, 1, True, 1.0)
    with pytest.raises(RuntimeError, match="every"):
        be.ema_update(e, w, None, None, st, None, None, 0, True, 0.5)
    with pytest.raises(RuntimeError, match="lengths"):
        be.ema_update(e, torch.ones(5), None, None, st, None, None, 1, True, 0.5)
