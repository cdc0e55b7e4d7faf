"""The fused LARS / LAMB kernels (csrc/kernels/optim_layerwise.hip): three steps against an
independent per-tensor fp64 loop on the sizes where segment mapping, tails and chunk edges can
break; arena path = per-tensor fallback and run = run, bit for bit; an unaligned fallback tensor;
the arena's padding; hipGraph replay across the schedule's knee; a NaN gradient.

Bounds: max|a - b| / max|b| < 1e-6 for parameters and state and relative 1e-5 for the trust ratios
(tests/test_kernels_gpu.py's bounds for sgd / adam and grad_norm)."""
import copy

import pytest
import torch

from deeplearning_mpi_amd.models import UNet, resnet18
from deeplearning_mpi_amd.ops import bce_with_logits, cross_entropy
from deeplearning_mpi_amd.ops.backend import make_backend
from deeplearning_mpi_amd.optim import LAMB, LARS, clip_grad_norm_
from deeplearning_mpi_amd.utils.arena import LW_CHUNK, ParamArena
from deeplearning_mpi_amd.utils.graphs import CapturedStep
from layerwise_ref import (Bag, C, arena_state, lr_at, make_grads, padding_mask, ref_lamb, ref_lars, rel_err,
                           set_grads)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_P, TOL_R = 1e-6, 1e-5
LARS_HP = dict(lr=1.0, momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02)
LAMB_HP = dict(lr=0.02, weight_decay=0.01)
SCHED = dict(kind="cosine", warmup_steps=2, total_steps=5, min_lr=0.01)


def _make(which, params, **kw):
    if which == "lars":
        return LARS(params, schedule=SCHED, **LARS_HP, **kw)
    return LAMB(params, schedule=SCHED, **LAMB_HP, **kw)


def _run_arena(which, grads, clip=False):
    m = Bag().to(DEV)
    arena = ParamArena(m, DEV, make_backend(DEV))
    opt = _make(which, m.parameters())
    for gs in grads:
        opt.zero_grad()
        set_grads(m, gs, DEV)
        if clip:
            clip_grad_norm_(list(m.parameters()), 1e9, optimizer=opt)
        opt.step()
    torch.cuda.synchronize()
    assert opt._arena is arena and opt._be.__class__.__name__ == "NativeBackend"
    return m, arena, opt


@pytest.fixture(scope="module")
def grads3():
    return make_grads(Bag(), 3)


@pytest.fixture(scope="module")
def arena_runs(grads3):
    """One 3-step arena run per optimizer, shared (read-only) by the tests below."""
    return {w: _run_arena(w, grads3) for w in ("lars", "lamb")}


@pytest.fixture(scope="module")
def refs(grads3):
    ws = [p.detach() for p in Bag().parameters()]
    ex = [p.dim() <= 1 for p in ws]
    return {"lars": ref_lars(ws, grads3, ex, 1.0, wd=1e-4, tc=0.02, sched=SCHED),
            "lamb": ref_lamb(ws, grads3, ex, 0.02, wd=0.01, sched=SCHED)}


def test_chunk_size_is_the_kernels():
    from deeplearning_mpi_amd._ext import native

    assert native().lw_chunk() == LW_CHUNK == C


def test_lars_matches_fp64_loop(arena_runs, refs):
    m, arena, opt = arena_runs["lars"]
    ws, ms, ratios, lr_t = refs["lars"]
    mom = arena_state(arena, opt.state["__flat__"]["momentum_buffer"])
    for n, p, w, a, b in zip(arena.names, m.parameters(), ws, mom, ms):
        print(f"lars {n}: param {rel_err(p, w):.2e} momentum {rel_err(a, b):.2e}")
        assert rel_err(p, w) < TOL_P, n
        assert rel_err(a, b) < TOL_P, n
    got = opt.trust_ratios().double().cpu()
    print("lars ratios", float(((got - ratios).abs() / ratios).max()))
    assert float(((got - ratios).abs() / ratios).max()) < TOL_R
    assert abs(float(opt.current_lr) - lr_t) <= 1e-6 * lr_t
    assert float(opt.state["__flat__"]["step"]) == 3


def test_lamb_matches_fp64_loop(arena_runs, refs):
    m, arena, opt = arena_runs["lamb"]
    ws, ms, vs, ratios, lr_t = refs["lamb"]
    st = opt.state["__flat__"]
    for n, p, w, a, b, c, d in zip(arena.names, m.parameters(), ws, arena_state(arena, st["exp_avg"]), ms,
                                   arena_state(arena, st["exp_avg_sq"]), vs):
        print(f"lamb {n}: param {rel_err(p, w):.2e} m {rel_err(a, b):.2e} v {rel_err(c, d):.2e}")
        assert rel_err(p, w) < TOL_P, n
        assert rel_err(a, b) < TOL_P and rel_err(c, d) < TOL_P, n
    got = opt.trust_ratios().double().cpu()
    print("lamb ratios", float(((got - ratios).abs() / ratios).max()))
    assert float(((got - ratios).abs() / ratios).max()) < TOL_R
    assert abs(float(opt.current_lr) - lr_t) <= 1e-6 * lr_t
    assert float(st["step"]) == 3


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_padding_stays_zero(arena_runs, which):
    _, arena, opt = arena_runs[which]
    pad = padding_mask(arena).to(DEV)
    assert int(pad.sum()) > 0
    for name, t in [("flat", arena.flat)] + [(k, v) for k, v in opt.state["__flat__"].items() if k != "step"]:
        assert not t[pad].any(), name


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_two_runs_are_bit_identical(arena_runs, grads3, which):
    _, a1, o1 = arena_runs[which]
    _, a2, o2 = _run_arena(which, grads3)
    assert torch.equal(a1.flat, a2.flat)
    assert torch.equal(o1.trust_ratios(), o2.trust_ratios())
    for k, v in o1.state["__flat__"].items():
        assert torch.equal(v, o2.state["__flat__"][k]), k


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_arena_path_equals_per_tensor_fallback(arena_runs, grads3, which):
    """The fallback tensors hold what the arena holds, in the arena's memory order (the conv weight
    as stored: [K][R][S][C]); chunks are relative to each tensor's start, so every sum is the same."""
    m, arena, o1 = arena_runs[which]
    init = Bag().to(DEV)
    a0 = ParamArena(init, DEV, make_backend(DEV))

    def stored(src_arena, p, t):
        """t (logical shape of p) as a contiguous tensor in the arena's memory order."""
        i = src_arena.index[id(p)]
        if src_arena.layouts[i] == "krsc":
            return t.permute(0, 2, 3, 1).contiguous()
        return t.contiguous()

    params = [torch.nn.Parameter(stored(a0, p, p.detach()).clone()) for p in a0.params]
    opt = _make(which, params)
    for gs in grads3:
        for q, p, g in zip(params, a0.params, gs):
            q.grad = stored(a0, p, g.to(DEV)).clone()
        opt.step()
    torch.cuda.synchronize()
    assert opt._arena is None
    for q, p0, p in zip(params, a0.params, m.parameters()):
        assert torch.equal(q.detach(), stored(a0, p0, p.detach()))
    assert torch.equal(opt.trust_ratios(), o1.trust_ratios())
    assert torch.equal(opt.current_lr, o1.current_lr)


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_unaligned_fallback_tensor_matches_fp64_loop(which):
    """A [1:] view starts 4 bytes off a 16-byte boundary: the element loop."""
    g = torch.Generator().manual_seed(5)
    n = 2 * C + 7
    base = torch.randn(3, n + 1, generator=g)
    grads = [[torch.randn(3, n, generator=g) * 0.3] for _ in range(3)]
    store = base.to(DEV).reshape(-1)[1:1 + 3 * n]
    p = torch.nn.Parameter(store.view(3, n))
    assert p.data_ptr() % 16 == 4 and p.is_contiguous()
    w0 = p.detach().cpu().clone()
    opt = _make(which, [p])
    for gs in grads:
        p.grad = gs[0].to(DEV)
        opt.step()
    torch.cuda.synchronize()
    if which == "lars":
        ws, _, ratios, _ = ref_lars([w0], grads, [False], 1.0, wd=1e-4, tc=0.02, sched=SCHED)
    else:
        ws, _, _, ratios, _ = ref_lamb([w0], grads, [False], 0.02, wd=0.01, sched=SCHED)
    print(which, "unaligned", rel_err(p, ws[0]))
    assert rel_err(p, ws[0]) < TOL_P
    assert float(((opt.trust_ratios().double().cpu() - ratios).abs() / ratios).max()) < TOL_R


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_nan_gradient_step_is_a_no_op(arena_runs, which):
    """A NaN gradient on step 2 equals the run without that step (LARS sees it in its own gradient
    norm, LAMB through clip_grad_norm_'s skip flag)."""
    out = []
    for nan_step in (1, None):
        _, arena, opt = _run_arena(which, make_grads(Bag(), 3, nan_step=nan_step), clip=which == "lamb")
        st = opt.state["__flat__"]
        out.append([arena.flat.clone(), opt.current_lr.clone(), st["step"].clone()] +
                   [st[k].clone() for k in sorted(st) if k != "step"])
    assert float(out[0][2]) == 3
    for a, b in zip(*out):
        assert torch.equal(a, b)
    if which == "lars":   # and that run is the shared one
        assert torch.equal(out[1][0], arena_runs["lars"][1].flat)


# ---------------------------------------------------------------- hipGraph replay
GRAPH_SCHED = dict(kind="cosine", warmup_steps=3, total_steps=6)


def _run_graph(model, opt_fn, loss_fn, batches, graph):
    opt = opt_fn(model)
    x = batches[0][0].clone()
    y = batches[0][1].clone()

    def step():
        opt.zero_grad()
        loss = loss_fn(model, x, y)
        loss.backward()
        if isinstance(opt, LAMB):
            clip_grad_norm_(model.parameters(), 1.0, optimizer=opt)
        opt.step()
        return loss

    cs = CapturedStep(step, warmup=2, inputs=(x, y), enabled=graph)
    losses, lrs = [], []
    for bx, by in batches:
        cs.set_inputs(bx, by)
        losses.append(cs().clone())
        lrs.append(opt.current_lr.clone())
    torch.cuda.synchronize()
    if graph:
        assert cs.graph is not None
    return torch.stack(losses), torch.cat(lrs), [p.detach().clone() for p in model.parameters()], \
        [b.detach().clone() for b in model.buffers()]


def _check_graph(make, opt_fn, loss_fn, batches, base):
    torch.manual_seed(0)
    m1 = make().to(DEV)
    m2 = copy.deepcopy(m1)
    l1, r1, p1, b1 = _run_graph(m1, opt_fn, loss_fn, batches, graph=False)
    l2, r2, p2, b2 = _run_graph(m2, opt_fn, loss_fn, batches, graph=True)
    assert torch.equal(l1, l2), (l1, l2)
    assert torch.equal(r1, r2), (r1, r2)
    want = torch.tensor([lr_at(base, s, GRAPH_SCHED) for s in range(len(batches))])
    assert torch.allclose(r2.cpu().double(), want.double(), rtol=1e-6, atol=0), (r2, want)
    for a, b in zip(p1 + b1, p2 + b2):
        assert torch.equal(a, b)


def test_resnet18_lars_graph_replay_matches_eager():
    g = torch.Generator(device=DEV).manual_seed(3)
    batches = [(torch.randn(32, 3, 32, 32, device=DEV, generator=g),
                torch.randint(10, (32,), device=DEV, generator=g)) for _ in range(6)]
    _check_graph(lambda: resnet18(num_classes=10),
                 lambda m: LARS(m.parameters(), lr=1.0, momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02,
                                schedule=GRAPH_SCHED),
                 lambda m, x, y: cross_entropy(m(x), y), batches, 1.0)


def test_unet_lamb_clip_graph_replay_matches_eager():
    g = torch.Generator(device=DEV).manual_seed(4)
    batches = [(torch.randn(2, 3, 64, 64, device=DEV, generator=g),
                (torch.rand(2, 64, 64, device=DEV, generator=g) > 0.5).float()) for _ in range(6)]
    _check_graph(lambda: UNet(out_classes=1),
                 lambda m: LAMB(m.parameters(), lr=0.02, schedule=GRAPH_SCHED),
                 lambda m, x, y: bce_with_logits(m(x).squeeze(1), y), batches, 0.02)
