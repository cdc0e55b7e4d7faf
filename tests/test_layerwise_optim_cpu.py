"""LARS / LAMB on the reference backend (the CPU path): three steps against an independent fp64
per-tensor loop, the device-side schedule against its formulas, a skipped step against the run
that never had it, state_dict round trips, and the apps' --optimizer flags."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from deeplearning_mpi_amd.ops.backend import make_backend
from deeplearning_mpi_amd.optim import LAMB, LARS, clip_grad_norm_
from deeplearning_mpi_amd.utils.arena import ParamArena
from layerwise_ref import (Bag, arena_state, lr_at, make_grads, padding_mask, ref_lamb, ref_lars, rel_err,
                           set_grads)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"
# fp32 per-tensor loop against fp64: the bounds of the GPU tests (tests/test_kernels_gpu.py's for
# sgd / adam and grad_norm)
TOL_P, TOL_R = 1e-6, 1e-5
LARS_HP = dict(lr=1.0, momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02)
LAMB_HP = dict(lr=0.02, weight_decay=0.01)
SCHED = dict(kind="cosine", warmup_steps=2, total_steps=5, min_lr=0.01)


def _bag():
    m = Bag()
    arena = ParamArena(m, DEV, make_backend(DEV))
    return m, arena


def _excluded(m):
    return [p.dim() <= 1 for p in m.parameters()]


def _run(make_opt, grads, clip=False):
    m, arena = _bag()
    opt = make_opt(m)
    for gs in grads:
        opt.zero_grad()
        set_grads(m, gs, DEV)
        if clip:
            clip_grad_norm_(list(m.parameters()), 1e9, optimizer=opt)
        opt.step()
    return m, arena, opt


@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_three_steps_match_fp64_loop(nesterov):
    grads = make_grads(Bag(), 3)
    m, arena, opt = _run(lambda m: LARS(m.parameters(), nesterov=nesterov, schedule=SCHED, **LARS_HP), grads)
    assert opt._arena is arena
    ws, ms, ratios, lr_t = ref_lars([p.detach() for p in Bag().parameters()], grads, _excluded(m), LARS_HP["lr"],
                                    wd=LARS_HP["weight_decay"], nesterov=nesterov, tc=0.02, sched=SCHED)
    mom = arena_state(arena, opt.state["__flat__"]["momentum_buffer"])
    for n, p, w, mo, mr in zip(arena.names, m.parameters(), ws, mom, ms):
        assert rel_err(p, w) < TOL_P, n
        assert rel_err(mo, mr) < TOL_P, n
    got = opt.trust_ratios().double()
    assert float(((got - ratios).abs() / ratios).max()) < TOL_R
    assert got[arena.names.index("v10")] == 1 and got[arena.names.index("v1000")] == 1
    assert abs(float(opt.current_lr) - lr_t) <= 1e-6 * lr_t
    gn = torch.cat([g.reshape(-1) for g in grads[-1]]).double().norm()
    assert abs(float(opt.grad_norm) - float(gn)) <= 1e-5 * float(gn)
    assert not arena.flat[padding_mask(arena)].any()


def test_lamb_three_steps_match_fp64_loop():
    grads = make_grads(Bag(), 3)
    m, arena, opt = _run(lambda m: LAMB(m.parameters(), schedule=SCHED, **LAMB_HP), grads)
    ws, ms, vs, ratios, lr_t = ref_lamb([p.detach() for p in Bag().parameters()], grads, _excluded(m), 0.02, wd=0.01,
                                        sched=SCHED)
    st = opt.state["__flat__"]
    for n, p, w, a, b, c, d in zip(arena.names, m.parameters(), ws, arena_state(arena, st["exp_avg"]), ms,
                                   arena_state(arena, st["exp_avg_sq"]), vs):
        assert rel_err(p, w) < TOL_P, n
        assert rel_err(a, b) < TOL_P and rel_err(c, d) < TOL_P, n
    got = opt.trust_ratios().double()
    assert float(((got - ratios).abs() / ratios).max()) < TOL_R
    assert abs(float(opt.current_lr) - lr_t) <= 1e-6 * lr_t
    assert float(st["step"]) == 3
    assert not arena.flat[padding_mask(arena)].any()


def test_exclude_callable_and_none():
    grads = make_grads(Bag(), 1)
    for exclude, want in ((None, lambda n, p: False), (lambda n, p: n.startswith("mats."), None)):
        m, arena, opt = _run(lambda m: LARS(m.parameters(), exclude=exclude, **LARS_HP), grads)
        ex = [(want or exclude)(n, p) for n, p in zip(arena.names, arena.params)]
        ws, _, ratios, _ = ref_lars([p.detach() for p in Bag().parameters()], grads, ex, 1.0, wd=1e-4, tc=0.02)
        for n, p, w in zip(arena.names, m.parameters(), ws):
            assert rel_err(p, w) < TOL_P, n
        assert float(((opt.trust_ratios().double() - ratios).abs() / ratios).max()) < TOL_R


@pytest.mark.parametrize("kind", ["constant", "cosine", "poly"])
@pytest.mark.parametrize("cls", [LARS, LAMB])
def test_schedule_follows_the_formulas(cls, kind):
    """current_lr after update number s + 1 is the formula at s, for s = 0 .. T + 2: that covers
    s = 0, W - 1, W, the middle, T and beyond T."""
    W, T = 3, 8
    sched = dict(kind=kind, warmup_steps=W, total_steps=T, min_lr=0.05, power=2.0)
    p = torch.nn.Parameter(torch.randn(4, 5))
    opt = cls([p], lr=0.5, schedule=sched)
    for s in range(T + 3):
        p.grad = torch.randn(4, 5)
        opt.step()
        want = lr_at(0.5, s, sched)
        assert abs(float(opt.current_lr) - want) <= 1e-6 * want, (s, float(opt.current_lr), want)
    assert lr_at(0.5, 0, sched) == pytest.approx(0.5 / 3) and lr_at(0.5, W - 1, sched) == 0.5
    assert lr_at(0.5, T, sched) == (0.5 if kind == "constant" else 0.05)


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_skipped_step_is_a_no_op(which):
    """A NaN gradient on step 2: parameters, state, step count and current_lr equal the run that
    never had that step, bit for bit."""
    def make(m):
        if which == "lars":
            return LARS(m.parameters(), schedule=SCHED, **LARS_HP)
        return LAMB(m.parameters(), schedule=SCHED, **LAMB_HP)

    out = []
    for nan_step in (1, None):
        m, arena, opt = _run(make, make_grads(Bag(), 3, nan_step=nan_step), clip=which == "lamb")
        st = opt.state["__flat__"]
        out.append([arena.flat.clone(), opt.current_lr.clone(), st["step"].clone()] +
                   [st[k].clone() for k in sorted(st) if k != "step"])
    assert float(out[0][2]) == 3
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("which", ["lars", "lamb"])
def test_state_dict_round_trip_continues_bit_identically(which):
    def make(m):
        if which == "lars":
            return LARS(m.parameters(), schedule=SCHED, **LARS_HP)
        return LAMB(m.parameters(), schedule=SCHED, **LAMB_HP)

    grads = make_grads(Bag(), 4)
    m1, a1, o1 = _run(make, grads[:2])
    sd = copy.deepcopy(o1.state_dict())
    m2, a2 = _bag()
    with torch.no_grad():
        for q, p in zip(m2.parameters(), m1.parameters()):
            q.copy_(p)
    o2 = make(m2)
    o2.load_state_dict(sd)
    for m, o in ((m1, o1), (m2, o2)):
        for gs in grads[2:]:
            o.zero_grad()
            set_grads(m, gs, DEV)
            o.step()
    assert torch.equal(a1.flat, a2.flat)
    assert torch.equal(o1.current_lr, o2.current_lr)
    for k, v in o1.state["__flat__"].items():
        assert torch.equal(v, o2.state["__flat__"][k]), k


def test_fallback_without_arena_matches_arena_path():
    """Parameters not backed by one arena: the same update, one segment table per tensor."""
    grads = make_grads(Bag(), 2)
    m1, arena, o1 = _run(lambda m: LAMB(m.parameters(), **LAMB_HP), grads)
    m2 = Bag()
    o2 = LAMB(m2.parameters(), **LAMB_HP)
    for gs in grads:
        o2.zero_grad()
        set_grads(m2, gs, DEV)
        o2.step()
    assert o2._arena is None
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert rel_err(p, q) < TOL_P
    assert float((o1.trust_ratios() - o2.trust_ratios()).abs().max()) < TOL_R


# ---------------------------------------------------------------- the apps
def _run_app(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


COMMON = ["--synthetic", "--device", "cpu", "--backend", "gloo", "--workers", "0"]


def test_resnet_main_with_lars(tmp_path):
    out = _run_app([sys.executable, "pytorch/resnet/main.py", *COMMON, "--num_epochs", "1", "--batch_size", "8",
                    "--synthetic_size", "16", "--model_dir", str(tmp_path), "--optimizer", "lars", "--lr_schedule",
                    "cosine", "--warmup_steps", "1", "--trust_coefficient", "0.02"])
    assert "Epoch: 0, Accuracy:" in out and "Epoch 0 completed" in out
    assert (tmp_path / "resnet_distributed.pth").exists()


def test_unet_train_with_lamb(tmp_path):
    out = _run_app([sys.executable, "pytorch/unet/train.py", *COMMON, "--num_epochs", "1", "--batch_size", "2",
                    "--image_size", "32", "--synthetic_size", "4", "--eval_every", "1", "--log_dir",
                    str(tmp_path / "logs"), "--model_dir", str(tmp_path), "--optimizer", "lamb", "--weight_decay",
                    "0.02", "--lr_schedule", "poly", "--warmup_steps", "1"])
    assert "Dice Score" in out and "TRAINING COMPLETED" in out


def test_schedule_flags_need_the_layerwise_optimizer(capsys):
    from deeplearning_mpi_amd.apps import classification, segmentation

    for call in (lambda: classification.main("main", ["--warmup_steps", "5"]),
                 lambda: classification.main("main", ["--optimizer", "sgd", "--lr_schedule", "cosine"]),
                 lambda: segmentation.main(["--lr_schedule", "poly"]),
                 lambda: segmentation.main(["--optimizer", "adam", "--warmup_steps", "2"])):
        with pytest.raises(SystemExit) as e:
            call()
        assert e.value.code == 2
        assert "--lr_schedule / --warmup_steps" in capsys.readouterr().err
