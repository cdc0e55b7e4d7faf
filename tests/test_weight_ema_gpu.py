"""The weight-EMA kernels (csrc/kernels/ema.hip) through NativeBackend, and optim.WeightEMA on the native engine.

Kernel level: every flat size at which a loop changes (vector body, < 4 tail, more than one block, the second trip of
the capped grid plus a tail) times every buffer-range size, each operand carved out of sentinels that must survive,
once 16-byte aligned and once shifted by one element (the element loop: bit-equal to the vector loop).  One update
from identical fp32 state against the fp64 reference of tests/ema_ref.py, evaluated with the omd the device wrote to
state[3]: the element is one subtraction and one fma, so with u = 2^-24, g(k) = k u / (1 - k u),

    |err| <= g(2) (|e| + omd (|w| + |e|)) + 2^-149,

and state[3] itself is within one fp32 ulp of float32(1 - d_t).  Then the decision table (skip flag, step counter,
both; every 1 and 2; four calls each), the swap, the binding's refusals, and the model level: ResNet-18 eager against
a captured step (a process of its own) and a UNet whose NaN step the Adam clip hand-off skips.

The state vector: [n, s, counter seen, omd, fired, 0, 0, 0]; a skipped or non-firing call leaves the average bit for
bit and writes state[4] = 0."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import ema_ref as R
from deeplearning_mpi_amd.ops.backend import NativeBackend

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
ETA = 2.0 ** -149
F32, F64 = torch.float32, torch.float64
SENT = 640.0
PAD = 64          # sentinel elements on either side of an operand (a multiple of 4: 16-byte alignment stays)

NS = [1, 3, 4, 5, 7, 255, 256, 257, 1023, 1025]
N2V = 4 * 4096 * 256 + 4 * 256 + 3   # the grid is capped at 4096 blocks of 256 lanes of float4: a second trip and a tail of 3
NBS = [0, 1, 5, 260]


@pytest.fixture(scope="module")
def nb():
    return NativeBackend(DEV)


def _gam(k):
    return k * U / (1 - k * U)


def _carve(vals, shift=0):
    """(buffer of sentinels, the view of it that holds vals), the view `shift` elements off 16-byte alignment."""
    n = vals.numel()
    buf = torch.full((PAD + shift + n + PAD,), SENT, dtype=vals.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[PAD + shift:PAD + shift + n]
    v.copy_(vals.reshape(-1))
    return buf, v


def _intact(buf, v):
    off = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:off] == SENT).all()) and bool((buf[off + v.numel():] == SENT).all())


def _biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ shared inputs (computed once, never changed)
_STATE = {}


def _state(n, tag="p"):
    """fp32 (e, w) of n elements: magnitudes spanning 1 .. 1e-4 and exact zeros in both, so that a wrong update is
    not hidden under the rounding of a large value."""
    if (n, tag) not in _STATE:
        g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr((n, tag)).encode()))
        i = torch.arange(n, device=DEV)
        e = torch.randn(n, generator=g, device=DEV) * (10.0 ** -(i % 5).float())
        e[i % 11 == 3] = 0.0
        w = torch.randn(n, generator=g, device=DEV) * (10.0 ** -((i + 2) % 5).float())
        w[i % 7 == 2] = 0.0
        _STATE[(n, tag)] = (e, w)
    return _STATE[(n, tag)]


def _vec(vals):
    return _carve(torch.tensor(vals, dtype=F32, device=DEV))


class _Call:
    """One ema_update on carved copies of the shared inputs; keeps what the checks need."""

    def __init__(self, be, n, nbuf, shift, state=(0.0,) * 8, skip=None, counter=None, every=1, warmup=True, decay=0.9999,
                 e=None, eb=None):
        e0, w0 = _state(n)
        self.e0, self.w0 = (e0 if e is None else e), w0
        self.bufs = [_carve(self.e0, shift), _carve(w0, shift)]
        self.eb0 = self.b0 = None
        args = [self.bufs[0][1], self.bufs[1][1], None, None]
        if nbuf:
            eb0, b0 = _state(nbuf, "b")
            self.eb0, self.b0 = (eb0 if eb is None else eb), b0
            self.bufs += [_carve(self.eb0, shift), _carve(b0, shift)]
            args[2:] = [self.bufs[2][1], self.bufs[3][1]]
        self.bufs.append(_vec(list(state)))
        self.state0 = list(state)
        for s in (skip, counter):
            if s is not None:
                self.bufs.append(_vec([s]))
        sk = self.bufs[-2 if counter is not None else -1][1] if skip is not None else None
        ct = self.bufs[-1][1] if counter is not None else None
        be.ema_update(*args, self.bufs[4 if nbuf else 2][1], sk, ct, every, warmup, decay)
        torch.cuda.synchronize()
        self.e, self.eb = args[0].clone(), (args[2].clone() if nbuf else None)
        self.state = self.bufs[4 if nbuf else 2][1].tolist()
        self.intact = all(_intact(b, v) for b, v in self.bufs)
        # the inputs are read only
        self.inputs_kept = _biteq(args[1], w0) and (not nbuf or _biteq(args[3], self.b0))
        if skip is not None:
            self.inputs_kept &= self.bufs[-2 if counter is not None else -1][1].item() == skip
        if counter is not None:
            self.inputs_kept &= self.bufs[-1][1].item() == counter


def _bound_ok(got, e0, w0, omd, what):
    e, w = e0.double(), w0.double()
    ref = e + omd * (w - e)
    tol = _gam(2) * (e.abs() + omd * (w.abs() + e.abs())) + ETA
    err = (got.double() - ref).abs()
    ok = bool((err <= tol).all())
    r = torch.nan_to_num(err / tol, nan=float("inf"))
    assert ok, f"{what}: worst err / bound = {float(r.max()):.4g} at {int(r.argmax())} of {r.numel()}"


@pytest.mark.parametrize("nbuf", NBS)
@pytest.mark.parametrize("n", NS + [N2V])
def test_edge_sizes_aligned_and_shifted(nb, n, nbuf):
    a = _Call(nb, n, nbuf, 0)
    s = _Call(nb, n, nbuf, 1)
    for c in (a, s):
        assert c.intact and c.inputs_kept
        assert c.state[:3] == [1.0, 1.0, 0.0] and c.state[4:] == [1.0, 0.0, 0.0, 0.0]
    omd = a.state[3]
    assert omd == s.state[3] == float(np.float32(0.9))          # s = 0: d_t = (1 + 0) / (10 + 0)
    assert _biteq(a.e, s.e), "the element loop differs from the 16-byte loop"
    _bound_ok(a.e, a.e0, a.w0, omd, f"e n={n}")
    assert not _biteq(a.e, a.e0)
    if nbuf:
        assert _biteq(a.eb, s.eb)
        _bound_ok(a.eb, a.eb0, a.b0, omd, f"eb nb={nbuf}")
        assert not _biteq(a.eb, a.eb0)


@pytest.mark.parametrize("warmup,s,decay", [(True, 0, 0.9999), (True, 5, 0.9999), (True, 1000, 0.9999),
                                            (True, 89990, 0.9999), (True, 1e6, 0.9999), (False, 0, 0.9999),
                                            (False, 7, 0.0), (True, 3, 0.2), (False, 0, 1 - 2.0 ** -30)])
def test_omd_is_within_one_ulp_of_the_fp64_value(nb, warmup, s, decay):
    c = _Call(nb, 257, 5, 0, state=(s, s, 0, 0, 0, 0, 0, 0), warmup=warmup, decay=decay)
    want = np.float32(1.0 - R.decay_at(float(s), decay, warmup))
    assert abs(np.float32(c.state[3]) - want) <= np.spacing(want), (c.state[3], want)
    assert c.state[:2] == [s + 1, s + 1] and c.state[4] == 1.0 and c.intact
    _bound_ok(c.e, c.e0, c.w0, c.state[3], "e")
    _bound_ok(c.eb, c.eb0, c.b0, c.state[3], "eb")


# (skip flag or None, does the counter move before the call (None: no counter)) per call; expected: applied?
ROWS = {
    "no pointers": ([(None, None)] * 4, [True] * 4),
    "skip_flag 0": ([(0.0, None)] * 4, [True] * 4),
    "skip_flag 1": ([(1.0, None)] * 4, [False] * 4),
    "skip_flag mixed": ([(0.0, None), (1.0, None), (2.5, None), (0.0, None)], [True, False, False, True]),
    "counter moved": ([(None, True)] * 4, [True] * 4),
    "counter not moved": ([(None, False)] * 4, [False] * 4),
    "counter mixed": ([(None, True), (None, False), (None, True), (None, True)], [True, False, True, True]),
    "both": ([(0.0, True), (1.0, True), (0.0, False), (1.0, False)], [True, False, False, False]),
    "both applied": ([(0.0, True)] * 4, [True] * 4),
}


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("row", sorted(ROWS))
def test_decision_table(nb, row, every):
    calls, expect = ROWS[row]
    n, nbuf = 1025, 5
    e, eb = _state(n)[0], _state(nbuf, "b")[0]
    state = [0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    counter = 3.0                                     # the optimizer's count as the state last saw it
    seen_applied = fired = 0
    for t, ((skip, moves), want_applied) in enumerate(zip(calls, expect)):
        if moves:
            counter += 1.0
        ct = None if moves is None else counter
        c = _Call(nb, n, nbuf, 0, state=state, skip=skip, counter=ct, every=every, warmup=True, decay=0.9, e=e, eb=eb)
        assert c.intact and c.inputs_kept, (row, t)
        applied, fire = R.decide(state, skip, ct, every)
        assert applied == want_applied, (row, t)
        seen_applied += applied
        assert fire == (applied and seen_applied % every == 0)
        _, want_state, _ = R.update([], [], state, skip, ct, every, True, 0.9, omd=c.state[3])
        assert c.state[:3] == want_state[:3] and c.state[4:] == want_state[4:], (row, t, c.state, want_state)
        if fire:
            want_omd = np.float32(1.0 - R.decay_at(float(fired), 0.9, True))
            assert abs(np.float32(c.state[3]) - want_omd) <= np.spacing(want_omd)
            _bound_ok(c.e, e, c.w0, c.state[3], f"{row} call {t}")
            _bound_ok(c.eb, eb, c.b0, c.state[3], f"{row} call {t} (buffers)")
            assert not _biteq(c.e, e)
            fired += 1
        else:                                           # skipped or not firing: bit-unchanged, omd kept
            assert _biteq(c.e, e) and _biteq(c.eb, eb) and c.state[3] == state[3], (row, t)
        e, eb, state = c.e, c.eb, c.state
    assert state[0] == sum(expect) and state[1] == fired == sum(expect) // every


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n,nbuf", [(1, 0), (3, 1), (5, 5), (257, 260), (1025, 0), (N2V, 5)])
def test_swap_exchanges_exactly_and_twice_is_the_identity(nb, n, nbuf, shift):
    a0, b0 = _state(n)
    bufs = [_carve(a0, shift), _carve(b0, shift)]
    args = [bufs[0][1], bufs[1][1], None, None]
    if nbuf:
        a20, b20 = _state(nbuf, "b")
        bufs += [_carve(a20, shift), _carve(b20, shift)]
        args[2:] = [bufs[2][1], bufs[3][1]]
    nb.ema_swap(*args)
    assert _biteq(args[0], b0) and _biteq(args[1], a0)
    assert not nbuf or (_biteq(args[2], b20) and _biteq(args[3], a20))
    nb.ema_swap(*args)
    assert _biteq(args[0], a0) and _biteq(args[1], b0)
    assert not nbuf or (_biteq(args[2], a20) and _biteq(args[3], b20))
    assert all(_intact(b, v) for b, v in bufs)


def test_binding_refusals(nb):
    C = nb.C
    f = lambda n, dt=F32: torch.zeros(n, dtype=dt, device=DEV)   # noqa: E731
    e, w, eb, b, st = f(8), f(8), f(4), f(4), f(8)
    one = f(1)
    ok = (e, w, eb, b, st, one, one + 1, 1, True, 0.5, True)   # flag 0, counter moved from 0 to 1: applied

    def refused(match, **kw):
        names = ["e", "w", "eb", "b", "state", "skip_flag", "counter", "every", "warmup", "decay", "advance"]
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        with pytest.raises(RuntimeError, match=match):
            C.ema_update(*args)

    C.ema_update(*ok)
    C.ema_update(e, w, None, None, st, None, None, 1, False, 0.0, False)
    refused("ema_update: e must", e=f(8, F64))
    refused("ema_update: w must", w=f(8, torch.bfloat16))
    refused("ema_update: w must", w=f(9))
    refused("ema_update: e must", e=torch.zeros(8))
    refused("ema_update: w must", w=f(16)[::2])
    refused("ema_update: b must", b=f(5))
    refused("ema_update: eb must", eb=f(4, F64))
    refused("come together", b=None)
    refused("ema_update: state must", state=f(7))
    refused("ema_update: state must", state=f(8, F64))
    refused("ema_update: state must", state=torch.zeros(8))
    refused("ema_update: state must", state=f(8).view(2, 4))
    refused("ema_update: skip_flag must", skip_flag=f(2))
    refused("ema_update: counter must", counter=f(1, F64))
    refused("every", every=0)
    refused("every", every=-3)
    for bad in (1.0, 1.5, -0.1, float("nan")):
        refused("decay", decay=bad)
    big = f(16)
    refused("e overlaps w", e=big[0:8], w=big[4:12])
    refused("e overlaps w", e=big[0:8], w=big[0:8])
    refused("eb overlaps b", eb=big[0:4], b=big[3:7])
    assert st.tolist()[:3] == [1.0, 1.0, 1.0]   # the first accepted call advanced it; the refused ones launched nothing
    for args, match in [((e, f(9), None, None), "b must"), ((f(8, F64), w, None, None), "a must"),
                        ((big[0:8], big[7:15], None, None), "a overlaps b"), ((e, w, eb, None), "come together"),
                        ((e, w, eb, f(3)), "b2 must")]:
        with pytest.raises(RuntimeError, match="ema_swap: .*" + match):
            C.ema_swap(*args)


def test_resnet18_captured_step_keeps_the_warmup_and_equals_eager():
    """tests/weight_ema_graph_replay.py in a process of its own (as tests/cls_ce_graph_replay.py: a capture creates
    HIP streams, and the streams a process has created decide which hardware queue a later test's streams share)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "weight_ema_graph_replay.py")], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "captured equals eager: num_updates 3" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_unet_nan_step_is_skipped_by_the_clip_handoff():
    from deeplearning_mpi_amd import optim
    from deeplearning_mpi_amd.models import UNet
    from deeplearning_mpi_amd.ops import bce_with_logits

    torch.manual_seed(0)
    m = UNet(out_classes=1).to(DEV)
    opt = optim.Adam(m.parameters(), lr=1e-3)
    ema = optim.WeightEMA(m, decay=0.9, warmup=True, optimizer=opt)
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(2, 3, 64, 64, device=DEV, generator=g)
    y = (torch.rand(2, 64, 64, device=DEV, generator=g) > 0.5).float()

    def step(scale):
        opt.zero_grad()
        loss = bce_with_logits(m(x).squeeze(1), y) * scale
        loss.backward()
        optim.clip_grad_norm_(m.parameters(), 1.0, optimizer=opt)
        opt.step()
        ema.update()

    step(1.0)
    assert ema._arena is m.arena and ema.state.tolist()[:5] == [1, 1, 1, float(np.float32(0.9)), 1]
    e1, b1, s1, w1 = ema._flat.clone(), ema._fbuf.clone(), ema.state.clone(), m.arena.flat.clone()
    step(float("nan"))
    assert _biteq(w1, m.arena.flat)                                  # Adam skipped
    assert _biteq(e1, ema._flat) and _biteq(b1, ema._fbuf)
    assert torch.equal(s1[:4], ema.state[:4]) and ema.state[4] == 0
    step(1.0)
    st = ema.state.tolist()
    assert st[:3] == [2, 2, 2] and st[4] == 1 and st[3] == float(np.float32(1.0 - 2.0 / 11.0))
    assert not _biteq(e1, ema._flat) and not _biteq(b1, ema._fbuf)
    _bound_ok(ema._flat, e1, m.arena.flat, st[3], "unet e")
    assert bool(torch.isfinite(ema._flat).all()) and bool(torch.isfinite(ema._fbuf).all())
