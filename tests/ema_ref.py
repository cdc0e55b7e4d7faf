"""fp64 reference of the weight EMA (csrc/kernels/ema.hip, optim.WeightEMA): the recurrence and the decision
logic in plain Python on host copies of the state vector, written from the definition and evaluated on the same
inputs as the code under test.

    applied = not (skip_flag != 0) and not (counter == state[2])        (an absent pointer says "applied")
    fire    = applied and (n + 1) % every == 0                          n = state[0]
    d_t     = min(decay, (1 + s) / (10 + s)) if warmup else decay       s = state[1], in fp64
    e       = e + (1 - d_t) (w - e)                                     on fire

``update`` changes none of its arguments.  ``omd`` overrides 1 - d_t (a caller that compares with the kernel passes
the fp32 value the device wrote to state[3], so the bound counts the element's roundings only)."""
import torch

F64 = torch.float64
U = 2.0 ** -24


def decay_at(s, decay, warmup):
    return min(float(decay), (1.0 + s) / (10.0 + s)) if warmup else float(decay)


def decide(state, skip_flag, counter, every):
    """-> (applied, fire) from a host list of the state and host scalars (or None) of the two signals."""
    applied = not (skip_flag is not None and float(skip_flag) != 0.0) and \
        not (counter is not None and float(counter) == state[2])
    return applied, applied and (state[0] + 1) % every == 0


def update(tensors_e, tensors_w, state, skip_flag, counter, every, warmup, decay, omd=None):
    """-> (new fp64 e tensors, new state list, omd used or None)."""
    st = [float(v) for v in state]
    applied, fire = decide(st, skip_flag, counter, every)
    out = [e.to(F64).clone() for e in tensors_e]
    used = None
    if fire:
        used = (1.0 - decay_at(st[1], decay, warmup)) if omd is None else float(omd)
        out = [e + used * (w.to(F64) - e) for e, w in zip(out, tensors_w)]
        st[1] += 1
        st[3] = used
    if applied:
        st[0] += 1
    if counter is not None:
        st[2] = float(counter)
    st[4] = 1.0 if fire else 0.0
    return out, st, used


def closed_form(e0, ws, omds):
    """e_T = prod_t (1 - a_t) e_0 + sum_t a_t prod_{u > t} (1 - a_u) w_t, for the fired updates' (w_t, a_t)."""
    T = len(ws)
    acc = e0.to(F64).clone()
    for a in omds:
        acc = acc * (1.0 - a)
    for t in range(T):
        c = omds[t]
        for a in omds[t + 1:]:
            c = c * (1.0 - a)
        acc = acc + c * ws[t].to(F64)
    return acc
