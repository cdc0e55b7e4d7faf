"""Run by tests/test_weight_ema_gpu.py in a process of its own: ResNet-18 (32 x 32, batch 8, native bf16), SGD and a
WeightEMA(decay 0.9, every 2, warm-up on) whose update() sits inside the step.  Six eager steps against the same six
under CapturedStep (two eager warm-up calls, the capture, replays): the average, its state vector -- num_updates above
all: the warm-up advanced under replay -- and the weights are bit-equal.  Then, under applied(), the top-1 count on a
fixed batch equals that of a fresh model loaded with the average's state_dict."""
import copy

import torch

from deeplearning_mpi_amd import optim
from deeplearning_mpi_amd.models import resnet18
from deeplearning_mpi_amd.ops import cross_entropy, top1_correct
from deeplearning_mpi_amd.utils.graphs import CapturedStep

DEV = "cuda"


def run(model, batches, graph):
    opt = optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-5)
    ema = optim.WeightEMA(model, decay=0.9, warmup=True, every=2, optimizer=opt)
    x, y = batches[0][0].clone(), batches[0][1].clone()

    def step():
        opt.zero_grad()
        loss = cross_entropy(model(x), y)
        loss.backward()
        opt.step()
        ema.update()
        return loss

    cs = CapturedStep(step, warmup=2, inputs=(x, y), enabled=graph)
    for bx, by in batches:
        cs.set_inputs(bx, by)
        cs()
    torch.cuda.synchronize()
    assert not graph or cs.graph is not None, cs.capture_error
    return ema


def main():
    torch.manual_seed(0)
    g = torch.Generator(device=DEV).manual_seed(3)
    batches = [(torch.randn(8, 3, 32, 32, device=DEV, generator=g), torch.randint(10, (8,), device=DEV, generator=g))
               for _ in range(6)]
    m1 = resnet18(num_classes=10).to(DEV)
    m2 = copy.deepcopy(m1)
    e1, e2 = run(m1, batches, False), run(m2, batches, True)
    assert e1._arena is m1.arena and e2._arena is m2.arena
    assert torch.equal(e1.state, e2.state), (e1.state, e2.state)
    st = e2.state.tolist()
    assert st[:2] == [6.0, 3.0] and st[4] == 1.0 and float(e2.num_updates) == 3.0, st
    assert abs(st[3] - (1.0 - 3.0 / 12.0)) < 1e-7, st                  # s = 2 at the third update: d = 3 / 12
    assert torch.equal(e1._flat, e2._flat) and torch.equal(e1._fbuf, e2._fbuf)
    assert torch.equal(m1.arena.flat, m2.arena.flat) and torch.equal(m1.arena.fbuf, m2.arena.fbuf)
    assert not torch.equal(e2._flat, m2.arena.flat) and bool(torch.isfinite(e2._flat).all())

    x, y = batches[0]
    sd = e2.state_dict()
    fresh = resnet18(num_classes=10).to(DEV)
    missing = fresh.load_state_dict({**sd["params"], **sd["buffers"]}, strict=False)
    assert not missing.unexpected_keys and all("num_batches_tracked" in k for k in missing.missing_keys)
    fresh.eval()
    m2.eval()
    with torch.no_grad():
        want = int(top1_correct(fresh(x), y))
        plain = m2(x).clone()
        with e2.applied():
            logits = m2(x).clone()
            got = int(top1_correct(logits, y))
        again = m2(x)
    assert got == want, (got, want)
    assert torch.equal(logits, fresh(x)) and not torch.equal(logits, plain) and torch.equal(plain, again)
    print(f"captured equals eager: num_updates {int(e2.num_updates)}, top-1 {got} of {len(y)}")


if __name__ == "__main__":
    main()
