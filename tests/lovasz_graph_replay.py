"""Run by tests/test_lovasz_gpu.py in a process of its own: the CE + Lovasz-Softmax loss and the BCE + Lovasz hinge
loss give the same bits in two eager runs and in the replays of one captured graph whose logits and labels are
rewritten between replays; the counted classes follow the labels, which change with them."""
import torch

import lovasz_ref as R
from deeplearning_mpi_amd.ops import BCELovaszLoss, CELovaszLoss
from deeplearning_mpi_amd.utils.graphs import CapturedStep

DEV = "cuda"
K = 4


def run(crit, x, y, inputs):
    one = torch.ones((), device=DEV)

    def step():
        loss = crit(x, y)
        return loss, torch.autograd.grad(loss, x, one)[0], crit.last_stats["n_classes"]

    captured = CapturedStep(step, warmup=1, inputs=(x, y))
    equal, counted = 0, set()
    for i in range(4):                      # one eager warm-up call, the capture, two replays
        with torch.no_grad():
            captured.set_inputs(*inputs(i))
        loss, grad, ncls = (t.clone() for t in captured())
        for _ in range(2):                  # two eager runs
            el, eg, en = step()
            assert torch.equal(loss, el) and torch.equal(grad, eg) and torch.equal(ncls, en), i
        assert torch.isfinite(loss) and float(grad.abs().sum()) > 0
        counted.add(ncls.item())
        equal += captured.graph is not None and i >= 2
    assert captured.graph is not None, captured.capture_error
    return equal, counted


def main():
    def softmax_inputs(i):
        xc, yc = R.softmax_inputs(K, 20 + i)
        yc[yc >= K - i] = 0                 # another number of classes present every time
        return xc.to(DEV).permute(0, 3, 1, 2), yc.to(DEV)

    def hinge_inputs(i):
        xc, t = R.hinge_inputs(30 + i)
        return xc.to(DEV), t.to(DEV)

    x = torch.zeros(R.N, R.H, R.W, K, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
    y = torch.zeros(R.N, R.H, R.W, dtype=torch.int64, device=DEV)
    equal, counted = run(CELovaszLoss(lovasz_weight=0.5), x, y, softmax_inputs)
    assert counted == {4, 3, 2, 1}, counted
    xb = torch.zeros(R.N, R.H, R.W, device=DEV, requires_grad=True)
    equal += run(BCELovaszLoss(lovasz_weight=0.5), xb, torch.zeros(R.N, R.H, R.W, device=DEV), hinge_inputs)[0]
    print(f"replays equal eager: {equal}")


if __name__ == "__main__":
    main()
