"""Run by tests/test_boundary_gpu.py in a process of its own: the CE + boundary loss and the BCE + boundary loss give
the same bits in two eager runs and in the replays of one captured graph whose logits, labels (so the distance
transform runs inside the graph) and device-side boundary weight are rewritten between replays."""
import torch

import boundary_ref as R
from deeplearning_mpi_amd.ops import BCEBoundaryLoss, CEBoundaryLoss
from deeplearning_mpi_amd.utils.graphs import CapturedStep

DEV = "cuda"
K = 4


def run(crit, x, y, inputs):
    one = torch.ones((), device=DEV)

    def step():
        loss = crit(x, y)
        return loss, torch.autograd.grad(loss, x, one)[0]

    captured = CapturedStep(step, warmup=1, inputs=(x, y))
    equal, losses = 0, set()
    for i in range(4):                      # one eager warm-up call, the capture, two replays
        with torch.no_grad():
            captured.set_inputs(*inputs(i % 2))          # two input sets, so that only the weight tells 0 from 2
            crit.boundary_weight.fill_(0.25 * (i + 1))   # the schedule's write, outside the captured step
        loss, grad = (t.clone() for t in captured())
        for _ in range(2):                  # two eager runs
            el, eg = step()
            assert torch.equal(loss, el) and torch.equal(grad, eg), i
        assert torch.isfinite(loss) and float(grad.abs().sum()) > 0
        losses.add(loss.item())
        equal += captured.graph is not None and i >= 2
    assert captured.graph is not None, captured.capture_error
    assert len(losses) == 4, losses         # every replay followed its inputs and its weight
    return equal


def main():
    def softmax_inputs(i):
        xc, yc, _ = R.softmax_inputs(K, 20 + i)
        return xc.to(DEV).permute(0, 3, 1, 2), yc.to(DEV)

    def sigmoid_inputs(i):
        xc, t, _ = R.sigmoid_inputs(30 + i)
        return xc.to(DEV), t.to(DEV)

    weight = torch.zeros(1, device=DEV)
    x = torch.zeros(R.N, R.H, R.W, K, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
    y = torch.zeros(R.N, R.H, R.W, dtype=torch.int64, device=DEV)
    equal = run(CEBoundaryLoss(boundary_weight=weight), x, y, softmax_inputs)
    xb = torch.zeros(R.N, R.H, R.W, device=DEV, requires_grad=True)
    equal += run(BCEBoundaryLoss(boundary_weight=weight), xb, torch.zeros(R.N, R.H, R.W, device=DEV), sigmoid_inputs)
    print(f"replays equal eager: {equal}")


if __name__ == "__main__":
    main()
