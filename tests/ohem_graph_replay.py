"""Run by tests/test_ohem_gpu.py in a process of its own: the OHEM loss and its backward give the same bits in two
eager runs and in the replays of one captured graph whose logits and labels are rewritten between replays; k
follows the number of ignored labels, which changes with them."""
import torch

import ohem_ref as R
from deeplearning_mpi_amd.ops import OHEMCrossEntropyLoss
from deeplearning_mpi_amd.utils.graphs import CapturedStep

DEV = "cuda"


def main():
    K = 4
    x = torch.zeros(R.N, R.H, R.W, K, device=DEV).permute(0, 3, 1, 2).requires_grad_(True)
    y = torch.zeros(R.N, R.H, R.W, dtype=torch.int64, device=DEV)
    one, crit = torch.ones((), device=DEV), OHEMCrossEntropyLoss(keep_ratio=0.25, thresh=0.7)

    def step():
        loss = crit(x, y)
        return loss, torch.autograd.grad(loss, x, one)[0], crit.last_stats["k"]

    captured = CapturedStep(step, warmup=1, inputs=(x, y))
    equal, ks = 0, set()
    for i in range(4):                      # one eager warm-up call, the capture, two replays
        xc, yc, _ = R.softmax_inputs(K, 20 + i)
        yc[1, : 2 * i] = -100               # another number of ignored labels every time
        with torch.no_grad():
            captured.set_inputs(xc.to(DEV).permute(0, 3, 1, 2), yc.to(DEV))
        loss, grad, k = (t.clone() for t in captured())
        for _ in range(2):                  # two eager runs
            el, eg, ek = step()
            assert torch.equal(loss, el) and torch.equal(grad, eg) and torch.equal(k, ek), i
        nv = int(((yc >= 0) & (yc < K)).sum())
        assert k.item() == -(-nv // 4) and torch.isfinite(loss) and float(grad.abs().sum()) > 0
        ks.add(k.item())
        equal += captured.graph is not None and i >= 2
    assert captured.graph is not None, captured.capture_error
    assert len(ks) == 4
    print(f"replays equal eager: {equal}")


if __name__ == "__main__":
    main()
