"""Recorded bits of the segmentation losses (csrc/kernels/pixel_ce.hip, seg_dice.hip, pixel_softmax.h).

The other GPU tests compare against fp64 torch with a 1e-4 tolerance; they do not see a changed summation
order or a product and sum newly contracted into an fma.  This one does: for every case it calls the
NativeBackend methods (pixel_ce_fwd / bwd, pixel_ce_dice_fwd / bwd, bce_dice_fwd / bwd, seg_counts) and
compares a sha256 (16 hex digits, over the bytes in logical NCHW order) of every tensor they return --
loss, lse, den, tab, dlogits, counts -- with tests/fixtures/seg_loss_bits.json.

Inputs come from a CPU torch.Generator with a fixed seed per case and are then copied to the GPU; the
fixture also holds a hash of each case's inputs, so a change of the inputs is reported as such and not as
a change of the kernels.

The cases: three shapes (2 and 3 samples of 17 x 23: a block of the 1-D CE grid spans a sample boundary,
the last tile is partial; 1 x 70 x 70: 20 blocks per sample), K = 2, 3, 4 (registers, 8 / 16 byte vector
access), 5, 21 (LDS tiles, odd H W K: a sample base off 16 bytes in the fused tile kernels), 32, 40, 256
(full and narrower tiles), the NHWC view and plain NCHW, for K = 4, 5 a buffer 4 bytes past a 16-byte
boundary, ignored and out-of-range labels, with and without class weights, three (ce_weight, dice_weight)
settings, go absent and a non-unit scalar; the binary form with hard and soft targets.

``python tests/test_seg_loss_bits_gpu.py --record`` rewrites the fixture.  That is legitimate only when
the numerics are changed on purpose (another summation order, another formula); a refactor, a tuning of
tiles or launch shapes that keeps the arithmetic, or a compiler update must pass against the fixture as it
is.  The fixture notes the hipcc version it was recorded with, for information only.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from deeplearning_mpi_amd.ops.backend import NativeBackend  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "seg_loss_bits.json")

SHAPES = [(2, 17, 23), (3, 17, 23), (1, 70, 70)]
KS = [2, 3, 4, 5, 21, 32, 40, 256]
# (ce_weight, dice_weight, smooth, include_background)
DICE_OPTS = [(1.0, 1.0, 1.0, True), (0.0, 1.0, 1.0, True), (0.7, 1.3, 0.5, False)]
GO = 0.37


def _multiclass_cases():
    out = []
    for shape in SHAPES:
        for K in KS:
            if K == 256 and shape[1:] != (17, 23):
                continue
            for layout in ("nhwc", "nchw") + (("off4",) if K in (4, 5) else ()):
                out.append((shape, K, layout))
    return out


MULTI = _multiclass_cases()
BINARY = [(shape, soft) for shape in [(2, 17, 23), (1, 70, 70)] for soft in (False, True)]


def _multi_id(case):
    (n, h, w), K, layout = case
    return f"multi-{n}x{h}x{w}-K{K}-{layout}"


def _binary_id(case):
    (n, h, w), soft = case
    return f"binary-{n}x{h}x{w}-{'soft' if soft else 'hard'}"


def _seed(cid):
    return int(hashlib.sha256(cid.encode()).hexdigest()[:8], 16)


def _hash(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def _multi_inputs(case):
    """-> x [N, K, H, W] on the GPU in the case's layout, labels, class weights, go (from a CPU generator)."""
    (N, H, W), K, layout = case
    g = torch.Generator().manual_seed(_seed(_multi_id(case)))
    base = torch.randn(N, H, W, K, generator=g)
    y = torch.randint(K, (N, H, W), generator=g)
    y[0, :3] = -100
    y[-1, 5, 7] = K + 3   # out of range: ignored as well
    w = torch.rand(K, generator=g) + 0.5
    if layout == "nhwc":
        x = base.to(DEV).permute(0, 3, 1, 2)
    elif layout == "nchw":
        x = base.permute(0, 3, 1, 2).contiguous().to(DEV)
    else:   # the NHWC view of a buffer that starts 4 bytes past a 16-byte boundary
        flat = torch.empty(base.numel() + 1, device=DEV)
        flat[1:].copy_(base.flatten())
        x = flat[1:].view(N, H, W, K).permute(0, 3, 1, 2)
        assert x.data_ptr() % 16 == 4
    return x, y.to(DEV), w.to(DEV), torch.tensor([GO], device=DEV)


def _run_multi(be, case):
    """-> (hash of the inputs, {name: hash} of every returned tensor)."""
    x, y, w, go = _multi_inputs(case)
    out = {"counts": _hash(be.seg_counts(x, y))}
    for wn, wt in (("", None), ("w", w)):
        loss, lse, den = be.pixel_ce_fwd(x, y, wt)
        out.update({f"ce{wn}.loss": _hash(loss), f"ce{wn}.lse": _hash(lse), f"ce{wn}.den": _hash(den)})
        for gn, gt in (("", None), ("go", go)):
            d = be.pixel_ce_bwd(x, y, lse, den, gt, wt)
            assert d.stride() == x.stride()
            out[f"ce{wn}.dlogits{gn}"] = _hash(d)
        for i, (cw, dw, smooth, bg) in enumerate(DICE_OPTS):
            loss, lse, den, tab = be.pixel_ce_dice_fwd(x, y, wt, -100, cw, dw, smooth, bg)
            p = f"dice{i}{wn}"
            out.update({f"{p}.loss": _hash(loss), f"{p}.lse": _hash(lse), f"{p}.den": _hash(den),
                        f"{p}.tab": _hash(tab)})
            for gn, gt in (("", None), ("go", go)):
                d = be.pixel_ce_dice_bwd(x, y, lse, den, tab, gt, wt, -100, cw)
                assert d.stride() == x.stride()
                out[f"{p}.dlogits{gn}"] = _hash(d)
    return _hash(x) + _hash(y) + _hash(w), out


def _run_binary(be, case):
    (N, H, W), soft = case
    g = torch.Generator().manual_seed(_seed(_binary_id(case)))
    x = torch.randn(N, H, W, generator=g)
    t = torch.rand(N, H, W, generator=g)
    if not soft:
        t = (t > 0.5).float()
    x, t, go = x.to(DEV), t.to(DEV), torch.tensor([GO], device=DEV)
    out = {}
    for i, (bw, dw, smooth, _) in enumerate(DICE_OPTS):
        loss, tab = be.bce_dice_fwd(x, t, bw, dw, smooth)
        out.update({f"bce{i}.loss": _hash(loss), f"bce{i}.tab": _hash(tab)})
        for gn, gt in (("", None), ("go", go)):
            out[f"bce{i}.dlogits{gn}"] = _hash(be.bce_dice_bwd(x, t, tab, gt, bw))
    return _hash(x) + _hash(t), out


@pytest.fixture(scope="module")
def be():
    return NativeBackend(DEV)


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def _compare(cid, got, recorded):
    assert cid in recorded, f"{cid}: not in the fixture"
    inputs, out = got
    rec = recorded[cid]
    assert inputs == rec["inputs"], f"{cid}: the generated inputs differ from the recorded ones (not the kernels)"
    assert sorted(out) == sorted(rec["out"]), f"{cid}: the set of compared tensors changed"
    bad = [k for k in sorted(out) if out[k] != rec["out"][k]]
    assert not bad, f"{cid}: bits changed in {bad}"


@pytest.mark.parametrize("case", MULTI, ids=_multi_id)
def test_multiclass_bits(be, recorded, case):
    _compare(_multi_id(case), _run_multi(be, case), recorded)


@pytest.mark.parametrize("case", BINARY, ids=_binary_id)
def test_binary_bits(be, recorded, case):
    _compare(_binary_id(case), _run_binary(be, case), recorded)


def _hipcc_version():
    try:
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        txt = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in txt.splitlines() if ln.strip()][:2]
    except (OSError, subprocess.SubprocessError):
        return ["unknown"]


def _record():
    be = NativeBackend(DEV)
    cases = {}
    for case in MULTI:
        inputs, out = _run_multi(be, case)
        cases[_multi_id(case)] = {"inputs": inputs, "out": out}
    for case in BINARY:
        inputs, out = _run_binary(be, case)
        cases[_binary_id(case)] = {"inputs": inputs, "out": out}
    doc = {"note": "sha256[:16] of every tensor returned by the segmentation-loss kernels; see "
                   "tests/test_seg_loss_bits_gpu.py for when re-recording is legitimate",
           "hipcc_version": _hipcc_version(), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "cases": cases}
    with open(FIXTURE, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":"), sort_keys=True).replace('},"', '},\n"') + "\n")
    print(f"recorded {len(cases)} cases, {sum(len(c['out']) for c in cases.values())} hashes -> {FIXTURE}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/test_seg_loss_bits_gpu.py --record")
    _record()
