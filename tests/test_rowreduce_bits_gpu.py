"""Recorded bits of the chunked row reductions (csrc/kernels/rowreduce.h) and their clients: the fused
gradient producers outer_dgrad_bn / head_dgrad_bn (head.hip) and maxpool_bwd_bn (pool.hip), and bn_stats,
bn_bwd_reduce and channel_sum (bn.hip).

The fp64 tests of these kernels allow 1e-4 or count roundings; they do not see a product and sum newly
contracted into an fma, or a changed summation order.  This one does: every case calls the binding
directly and compares a sha256 (16 hex digits) of every tensor it returns or writes -- dx and the block
partials, the pool's index bytes -- with tests/fixtures/rowreduce_bits.json.

Inputs come from a CPU torch.Generator with a fixed seed per case, are rounded to the storage type on the
CPU and then copied to the GPU; the fixture also holds a hash of each case's inputs, so a change of the
inputs is reported as such and not as a change of the kernels.

The cases, each in bf16 and fp32:
* outer_dgrad_bn: C = 8, 72 (28 row lanes, 4 idle threads), 2048 (one row per block trip) x M = 1 (most
  blocks empty), 257 (one row past a block multiple of the 64-channel maps), 1031;
* head_dgrad_bn: K = 2, 3, 4 x C = 16, 64 x M = 257, 1031;
* maxpool_bwd_bn, C = 8, 64: 3x3/s2/p1 on 2 x 9 x 7 (two windows per axis, odd extents, clipped windows),
  2x2/s2/p0 on 2 x 8 x 12 with `add` a channel slice (ld = 2C, off = C) and without, 3x3/s1/p1 on 1 x 5 x 6
  (the general window loop);
* bn_stats, bn_bwd_reduce (with and without ymask / x), channel_sum: C = 8, 72, 2048 x M = 1, 37, 1031.

``python tests/test_rowreduce_bits_gpu.py --record`` rewrites the fixture.  That is legitimate only when
the numerics are changed on purpose (another summation order, another formula); a refactor, a tuning of
grids or launch shapes that keeps the arithmetic, or a compiler update must pass against the fixture as it
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
FIXTURE = os.path.join(ROOT, "tests", "fixtures", "rowreduce_bits.json")
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
KP = 8   # row pitch of the head's gradient and weight buffers (K padded to 8)

OUTER = [("outer", C, M, dt) for C in (8, 72, 2048) for M in (1, 257, 1031) for dt in DTYPES]
HEAD = [("head", K, C, M, dt) for K in (2, 3, 4) for C in (16, 64) for M in (257, 1031) for dt in DTYPES]
# (N, H, W, k, stride, pad, add: None / "slice")
POOLS = [(2, 9, 7, 3, 2, 1, None), (2, 8, 12, 2, 2, 0, "slice"), (2, 8, 12, 2, 2, 0, None), (1, 5, 6, 3, 1, 1, None)]
POOL = [("pool", C) + p + (dt,) for C in (8, 64) for p in POOLS for dt in DTYPES]
REDUCE = [("reduce", C, M, dt) for C in (8, 72, 2048) for M in (1, 37, 1031) for dt in DTYPES]
CASES = OUTER + HEAD + POOL + REDUCE


def _id(case):
    return "-".join(str(v) for v in case)


def _seed(cid):
    return int(hashlib.sha256(cid.encode()).hexdigest()[:8], 16)


def _hash(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


class _Gen:
    """Tensors from one seeded CPU generator, rounded to the storage type on the CPU; remembers their hashes."""

    def __init__(self, case):
        self.g = torch.Generator().manual_seed(_seed(_id(case)))
        self.dtype = DTYPES[case[-1]]
        self.seen = []

    def _out(self, t):
        self.seen.append(_hash(t))
        return t.to(DEV)

    def act(self, *shape):
        return self._out(torch.randn(*shape, generator=self.g).to(self.dtype))

    def relu_like(self, *shape):   # a stored ReLU output: positive values and exact zeros
        t = torch.randn(*shape, generator=self.g)
        t[torch.rand(*shape, generator=self.g) < 0.4] = 0.0
        return self._out(t.clamp_min(0.0).to(self.dtype))

    def vec(self, n, lo=0.0, spread=1.0, normal=False):
        t = torch.randn(n, generator=self.g) if normal else torch.rand(n, generator=self.g)
        return self._out(t * spread + lo)

    def inputs(self):
        return "".join(self.seen)


def _mask_vectors(gen, C):
    """scale / shift such that z * scale + shift > 0 for about half of a standard normal z."""
    return gen.vec(C, 0.5), gen.vec(C, 0.0, 0.5, normal=True)


def _run_outer(Cx, case):
    _, C, M, _ = case
    gen = _Gen(case)
    dy, w, z = gen.act(M, KP), gen.act(C, KP), gen.act(M, C)
    sc, sh = _mask_vectors(gen, C)
    dx = torch.full((M, C), 3.0, device=DEV, dtype=gen.dtype)
    part = Cx.outer_dgrad_bn(dy, KP, M, C, w.view(-1), KP, z, sc, sh, dx)
    return gen.inputs(), {"dx": _hash(dx), "part": _hash(part)}


def _run_head(Cx, case):
    _, K, C, M, _ = case
    gen = _Gen(case)
    dl, w, z = gen.act(M, KP), gen.act(C, KP), gen.act(M, C)
    sc, sh = _mask_vectors(gen, C)
    dx = torch.full((M, C), 3.0, device=DEV, dtype=gen.dtype)
    part = Cx.head_dgrad_bn(dl, KP, K, M, C, w.view(-1), KP, z, sc, sh, dx)
    return gen.inputs(), {"dx": _hash(dx), "part": _hash(part)}


def _run_pool(Cx, case):
    _, C, N, H, W, k, s, p, add, _ = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    M, MO = N * H * W, N * OH * OW
    gen = _Gen(case)
    x, dy, z = gen.relu_like(M, C), gen.act(MO, C), gen.act(M, C)
    sc, sh = _mask_vectors(gen, C)
    addbuf = gen.act(M, 2 * C) if add else None
    y = torch.empty(MO, C, device=DEV, dtype=gen.dtype)
    idx = torch.empty(MO * C, dtype=torch.uint8, device=DEV)
    Cx.maxpool_fwd(x, N, H, W, C, C, 0, k, s, p, y, idx, OH, OW, None, None, None, 0, 0)
    dx = torch.full((M, C), 3.0, device=DEV, dtype=gen.dtype)
    part = Cx.maxpool_bwd_bn(dy, idx, N, H, W, C, k, s, p, OH, OW, z, sc, sh, addbuf, 2 * C if add else 0,
                             C if add else 0, dx)
    return gen.inputs(), {"idx": _hash(idx), "dx": _hash(dx), "part": _hash(part)}


def _run_reduce(Cx, case):
    _, C, M, _ = case
    gen = _Gen(case)
    x, dy, ym = gen.act(M, C), gen.act(M, C), gen.relu_like(M, C)
    mean, invstd = gen.vec(C, 0.0, 0.3, normal=True), gen.vec(C, 0.5)
    acc = gen.vec(C, 0.0, 3.0, normal=True)
    nblk = Cx.reduce_blocks(M, C)
    out = {"nblk": str(nblk)}

    def partial():
        return torch.zeros(nblk, 2, C, device=DEV)

    part = partial()
    Cx.bn_stats(x, M, C, C, 0, part, nblk)
    out["bn_stats"] = _hash(part)
    for name, mask, xx in (("bwd", None, x), ("bwd.ymask", ym, x), ("bwd.nox", None, None), ("bwd.ymask.nox", ym, None)):
        part = partial()
        Cx.bn_bwd_reduce(dy, C, 0, mask, C if mask is not None else 0, 0, xx, C if xx is not None else 0, 0, M, C,
                         mean if xx is not None else None, invstd if xx is not None else None, part, nblk)
        out[name] = _hash(part)
    Cx.channel_sum(x, M, C, C, 0, acc)
    out["channel_sum"] = _hash(acc)
    return gen.inputs(), out


RUN = {"outer": _run_outer, "head": _run_head, "pool": _run_pool, "reduce": _run_reduce}


@pytest.fixture(scope="module")
def Cx():
    return NativeBackend(DEV).C


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rowreduce_bits(Cx, recorded, case):
    cid = _id(case)
    assert cid in recorded, f"{cid}: not in the fixture"
    inputs, out = RUN[case[0]](Cx, case)
    rec = recorded[cid]
    assert inputs == rec["inputs"], f"{cid}: the generated inputs differ from the recorded ones (not the kernels)"
    assert sorted(out) == sorted(rec["out"]), f"{cid}: the set of compared tensors changed"
    bad = [k for k in sorted(out) if out[k] != rec["out"][k]]
    assert not bad, f"{cid}: bits changed in {bad}"


def _hipcc_version():
    try:
        hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        txt = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in txt.splitlines() if ln.strip()][:2]
    except (OSError, subprocess.SubprocessError):
        return ["unknown"]


def _record():
    Cx = NativeBackend(DEV).C
    cases = {}
    for case in CASES:
        inputs, out = RUN[case[0]](Cx, case)
        cases[_id(case)] = {"inputs": inputs, "out": out}
    doc = {"note": "sha256[:16] of every tensor written by the row-reduction kernels and the fused gradient "
                   "producers; see tests/test_rowreduce_bits_gpu.py for when re-recording is legitimate",
           "hipcc_version": _hipcc_version(), "device": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "cases": cases}
    with open(FIXTURE, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":"), sort_keys=True).replace('},"', '},\n"') + "\n")
    print(f"recorded {len(cases)} cases, {sum(len(c['out']) for c in cases.values())} hashes -> {FIXTURE}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/test_rowreduce_bits_gpu.py --record")
    _record()
