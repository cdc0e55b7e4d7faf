"""Compute backends of the execution engine.

* :class:`NativeBackend` -- the product path: bf16 NHWC activations, every op is one of our
  gfx950 HIP kernels (``_C``), launched on the current HIP stream (graph-capturable).  With
  ``act_dtype=torch.float32`` the same kernels run instantiated for fp32 storage (fp32 MFMA
  v_mfma_f32_16x16x4_f32 in the GEMMs): the ``--precision fp32`` path.
* :class:`RefBackend` -- fp32 torch reference of exactly the same op set and semantics.  It runs
  on CPU (CPU test-suite, gloo multi-process tests) and is the numerics oracle for the kernels.

Both expose the same methods; the engine (models/*) is written once against this interface.
"""
from __future__ import annotations

import os
import weakref
import struct

import torch
import torch.nn.functional as F

from .act import Act, Deferred


# --------------------------------------------------------------------------------------------
_AUX_STREAMS = {}
_BACKENDS = weakref.WeakSet()   # NativeBackend instances (their aux stream references)


def _new_aux_stream(idx, C, role):
    with torch.cuda.device(idx):
        # a raw HIP stream, not a torch pool stream: if a failed hipGraph capture leaves it stuck in
        # capture mode it is abandoned (replace_poisoned_aux_streams), never handed out again
        st = torch.cuda.ExternalStream(C.create_stream(), device=torch.device("cuda", idx))
        C.set_aux_stream(st.cuda_stream, role)
    return st


def _aux_stream(device, C, role):
    """Auxiliary streams, one per (device, role), shared by every backend instance: role 1 = the
    weight-gradient side stream, role 2 = the residual-branch stream.  The kernels keep a separate
    last-arriver ticket array per role (stream_roles.hip:fin_tickets)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _AUX_STREAMS.get((idx, role))
    if st is None:
        st = _AUX_STREAMS[(idx, role)] = _new_aux_stream(idx, C, role)
    return st


def replace_poisoned_aux_streams() -> int:
    """After a failed hipGraph capture (utils/graphs.py): every auxiliary stream that the capture
    had forked and that HIP left in capture mode is replaced by a fresh one, in the registry, in the
    kernels' role table and in every live backend.  Returns the number replaced."""
    if not _AUX_STREAMS:
        return 0
    from .._ext import native

    C = native()
    n = 0
    for (idx, role), st in list(_AUX_STREAMS.items()):
        if not C.stream_capturing(st.cuda_stream):
            continue
        fresh = _AUX_STREAMS[(idx, role)] = _new_aux_stream(idx, C, role)
        for be in list(_BACKENDS):
            if be._side is st:
                be._side = fresh
            if be._branch is st:
                be._branch = fresh
        n += 1
    return n


def pixel_strides(x: torch.Tensor):
    """(sample, class, pixel) element strides of [N, K, H, W] logits in one of the two layouts the pixel
    kernels address in place -- contiguous NCHW, or an NHWC buffer viewed as NCHW (the engine's
    output) -- else None."""
    N, K, H, W = x.shape
    if x.is_contiguous():
        return K * H * W, H * W, 1
    if x.permute(0, 2, 3, 1).is_contiguous():
        return H * W * K, 1, K
    return None


class NativeBackend:
    name = "native"
    use_side_stream = True     # False: weight gradients on the current stream (A/B)
    use_branch_stream = True   # False: the ResNet downsample branch on the current stream (A/B)
    dt = torch.float32
    pad_cast_calls = 0         # nchw_to_nhwc calls served by the channels-last pad-cast (tests)

    def __init__(self, device, act_dtype=torch.bfloat16):
        from .._ext import native

        if act_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"native activations are bf16 or fp32, got {act_dtype}")
        self.C = native()
        self.device = torch.device(device)
        self.act_dtype = act_dtype
        self.f32 = act_dtype == torch.float32
        # the GEMM operand prologues (deferred BN passes) are instantiated for bf16 only
        self.prologue = not self.f32
        self._cast_cache = {}
        self.held = []   # buffers read on the side stream, dropped at the backward's join (engine.grad_side)
        # parameter-gradient work (weight-gradient GEMMs + split reductions, DDP bucket launches)
        # runs on this side stream, off the data-gradient critical path (models/engine.py:grad_side);
        self._side = _aux_stream(self.device, self.C, 1) if self.use_side_stream \
            else None
        # independent residual branches (the ResNet downsample conv + BN) run on this stream beside
        # the main branch, forward and backward (models/resnet.py:_BlockExec)
        self._branch = _aux_stream(self.device, self.C, 2) \
            if self.use_branch_stream else None
        # The auxiliary streams pay off when kernels are long enough to leave idle CUs beside each
        # other; a launch-bound step (ResNet-18 on 32x32 CIFAR: ~300 kernels of a few us) only pays
        # their per-launch event traffic (measured 31-36k vs 58-60k img/s eager).  The engine turns
        # them on per step when the input has >= aux_min_pixels (N*H*W) pixels
        # (EngineModule.forward; DLMPI_AUX_MIN_PIXELS, default 1M: on for ResNet-50 bs 256 at 224^2 and
        # UNet bs 16 at 512^2, off for CIFAR).
        self.aux_min_pixels = int(os.environ.get("DLMPI_AUX_MIN_PIXELS", str(1 << 20)))
        self.aux_on = True
        _BACKENDS.add(self)

    @property
    def side_stream(self):
        return self._side if self.aux_on else None

    @side_stream.setter
    def side_stream(self, s):
        self._side = s

    @property
    def branch_stream(self):
        return self._branch if self.aux_on else None

    @branch_stream.setter
    def branch_stream(self, s):
        self._branch = s

    # ---------------- conv family ----------------
    # the weight-gradient GEMM consumes ops.act.Deferred operands directly in its operand prologues
    # (bf16); the forward / data-gradient GEMMs take them materialized (one elementwise pass)
    prologue = True

    @staticmethod
    def _pro(op):
        """(source Act, prologue mode, k0, k1, Z buffer, Z ld, Z offset) of a GEMM operand."""
        if not isinstance(op, Deferred):
            return op, 0, None, None, None, 0, 0
        if op.kind == "affine":
            return op.src, 1, op.k0, op.k1, None, 0, 0
        return op.src, 2, op.k0, None, op.z.buf, op.z.ld, op.z.off

    def materialize(self, d) -> Act:
        """The stored form of a Deferred operand (one elementwise pass)."""
        if not isinstance(d, Deferred):
            return d
        src = d.src
        out = Act.empty(src.N, src.H, src.W, src.C, self.act_dtype, src.device)
        if d.kind in ("affine", "bn"):
            self.bn_apply(src, d.k0, d.k1, None, d.kind == "affine", out)
        else:
            self.C.bn_bwd_apply(src.buf, src.ld, src.off, None, 0, 0, d.z.buf, d.z.ld, d.z.off, src.rows, src.C,
                                d.k0, out.buf, None)
        return out

    def conv_mtiles(self, N, H, W, C, K, R, S, stride, pad, pro=0):
        """BN-statistics rows the forward conv will write; pro: 3 = the consumer GEMM of a pending
        residual BN-apply (conv_fwd_bn_apply), else 0."""
        return self.C.conv2d_fwd_mtiles_pro(N, H, W, C, K, R, S, stride, pad, 0, 3 if pro == 3 else 0,
                                            int(self.f32))

    def conv_fwd(self, x, w, K, R, S, stride, pad, y: Act, bias=None, res: Act = None, scale=None,
                 shift=None, relu=False, stats=None, kvalid=0):
        """Returns the number of BN-statistics rows written (stats given).  A Deferred.affine input is
        materialized, except for the <= 4-output 1x1 head, which applies it on the fly."""
        if (isinstance(x, Deferred) and x.kind == "affine" and R == 1 and S == 1 and stride == 1 and pad == 0
                and 0 < kvalid <= 4 and res is None and scale is None and not relu and stats is None
                and not self.f32 and x.C in (16, 32, 64, 128, 256, 512) and self.C.head1x1_on()):
            z = x.src
            # w is the flat [K][1][1][C] compute copy: its row stride is C (w.shape[-1], the whole slice's
            # length, sent every class after the first to weights outside this layer)
            self.C.conv1x1_head_affine(z.buf, z.N, z.H, z.W, z.C, z.ld, z.off, w, z.C, int(kvalid), x.k0,
                                       x.k1, y.buf, y.ld, y.off, bias)
            return 0
        x = self.materialize(x)
        return self.C.conv2d_fwd(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, w, K, R, S, stride, pad, y.buf, y.ld,
                                 y.off, bias, res.buf if res is not None else None,
                                 res.ld if res is not None else 0, res.off if res is not None else 0, scale, shift,
                                 bool(relu), stats, 0, int(kvalid), 0)

    def conv_fwd_bn(self, x, w, K, R, S, stride, pad, z: Act, bias, stats, count, gamma, beta, rm, rv, momentum,
                    eps, scale, shift, save_mean, save_invstd):
        """conv_fwd into z with the BN-statistics epilogue AND the training-BN finalize of those
        statistics (scale / shift / mean / invstd / running stats): the conv, then the column-reduce +
        finalize launch."""
        x = self.materialize(x)
        self.C.conv2d_fwd_bn(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, w, K, R, S, stride, pad, z.buf, z.ld, z.off,
                             bias, stats, 0, None, None, None, 0, 0, float(count), gamma, beta, rm, rv,
                             float(momentum), float(eps), scale, shift, save_mean, save_invstd)

    def conv_fwd_bn_apply(self, xp, w, K, z: Act, bias, stats, count, gamma, beta, rm, rv, momentum, eps, scale,
                          shift, save_mean, save_invstd):
        """conv_fwd_bn (1x1, stride 1) whose input is a pending BN-apply (engine.PendingApply: y =
        relu(z * scale + shift + res), res an Act or a Deferred.bn): the conv's operand prologue computes y,
        uses it and stores it with its ReLU mask bits (pro 3) -- no separate apply pass."""
        x, res = xp.z, xp.res
        rs = rh = None
        if isinstance(res, Deferred):
            assert res.kind == "bn", res
            res, rs, rh = res.src, res.k0, res.k1
        y = xp.y
        self.C.conv2d_fwd_bn_apply(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, w, K, z.buf, z.ld, z.off, bias, stats,
                                   xp.scale, xp.shift, res.buf, res.ld, res.off, rs, rh, y.buf, y.ld, y.off, xp.mbits,
                                   float(count), gamma, beta, rm, rv, float(momentum), float(eps), scale, shift,
                                   save_mean, save_invstd)

    def conv3_pro_ok(self, z: Act, y: Act) -> bool:
        """The fused BN-apply + streaming 3x3 launch applies to this input z / applied output y."""
        return bool(self.C.conv3_pro_ok(z.N, z.H, z.W, z.C, 64, z.ld, z.off, y.ld, y.off, y.ld, y.off))

    def conv3_fwd_bn_apply(self, xp, w, K, z: Act, bias, stats, count, gamma, beta, rm, rv, momentum, eps, scale,
                           shift, save_mean, save_invstd):
        """conv_fwd_bn of a 3x3 / s1 / p1 64 -> 64 conv whose input is a pending BN-apply + ReLU without
        residual (engine.PendingApply): the streaming 3x3 kernel applies it to its staged input tiles and
        stores it to xp.y (each pixel once) -- no separate apply pass.  Falls back to the apply pass +
        conv_fwd_bn where the fused launch does not apply."""
        x, y = xp.z, xp.y
        r = self.C.conv3x3_fwd_bn_apply(x.buf, x.N, x.H, x.W, x.ld, x.off, w, z.buf, z.ld, z.off, bias, stats,
                                        xp.scale, xp.shift, y.buf, y.ld, y.off, float(count), gamma, beta, rm, rv,
                                        float(momentum), float(eps), scale, shift, save_mean, save_invstd)
        if r < 0:
            self.bn_apply(xp.z, xp.scale, xp.shift, None, True, y)
            self.conv_fwd_bn(y, w, K, 3, 3, 1, 1, z, bias, stats, count, gamma, beta, rm, rv, momentum, eps, scale,
                             shift, save_mean, save_invstd)

    def conv_fwd_bnbwd(self, x: Act, w, K, R, S, stride, pad, y: Act, fuse):
        """Forward conv producing the gradient of relu(BN(z)) (fuse = BwdFuse(None, z, None, scale,
        shift)): masked in the epilogue, BN-backward partials [tiles][2][K] returned."""
        z = fuse.z
        return self.C.conv2d_fwd_bnbwd(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, w, K, R, S, stride, pad, y.buf, y.ld,
                                       y.off, z.buf, z.ld, z.off, fuse.scale, fuse.shift)

    def conv_dgrad(self, dy: Act, wT, C, R, S, stride, pad, dx: Act, res: Act = None, fuse=None, colsum=False,
                   bias=None):
        """fuse = BwdFuse(mask, z, z2, scale, shift): dx is the gradient of relu(BN(z) [+ BN2(z2)]);
        the epilogue applies the ReLU mask (y > 0, or z*scale + shift > 0 without a residual) and
        returns BN-backward partials [tiles][2|3][C].  colsum (no fuse): returns per-tile
        {sum dx, sum dx^2} [tiles][2][C] of the stored dx instead.  bias: fp32 [C] added to the
        GEMM result first (the dual 1x1 data gradient's W . k3 term)."""
        m, z, z2, sc, sh, mb = fuse if fuse is not None else (None, None, None, None, None, None)

        def t(a):
            return (a.buf, a.ld, a.off) if a is not None else (None, 0, 0)

        dy = self.materialize(dy)
        return self.C.conv2d_dgrad_pro(dy.buf, dy.N, dy.H, dy.W, dy.C, dy.ld, dy.off, wT, C, R, S, stride, pad, dx.H,
                                       dx.W, dx.buf, dx.ld, dx.off, *t(res), *t(m), *t(z), *t(z2), sc, sh, mb,
                                       bool(colsum and fuse is None), 0, None, None, None, 0, 0, bias)

    def dual_weights(self, wT, C, K, coef):
        """[dy | z] weights of the dual 1x1 data gradient (engine.ConvUnit, dual path): w2 [C][2K] =
        {wT * coef[0], wT * coef[1]} in the storage type, b [C] = wT . coef[2] in fp32."""
        w2 = torch.empty(C, 2 * K, dtype=self.act_dtype, device=self.device)
        b = torch.empty(C, dtype=torch.float32, device=self.device)
        self.C.dual_dgrad_weights(wT, C, K, coef, w2, b)
        return w2, b

    def convT_fwd(self, x: Act, wf, Cout, y: Act, bias=None):
        self.C.convT2x2_fwd(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, wf, Cout, y.buf, y.ld, y.off, bias)

    def wgrad_defer(self, on: bool):
        """Queue weight-gradient split reductions (on) / flush the queue and launch them at once
        again (off); conv_bwd.cpp wgrad_reduce_or_defer."""
        self.C.set_wgrad_defer(bool(on))

    def wgrad_flush(self):
        self.C.wgrad_flush()

    def wgrad_discard(self):
        """Drop the queued reductions of a failed backward and turn deferral off."""
        self.C.wgrad_discard()

    def wgrad_bypass(self, on: bool):
        """Reduce the next weight gradients right away (their consumer reads them next), queue kept."""
        self.C.set_wgrad_bypass(bool(on))

    def conv_wgrad(self, dy, x, R, S, stride, pad, grad, Creal, Ko_real):
        direct = R == 1 and S == 1 and stride == 1 and pad == 0
        if isinstance(dy, Deferred) and isinstance(x, Deferred) or (isinstance(x, Deferred) and not direct):
            x = self.materialize(x)   # (prologue combinations the kernel is not built for: dlmpi_wgrad_pro_ok)
        dy, pa, ca, _, zb, zld, zoff = self._pro(dy)
        x, pb, sb, hb, _, _, _ = self._pro(x)
        assert pa in (0, 2) and pb in (0, 1)
        self.C.conv2d_wgrad_pro(dy.buf, dy.ld, dy.off, dy.C, x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, R, S, stride,
                                pad, dy.H, dy.W, grad, Creal, Ko_real, pa, ca, zb, zld, zoff, pb, sb, hb)

    # ---------------- batch norm ----------------
    def bn_finalize(self, stats, ntiles, C, count, gamma, beta, rm, rv, momentum, eps, scale, shift, save_mean,
                    save_invstd):
        self.C.bn_finalize(stats, ntiles, C, float(count), gamma, beta, rm, rv, float(momentum), float(eps), scale,
                           shift, save_mean, save_invstd)

    def bn_stats(self, x: Act):
        nblk = self.C.reduce_blocks(x.rows, x.C)
        part = torch.empty(nblk, 2, x.C, dtype=torch.float32, device=x.device)
        self.C.bn_stats(x.buf, x.rows, x.C, x.ld, x.off, part, nblk)
        return part, nblk

    def bn_apply(self, x: Act, scale, shift, res, relu, y: Act, mbits=None):
        """res: an Act, or a Deferred.bn residual (applied on the fly, never materialised)."""
        rs = rh = None
        if isinstance(res, Deferred):
            assert res.kind == "bn", res
            res, rs, rh = res.src, res.k0, res.k1
        self.C.bn_apply(x.buf, x.ld, x.off, x.rows, x.C, scale, shift, res.buf if res is not None else None,
                        res.ld if res is not None else 0, res.off if res is not None else 0, bool(relu), y.buf, y.ld,
                        y.off, mbits, rs, rh)

    def bn_bwd_deferred(self, dy: Act, x: Act, mean, invstd, gamma, dgamma, dbeta, pre, k2=1) -> Deferred:
        """BN backward from the producer's fused partials (``pre``): finalize only (dgamma, dbeta and
        the apply coefficients); dz stays a Deferred operand of the unit's wgrad / dgrad GEMMs."""
        coef = torch.empty(3, x.C, dtype=torch.float32, device=x.device)
        self.C.bn_bwd_finalize_fused(pre, k2, x.C, float(x.rows), gamma, mean, invstd, dgamma, dbeta, coef)
        return Deferred.bnbwd(dy, x, coef)

    def bn_bwd(self, dy: Act, ymask: Act, x: Act, mean, invstd, gamma, dgamma, dbeta, dx: Act, dyr_out: Act = None,
               pre=None, k2=1):
        M, Cc = x.rows, x.C
        coef = torch.empty(3, Cc, dtype=torch.float32, device=x.device)
        if pre is not None:   # partials {sum dyr, sum dyr*z} came from the producer's dgrad epilogue
            assert ymask is None
            self.C.bn_bwd_finalize_fused(pre, k2, Cc, float(M), gamma, mean, invstd, dgamma, dbeta, coef)
        else:
            nblk = self.C.reduce_blocks(M, Cc)
            part = torch.empty(nblk, 2, Cc, dtype=torch.float32, device=x.device)
            self.C.bn_bwd_reduce(dy.buf, dy.ld, dy.off, ymask.buf if ymask is not None else None,
                                 ymask.ld if ymask is not None else 0, ymask.off if ymask is not None else 0, x.buf,
                                 x.ld, x.off, M, Cc, mean, invstd, part, nblk)
            self.C.bn_bwd_finalize(part, nblk, Cc, float(M), gamma, mean, invstd, dgamma, dbeta, coef)
        assert dx.ld == Cc and dx.off == 0
        if dyr_out is not None:
            assert dyr_out.ld == Cc and dyr_out.off == 0
        self.C.bn_bwd_apply(dy.buf, dy.ld, dy.off, ymask.buf if ymask is not None else None,
                            ymask.ld if ymask is not None else 0, ymask.off if ymask is not None else 0, x.buf, x.ld,
                            x.off, M, Cc, coef, dx.buf, dyr_out.buf if dyr_out is not None else None)

    def channel_sum(self, x: Act, out_acc):
        self.C.channel_sum(x.buf, x.rows, x.C, x.ld, x.off, out_acc)

    # ---------------- pooling / layout ----------------
    def maxpool_fwd(self, x: Act, k, s, p, y: Act, bn=None, store: Act = None):
        """bn = (scale, shift): pool relu(x * scale + shift) -- a BN-apply + ReLU fused into the pool;
        store (2x2 / s2 only): also write that applied input there (the BN-apply's own output)."""
        idx = torch.empty(y.rows * y.C, dtype=torch.uint8, device=x.device)
        assert y.ld == y.C and y.off == 0
        sc, sh = bn if bn is not None else (None, None)
        self.C.maxpool_fwd(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, k, s, p, y.buf, idx, y.H, y.W, sc, sh,
                           store.buf if store is not None else None, store.ld if store is not None else 0,
                           store.off if store is not None else 0)
        return idx

    def maxpool_bwd(self, dy: Act, idx, x: Act, k, s, p, dx: Act, add: Act = None, fuse=None):
        """fuse = BwdFuse(None, z, scale=, shift=): dx is the gradient of relu(BN(z)); it is written
        masked and the BN-backward partials are returned (for bn_bwd(pre=...)).  add: a second
        gradient of the pool input, summed in before the mask."""
        if fuse is not None:
            assert fuse.scale is not None and dx.ld == dx.C and fuse.z.ld == fuse.z.C
            assert dy.ld == dy.C and dy.off == 0 and dx.off == 0 and fuse.z.off == 0
            return self.C.maxpool_bwd_bn(dy.buf, idx, x.N, x.H, x.W, x.C, k, s, p, dy.H, dy.W, fuse.z.buf,
                                         fuse.scale, fuse.shift, add.buf if add is not None else None,
                                         add.ld if add is not None else 0, add.off if add is not None else 0,
                                         dx.buf)
        self.C.maxpool_bwd(dy.buf, idx, x.N, x.H, x.W, x.C, k, s, p, dy.H, dy.W, add.buf if add is not None else None,
                           add.ld if add is not None else 0, add.off if add is not None else 0, dx.buf, dx.ld, dx.off)

    def outer_dgrad_bn(self, dy: Act, wT, ldw, dx: Act, fuse):
        """Data gradient of a 1x1 conv with one output channel: dx[m, c] = dy[m, 0] * wT[c * ldw],
        as the masked gradient of relu(BN(z)) (fuse = BwdFuse(None, z, None, scale, shift)); returns
        the BN-backward partials [blocks][2][C]."""
        assert fuse.scale is not None and fuse.z2 is None and fuse.mask is None and fuse.mbits is None
        assert dx.ld == dx.C and dx.off == 0 and fuse.z.ld == fuse.z.C and fuse.z.off == 0
        return self.C.outer_dgrad_bn(dy.buf[:, dy.off:], dy.ld, dx.rows, dx.C, wT, ldw, fuse.z.buf, fuse.scale,
                                     fuse.shift, dx.buf)

    def head_dgrad_bn(self, dl: Act, K, wT, ldw, dx: Act, fuse):
        """outer_dgrad_bn for a 1x1 conv with K = 2..4 output channels (the multi-class head):
        dx[m, c] = sum_k dl[m, k] * wT[c * ldw + k], masked by relu(BN(z)); BN-backward partials."""
        assert fuse.scale is not None and fuse.z2 is None and fuse.mask is None and fuse.mbits is None
        assert dx.ld == dx.C and dx.off == 0 and fuse.z.ld == fuse.z.C and fuse.z.off == 0 and dl.off == 0
        return self.C.head_dgrad_bn(dl.buf, dl.ld, int(K), dx.rows, dx.C, wT, ldw, fuse.z.buf, fuse.scale, fuse.shift,
                                    dx.buf)

    def avgpool_fwd(self, x: Act, y: Act):
        self.C.avgpool_fwd(x.buf, x.N, x.H * x.W, x.C, y.buf)

    def avgpool_bwd(self, dy: Act, dx: Act):
        self.C.avgpool_bwd(dy.buf, dx.N, dx.H * dx.W, dx.C, dx.buf)

    def nchw_to_nhwc(self, x: torch.Tensor, Cpad) -> Act:
        N, Cc, H, W = x.shape
        if Cc > 1 and x.permute(0, 2, 3, 1).is_contiguous():
            # channels-last already (the pixel loss's gradient of the engine's own logits): pad + cast
            # in one launch instead of a copy to NCHW and the transpose back.  Keyed on the layout alone,
            # so a channels-last model input (or a contiguous [N, C, 1, 1] one) comes here as well: the
            # same values from another kernel, and pad_cast_calls counts those calls too.
            x = x.to(self.dt)
            y = Act.empty(N, H, W, Cpad, self.act_dtype, x.device)
            self.C.nhwc_pad_cast(x.permute(0, 2, 3, 1), N * H * W, Cc, Cpad, y.buf)
            self.pad_cast_calls += 1
            return y
        x = x.contiguous().to(self.dt)
        y = Act.empty(N, H, W, Cpad, self.act_dtype, x.device)
        self.C.nchw_to_nhwc(x, N, Cc, H, W, Cpad, y.buf)
        return y

    def s2d(self, x: torch.Tensor, pad, U, V, CS) -> Act:
        """2x2 space-to-depth of the zero-padded NCHW image -> [N, U, V, 4*CS] NHWC."""
        N, Cc, H, W = x.shape
        x = x.contiguous().to(self.dt)
        y = Act.empty(N, U, V, 4 * CS, self.act_dtype, x.device)
        self.C.s2d_nchw(x, N, Cc, H, W, pad, U, V, CS, y.buf)
        return y

    def upsample_fwd(self, x: Act, y: Act):
        self.C.upsample2x_fwd(x.buf, x.N, x.H, x.W, x.C, x.ld, x.off, y.buf, y.ld, y.off)

    def upsample_bwd(self, dy: Act, dx: Act):
        assert dx.ld == dx.C and dx.off == 0
        self.C.upsample2x_bwd(dy.buf, dx.N, dx.H, dx.W, dx.C, dy.ld, dy.off, dx.buf)

    # ---------------- weights ----------------
    def cast_weights(self, entries, total, dst_flat):
        """entries: list of (src fp32 tensor view, dst offset, dims[4], valid[4], src strides[4])."""
        key = (id(entries), len(entries), dst_flat.data_ptr())
        ent = self._cast_cache.get(key)
        if ent is None or ent[0] is not entries:
            blob = bytearray()
            base, esz = dst_flat.data_ptr(), dst_flat.element_size()
            assert dst_flat.dtype == self.act_dtype
            bmap = []
            for k, (src, doff, d, v, st) in enumerate(entries):
                blob += struct.pack("<QQ4i4i4qq", src.data_ptr(), base + esz * doff, *d, *v, *st, doff)
                # ~one block per 4096 destination elements (one 64x64 tile of the transpose path)
                nb = max(1, min(1024, -(-d[0] * d[1] * d[2] * d[3] // 4096)))
                bmap += [(k, j, nb, 0) for j in range(nb)]
            dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.device)
            bm = torch.tensor(bmap, dtype=torch.int32).to(self.device)
            self._cast_cache[key] = ent = (entries, dev, bm)
        self.C.cast_weights(ent[1], ent[2], self.f32)

    # ---------------- losses / eval ----------------
    def ce_fwd(self, logits, labels):
        N, K = logits.shape
        loss_rows = torch.empty(N, dtype=torch.float32, device=logits.device)
        lse = torch.empty(N, dtype=torch.float32, device=logits.device)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        self.C.softmax_ce_fwd(logits, logits.stride(0), labels, N, K, loss_rows, lse, loss)
        return loss, lse

    def ce_bwd(self, logits, labels, lse, go):
        N, K = logits.shape
        d = torch.empty(N, K, dtype=torch.float32, device=logits.device)
        self.C.softmax_ce_bwd(logits, logits.stride(0), labels, lse, N, K, K, go, 1.0 / N, d)
        return d

    def cls_ce_fwd(self, logits, labels, weight=None, ignore_index=-100, label_smoothing=0.0, labels_b=None,
                   lam=None):
        """Classification cross-entropy with weight / ignore_index / label smoothing and mixed targets
        (ops/losses.py cross_entropy): logits fp32 [N, K] with unit column stride -> (loss, lse [N], rows [N, 3] =
        per-row {numerator, denominator, S_n}, den [1])."""
        N, K = logits.shape
        lse = torch.empty(N, dtype=torch.float32, device=logits.device)
        rows, loss, den = lse.new_empty(N, 3), lse.new_empty(()), lse.new_empty(1)
        self.C.cls_ce_fwd(logits, logits.stride(0) if N > 1 else K, labels, labels_b, lam, weight, N, K,
                          int(ignore_index), float(label_smoothing), lse, rows, loss, den)
        return loss, lse, rows, den

    def cls_ce_bwd(self, logits, labels, lse, rows, den, go, weight=None, ignore_index=-100, label_smoothing=0.0,
                   labels_b=None, lam=None):
        N, K = logits.shape
        d = torch.empty(N, K, dtype=torch.float32, device=logits.device)
        self.C.cls_ce_bwd(logits, logits.stride(0) if N > 1 else K, labels, labels_b, lam, weight, N, K,
                          int(ignore_index), float(label_smoothing), lse, rows, den, go, d)
        return d

    def _pixel_fwd_out(self, logits):   # what every pixel-loss forward fills: lse [N*H*W], loss (scalar), den [1]
        lse = torch.empty(logits.numel() // logits.shape[1], dtype=torch.float32, device=logits.device)
        return lse, lse.new_empty(()), lse.new_empty(1)

    def _pixel_dlogits(self, logits):   # the gradient's buffer, in the strides of the logits
        d = torch.empty_like(logits)   # dense input: same strides
        assert d.stride() == logits.stride(), (d.stride(), logits.stride())
        return d

    def pixel_ce_fwd(self, logits, labels, weight=None, ignore_index=-100):
        """logits fp32 [N, K, H, W] in one of the two native layouts (pixel_strides), labels int64
        [N, H, W] -> (loss, per-pixel logsumexp [N*H*W], sum of the kept pixels' weights)."""
        N, K, H, W = logits.shape
        lse, loss, den = self._pixel_fwd_out(logits)
        st = pixel_strides(logits)
        self.C.pixel_ce_fwd(logits, *st, N, K, H * W, labels, int(ignore_index), weight, lse, loss, den)
        return loss, lse, den

    def pixel_ce_bwd(self, logits, labels, lse, den, go, weight=None, ignore_index=-100):
        """dlogits in the strides of logits, scaled by go / den on the device."""
        N, K, H, W = logits.shape
        d = self._pixel_dlogits(logits)
        self.C.pixel_ce_bwd(logits, *pixel_strides(logits), N, K, H * W, labels, int(ignore_index), weight, lse, go,
                            den, d)
        return d

    def seg_counts(self, logits, labels, ignore_index=-100):
        """int64 [N, K, 3]: per sample and class {|pred = c and target = c|, |pred = c|, |target = c|}."""
        N, K, H, W = logits.shape
        out = torch.empty(N, K, 3, dtype=torch.int64, device=logits.device)
        self.C.seg_counts(logits, *pixel_strides(logits), N, K, H * W, labels, int(ignore_index), out)
        return out

    def pixel_ce_dice_fwd(self, logits, labels, weight=None, ignore_index=-100, ce_weight=1.0, dice_weight=1.0,
                          smooth=1.0, include_background=True):
        """pixel_ce_fwd with the soft Dice fused in (seg_dice.hip): loss = ce_weight * CE + dice_weight * Dice
        -> (loss, lse [N*H*W], CE denominator, the Dice gradient's table [N, K, 2]); no host sync."""
        N, K, H, W = logits.shape
        lse, loss, den = self._pixel_fwd_out(logits)
        tab = torch.empty(N, K, 2, dtype=torch.float32, device=logits.device)
        self.C.pixel_ce_dice_fwd(logits, *pixel_strides(logits), N, K, H * W, labels, int(ignore_index), weight,
                                 float(ce_weight), float(dice_weight), float(smooth), bool(include_background), lse,
                                 loss, den, tab)
        return loss, lse, den, tab

    def pixel_ce_dice_bwd(self, logits, labels, lse, den, tab, go, weight=None, ignore_index=-100, ce_weight=1.0):
        """dlogits of pixel_ce_dice_fwd's loss in the strides of logits, scaled by go on the device."""
        N, K, H, W = logits.shape
        d = self._pixel_dlogits(logits)
        self.C.pixel_ce_dice_bwd(logits, *pixel_strides(logits), N, K, H * W, labels, int(ignore_index), weight, lse,
                                 go, den, tab, float(ce_weight), d)
        return d

    def bce_dice_fwd(self, logits, target, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
        """logits, target fp32 contiguous [N, H, W] -> (bce_weight * BCE + dice_weight * Dice, table [N, 2])."""
        N = logits.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        tab = torch.empty(N, 2, dtype=torch.float32, device=logits.device)
        self.C.bce_dice_fwd(logits, target, N, logits[0].numel(), float(bce_weight), float(dice_weight),
                            float(smooth), loss, tab)
        return loss, tab

    def bce_dice_bwd(self, logits, target, tab, go, bce_weight=1.0):
        d = torch.empty_like(logits, memory_format=torch.contiguous_format)
        self.C.bce_dice_bwd(logits, target, logits.shape[0], logits[0].numel(), go, tab, float(bce_weight), d)
        return d

    def bce_fwd(self, logits, target):
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        self.C.bce_fwd(logits, 1, target, logits.numel(), loss)
        return loss

    def bce_bwd(self, logits, target, go):
        d = torch.empty_like(logits, memory_format=torch.contiguous_format)
        self.C.bce_bwd(logits, 1, target, logits.numel(), go, 1.0 / logits.numel(), d)
        return d

    def argmax_correct(self, logits, labels):
        c = torch.zeros(1, dtype=torch.int32, device=logits.device)
        self.C.argmax_correct(logits, logits.stride(0), labels, logits.shape[0], logits.shape[1], c)
        return c

    def dice(self, logits, target):
        N = target.shape[0]
        out = torch.empty(N, dtype=torch.float32, device=logits.device)
        self.C.dice(logits, 1, target, N, target[0].numel(), out)
        return out

    # ---------------- optimizers ----------------
    def sgd(self, p, g, m, lr, momentum, dampening, wd, nesterov, first, skip_flag=None):
        self.C.sgd_step(p, g, m, lr, momentum, dampening, wd, nesterov, first, skip_flag)

    def adam(self, p, g, m, v, lr, b1, b2, eps, wd, adamw, bc1, bc2, clip=None, tstep=None, clip_writeback=False):
        self.C.adam_step(p, g, m, v, lr, b1, b2, eps, wd, adamw, bc1, bc2, clip, tstep, bool(clip_writeback))

    def grad_norm(self, g, max_norm, norm_out, coef_out):
        self.C.grad_norm(g, max_norm, norm_out, coef_out)

    def scale_(self, x, coef):
        self.C.scale_(x, coef)

    # layer-wise optimizers (csrc/kernels/optim_layerwise.hip): two chunk-indexed passes over the flat
    # buffers with seg_finish between them.  plan: the optimizer's tables for these buffers
    # (seg = Segments, flags, tab, partial); step: device count of the updates applied so far
    def lars(self, p, g, m, plan, step, skip_flag, lr, momentum, wd, nesterov, tc, eps, sched):
        s = plan.seg
        kind, warm, total, min_lr, power = sched
        self.C.seg_sumsq(p, g, s.chunks, plan.flags, s.extent, plan.partial)
        self.C.seg_finish(plan.partial, s.chunk_first, plan.flags, plan.tab, step, skip_flag, 0, tc, wd, eps, 0.0, 0.0,
                          kind, lr, warm, total, min_lr, power)
        self.C.lars_update(p, g, m, s.chunks, plan.flags, s.extent, plan.tab, momentum, wd, bool(nesterov))

    def lamb(self, p, g, m, v, plan, step, clip, lr, b1, b2, eps, wd, sched):
        s = plan.seg
        kind, warm, total, min_lr, power = sched
        if not plan.primed:   # new tables (first step, loaded state): the bias corrections of the next update
            self.C.seg_finish(plan.partial, s.chunk_first, plan.flags, plan.tab, step, None, 2, 0.0, wd, eps, b1, b2,
                              kind, lr, warm, total, min_lr, power)
            plan.primed = True
        self.C.lamb_moments(p, g, m, v, s.chunks, plan.flags, s.extent, plan.partial, plan.tab, clip, b1, b2, eps, wd)
        self.C.seg_finish(plan.partial, s.chunk_first, plan.flags, plan.tab, step, None if clip is None else clip[1:2],
                          1, 0.0, wd, eps, b1, b2, kind, lr, warm, total, min_lr, power)
        self.C.lamb_update(p, m, v, s.chunks, plan.flags, s.extent, plan.tab, eps, wd)

    # weight EMA (csrc/kernels/ema.hip): e toward w (and eb toward b, the flat BN statistics) in one launch;
    # state: fp32 [8], the device-side counters and the decision's memory (optim.WeightEMA)
    def ema_update(self, e, w, eb, b, state, skip_flag, counter, every, warmup, decay, advance=True):
        """advance False: the update alone, the state untouched (all but the last of a per-tensor series)."""
        self.C.ema_update(e, w, eb, b, state, skip_flag, counter, int(every), bool(warmup), float(decay),
                          bool(advance))

    def ema_swap(self, a, b, a2=None, b2=None):
        self.C.ema_swap(a, b, a2, b2)

    # ---------------- utilities (per-step glue on our own kernels) ----------------
    def fill_(self, t, v):
        self.C.fill_(t, float(v))

    def add_i64_(self, t, v):
        self.C.add_i64_(t, int(v))

    def gather_(self, dst, src, idx, accumulate=False):
        """dst.view(-1)[i] (+)= src.view(-1)[idx[i]] (idx < 0: zero)."""
        self.C.gather_(dst, src, idx, bool(accumulate))


# --------------------------------------------------------------------------------------------
class RefBackend:
    """fp32 torch reference with identical semantics (CPU tests / numerics oracle)."""

    name = "ref"

    def __init__(self, device="cpu", dtype=torch.float32):
        self.device = torch.device(device)
        self.dt = dtype            # float64 turns the whole engine into an fp64 oracle run
        self.act_dtype = dtype

    @staticmethod
    def _store(y: Act, v_nchw):
        y.nhwc().copy_(v_nchw[:, :y.C].permute(0, 2, 3, 1))

    prologue = False   # Deferred operands are materialized (same values) before each consumer

    def materialize(self, d) -> Act:
        if not isinstance(d, Deferred):
            return d
        src = d.src
        out = Act.empty(src.N, src.H, src.W, src.C, self.act_dtype, src.device)
        if d.kind in ("affine", "bn"):
            self.bn_apply(src, d.k0, d.k1, None, d.kind == "affine", out)
        else:
            c = d.k0.to(self.dt)
            out.nhwc().copy_(c[0] * src.nhwc().to(self.dt) + c[1] * d.z.nhwc().to(self.dt) + c[2])
        return out

    def bn_bwd_deferred(self, dy: Act, x: Act, mean, invstd, gamma, dgamma, dbeta, pre, k2=1) -> Deferred:
        """bn_bwd's result as coefficients: dz = k1*(dy - s1/M - xhat*s2/M) = c0*dy + c1*x + c2."""
        ps = pre.sum(0)
        s1 = ps[0]
        s2 = invstd * (ps[k2] - mean * s1)
        if dbeta is not None:
            dbeta.add_(s1)
        if dgamma is not None:
            dgamma.add_(s2)
        M = x.rows
        k1 = (gamma if gamma is not None else torch.ones_like(mean)) * invstd
        c0 = k1
        c1 = -k1 * invstd * s2 / M
        c2 = -k1 * s1 / M + k1 * mean * invstd * s2 / M
        return Deferred.bnbwd(dy, x, torch.stack([c0, c1, c2]).to(self.dt))

    def conv_mtiles(self, N, H, W, C, K, R, S, stride, pad, pro=False):
        return 1

    def conv_fwd(self, x, w, K, R, S, stride, pad, y: Act, bias=None, res=None, scale=None, shift=None,
                 relu=False, stats=None, kvalid=0):
        x = self.materialize(x)
        wk = w.view(K, R, S, x.C).permute(0, 3, 1, 2).to(self.dt)
        out = F.conv2d(x.nchw().to(self.dt), wk, None, stride, pad)
        if bias is not None:
            out = out + bias.view(1, -1, 1, 1)
        if stats is not None:
            stats.view(-1, 2, K)[0, 0].copy_(out.sum((0, 2, 3)))
            stats.view(-1, 2, K)[0, 1].copy_((out * out).sum((0, 2, 3)))
        if scale is not None:
            out = out * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if res is not None:
            out = out + res.nchw().to(self.dt)
        if relu:
            out = F.relu(out)
        self._store(y, out)

    def conv_fwd_bn(self, x, w, K, R, S, stride, pad, z: Act, bias, stats, count, gamma, beta, rm, rv, momentum,
                    eps, scale, shift, save_mean, save_invstd):
        self.conv_fwd(x, w, K, R, S, stride, pad, z, bias=bias, stats=stats)
        self.bn_finalize(stats, stats.shape[0], K, count, gamma, beta, rm, rv, momentum, eps, scale, shift,
                         save_mean, save_invstd)

    def dual_weights(self, wT, C, K, coef):
        w = wT.reshape(C, K).to(self.dt)
        c = coef.to(self.dt)
        w2 = torch.cat([w * c[0], w * c[1]], 1).to(self.act_dtype)
        return w2, (w * c[2]).sum(1)

    def conv_dgrad(self, dy, wT, C, R, S, stride, pad, dx: Act, res=None, fuse=None, colsum=False, bias=None):
        dy = self.materialize(dy)
        K = dy.C
        wk = wT.view(C, R, S, K).permute(3, 0, 1, 2).to(self.dt)
        g = torch.nn.grad.conv2d_input((dx.N, C, dx.H, dx.W), wk, dy.nchw().to(self.dt), stride, pad)
        if bias is not None:
            g = g + bias.to(self.dt).view(1, -1, 1, 1)
        if res is not None:
            g = g + res.nchw().to(self.dt)
        if fuse is None:
            self._store(dx, g)
            if colsum:
                v = dx.nhwc().to(self.dt)
                return torch.stack([v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))]).unsqueeze(0)
            return None
        m, z, z2, sc, sh, mb = fuse
        if mb is not None:
            g = g * self._unpack_bits(mb, z).permute(0, 3, 1, 2)
        elif m is not None:
            g = g * (m.nchw() > 0)
        else:   # mask recomputed from the BN input, as the forward BN-apply computed y
            keep = (z.nhwc().to(self.dt) * sc + sh) > 0
            g = g * keep.permute(0, 3, 1, 2)
        self._store(dx, g)
        v = dx.nhwc().to(self.dt)
        rows = [v.sum((0, 1, 2)), (v * z.nhwc().to(self.dt)).sum((0, 1, 2))]
        if z2 is not None:
            rows.append((v * z2.nhwc().to(self.dt)).sum((0, 1, 2)))
        return torch.stack(rows).unsqueeze(0)

    def conv_fwd_bn_apply(self, xp, w, K, z: Act, bias, stats, *fin):
        """Reference form of the fused consumer: the pending BN-apply as its own pass, then conv_fwd_bn."""
        self.bn_apply(xp.z, xp.scale, xp.shift, xp.res, xp.relu, xp.y, mbits=xp.mbits)
        self.conv_fwd_bn(xp.y, w, K, 1, 1, 1, 0, z, bias, stats, *fin)

    def conv3_fwd_bn_apply(self, xp, w, K, z: Act, bias, stats, *fin):
        """Reference form of the fused 3x3 consumer (the engine schedule is the same on every backend)."""
        self.bn_apply(xp.z, xp.scale, xp.shift, None, True, xp.y)
        self.conv_fwd_bn(xp.y, w, K, 3, 3, 1, 1, z, bias, stats, *fin)

    def conv_fwd_bnbwd(self, x: Act, w, K, R, S, stride, pad, y: Act, fuse):
        wk = w.view(K, R, S, x.C).permute(0, 3, 1, 2).to(self.dt)
        out = F.conv2d(x.nchw().to(self.dt), wk, None, stride, pad)
        zz = fuse.z.nhwc().to(self.dt)
        keep = (zz * fuse.scale + fuse.shift) > 0
        self._store(y, out * keep.permute(0, 3, 1, 2))
        v = y.nhwc().to(self.dt)
        return torch.stack([v.sum((0, 1, 2)), (v * zz).sum((0, 1, 2))]).unsqueeze(0)

    def convT_fwd(self, x: Act, wf, Cout, y: Act, bias=None):
        Cin = x.C
        wk = wf.view(Cout, 2, 2, Cin).permute(3, 0, 1, 2).to(self.dt)
        out = F.conv_transpose2d(x.nchw().to(self.dt), wk, bias, stride=2)
        self._store(y, out)

    def wgrad_defer(self, on: bool):
        pass

    def wgrad_flush(self):
        pass

    def wgrad_discard(self):
        pass

    def wgrad_bypass(self, on: bool):
        pass

    def conv_wgrad(self, dy, x, R, S, stride, pad, grad, Creal, Ko_real):
        dy, x = self.materialize(dy), self.materialize(x)
        Ko, Cc = dy.C, x.C
        gw = torch.nn.grad.conv2d_weight(x.nchw().to(self.dt), (Ko, Cc, R, S), dy.nchw().to(self.dt), stride, pad)
        gw = gw.permute(0, 2, 3, 1)[:Ko_real, :, :, :Creal]
        grad.view(Ko_real, R, S, Creal).add_(gw)

    def bn_finalize(self, stats, ntiles, C, count, gamma, beta, rm, rv, momentum, eps, scale, shift, save_mean,
                    save_invstd):
        s = stats.view(-1, 2, C)[:ntiles].double().sum(0)
        mean = s[0] / count
        var = (s[1] / count - mean * mean).clamp_min(0)
        invstd = 1.0 / torch.sqrt(var + eps)
        g = gamma.double() if gamma is not None else torch.ones_like(mean)
        b = beta.double() if beta is not None else torch.zeros_like(mean)
        sc = (g * invstd).to(self.dt)
        scale.copy_(sc)
        shift.copy_((b - mean * g * invstd).to(self.dt))
        if save_mean is not None:
            save_mean.copy_(mean.to(self.dt))
        if save_invstd is not None:
            save_invstd.copy_(invstd.to(self.dt))
        if rm is not None:
            unb = var * count / (count - 1) if count > 1 else var
            rm.mul_(1 - momentum).add_(momentum * mean.to(self.dt))
            rv.mul_(1 - momentum).add_(momentum * unb.to(self.dt))

    def bn_stats(self, x: Act):
        v = x.nhwc().to(self.dt)
        part = torch.stack([v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))]).unsqueeze(0)
        return part, 1

    def bn_apply(self, x: Act, scale, shift, res, relu, y: Act, mbits=None):
        v = x.nhwc().to(self.dt) * scale + shift
        if isinstance(res, Deferred):   # a BN output applied on the fly (no storage rounding)
            assert res.kind == "bn", res
            v = v + (res.src.nhwc().to(self.dt) * res.k0.to(self.dt) + res.k1.to(self.dt))
        elif res is not None:
            v = v + res.nhwc().to(self.dt)
        if relu:
            v = F.relu(v)
        y.nhwc().copy_(v)
        if mbits is not None:   # bit e of byte (row, g): y[row][8g + e] > 0
            pos = (y.nhwc().reshape(-1, y.C // 8, 8) > 0).to(torch.uint8)
            w = (2 ** torch.arange(8, device=pos.device, dtype=torch.uint8))
            mbits.copy_((pos * w).sum(-1).to(torch.uint8).view(mbits.shape))

    @staticmethod
    def _unpack_bits(mbits, like: Act):
        b = mbits.view(-1, like.C // 8, 1).to(torch.int32)
        bits = (b >> torch.arange(8, device=b.device, dtype=torch.int32)) & 1
        return bits.view(like.N, like.H, like.W, like.C).bool()

    def bn_bwd(self, dy: Act, ymask, x: Act, mean, invstd, gamma, dgamma, dbeta, dx: Act, dyr_out=None, pre=None,
               k2=1):
        g = dy.nhwc().to(self.dt)
        if ymask is not None:
            g = g * (ymask.nhwc() > 0)
        M = x.rows
        xhat = (x.nhwc().to(self.dt) - mean) * invstd
        if pre is not None:
            assert ymask is None
            ps = pre.sum(0)
            s1 = ps[0]
            s2 = invstd * (ps[k2] - mean * s1)
        else:
            s1 = g.sum((0, 1, 2))
            s2 = (g * xhat).sum((0, 1, 2))
        if dbeta is not None:
            dbeta.add_(s1)
        if dgamma is not None:
            dgamma.add_(s2)
        k1 = (gamma if gamma is not None else torch.ones_like(mean)) * invstd
        dx.nhwc().copy_(k1 * (g - s1 / M - xhat * s2 / M))
        if dyr_out is not None:
            dyr_out.nhwc().copy_(g)

    def channel_sum(self, x: Act, out_acc):
        out_acc.add_(x.nhwc().to(self.dt).sum((0, 1, 2)))

    def maxpool_fwd(self, x: Act, k, s, p, y: Act, bn=None, store: Act = None):
        v = x.nchw().to(self.dt)
        if bn is not None:
            v = F.relu(v * bn[0].view(1, -1, 1, 1) + bn[1].view(1, -1, 1, 1)).to(x.dtype).to(self.dt)
        if store is not None:
            self._store(store, v)
        out, idx = F.max_pool2d(v, k, s, p, return_indices=True)
        self._store(y, out)
        return idx

    def maxpool_bwd(self, dy: Act, idx, x: Act, k, s, p, dx: Act, add=None, fuse=None):
        g = torch.ops.aten.max_pool2d_with_indices_backward(dy.nchw().to(self.dt).contiguous(), x.nchw().to(self.dt), [k, k],
                                                            [s, s], [p, p], [1, 1], False, idx)
        if add is not None:
            g = g + add.nchw().to(self.dt)
        if fuse is None:
            self._store(dx, g)
            return None
        zz = fuse.z.nhwc().to(self.dt)
        keep = (zz * fuse.scale + fuse.shift) > 0
        self._store(dx, g * keep.permute(0, 3, 1, 2))
        v = dx.nhwc().to(self.dt)
        return torch.stack([v.sum((0, 1, 2)), (v * zz).sum((0, 1, 2))]).unsqueeze(0)

    def outer_dgrad_bn(self, dy: Act, wT, ldw, dx: Act, fuse):
        """dx[m, c] = dy[m, 0] * wT[c * ldw], ReLU-masked by relu(BN(z)); BN-backward partials."""
        d = dy.nhwc()[..., :1].to(self.dt)
        w = wT.reshape(-1)[::ldw][:dx.C].to(self.dt)
        zz = fuse.z.nhwc().to(self.dt)
        keep = (zz * fuse.scale + fuse.shift) > 0
        dx.nhwc().copy_(d * w * keep)
        v = dx.nhwc().to(self.dt)
        return torch.stack([v.sum((0, 1, 2)), (v * zz).sum((0, 1, 2))]).unsqueeze(0)

    def avgpool_fwd(self, x: Act, y: Act):
        y.nhwc().copy_(x.nhwc().to(self.dt).mean((1, 2), keepdim=True))

    def avgpool_bwd(self, dy: Act, dx: Act):
        dx.nhwc().copy_(dy.nhwc().to(self.dt).expand(dx.N, dx.H, dx.W, dx.C) / (dx.H * dx.W))

    def nchw_to_nhwc(self, x: torch.Tensor, Cpad) -> Act:
        N, Cc, H, W = x.shape
        y = Act.zeros(N, H, W, Cpad, self.dt, x.device)
        y.nhwc()[..., :Cc].copy_(x.permute(0, 2, 3, 1))
        return y

    def s2d(self, x: torch.Tensor, pad, U, V, CS) -> Act:
        N, Cc, H, W = x.shape
        xp = torch.zeros(N, CS, 2 * U, 2 * V, dtype=self.dt, device=x.device)
        hh, ww = min(H, 2 * U - pad), min(W, 2 * V - pad)
        xp[:, :Cc, pad:pad + hh, pad:pad + ww] = x[:, :, :hh, :ww].to(self.dt)
        # [N, CS, U, vh, V, vw] -> [N, U, V, vh, vw, CS]
        y = xp.view(N, CS, U, 2, V, 2).permute(0, 2, 4, 3, 5, 1).reshape(N * U * V, 4 * CS)
        return Act(y.contiguous(), N, U, V, 4 * CS)

    def upsample_fwd(self, x: Act, y: Act):
        out = F.interpolate(x.nchw().to(self.dt), scale_factor=2, mode="bilinear", align_corners=True)
        self._store(y, out)

    def upsample_bwd(self, dy: Act, dx: Act):
        xin = torch.zeros(dx.N, dx.C, dx.H, dx.W, dtype=self.dt, device=dy.device, requires_grad=True)
        with torch.enable_grad():
            out = F.interpolate(xin, scale_factor=2, mode="bilinear", align_corners=True)
            (g,) = torch.autograd.grad(out, xin, dy.nchw().to(self.dt))
        self._store(dx, g)

    def cast_weights(self, entries, total, dst_flat):
        for (src, doff, d, v, st) in entries:
            n = d[0] * d[1] * d[2] * d[3]
            dst = dst_flat[doff:doff + n].view(*d)
            dst.zero_()
            dst[:v[0], :v[1], :v[2], :v[3]].copy_(src.as_strided(tuple(v), tuple(st)))

    def ce_fwd(self, logits, labels):
        lse = torch.logsumexp(logits.to(self.dt), 1)
        loss = F.cross_entropy(logits.to(self.dt), labels)
        return loss, lse

    def ce_bwd(self, logits, labels, lse, go):
        p = torch.exp(logits.to(self.dt) - lse[:, None])
        p[torch.arange(len(labels)), labels] -= 1.0
        return p * (go if go is not None else 1.0) / logits.shape[0]

    def _cls_terms(self, logits, labels, weight, ignore_index, eps, labels_b, lam):
        """The closed form of the classification loss: (x, w [K], q [N, K], D)."""
        x = logits.to(self.dt)
        N, K = x.shape
        a = labels
        b = labels_b if labels_b is not None else labels
        l = lam.to(self.dt).reshape(-1).expand(N) if lam is not None else torch.ones(N, dtype=self.dt, device=x.device)
        w = weight.to(self.dt) if weight is not None else torch.ones(K, dtype=self.dt, device=x.device)
        la = l * self._pix_keep(a, K, ignore_index)
        lb = (1 - l) * self._pix_keep(b, K, ignore_index)
        t = (la[:, None] * F.one_hot(a.clamp(0, K - 1), K) + lb[:, None] * F.one_hot(b.clamp(0, K - 1), K)).to(self.dt)
        q = (1 - eps) * t + (eps / K) * (la + lb)[:, None]
        return x, w, q, (t * w).sum()

    def cls_ce_fwd(self, logits, labels, weight=None, ignore_index=-100, label_smoothing=0.0, labels_b=None,
                   lam=None):
        x, w, q, D = self._cls_terms(logits, labels, weight, ignore_index, label_smoothing, labels_b, lam)
        lse = torch.logsumexp(x, 1)
        wq = w * q
        rows = torch.stack([(wq * (lse[:, None] - x)).sum(1), torch.zeros_like(lse), wq.sum(1)], 1)
        return rows[:, 0].sum() / D, lse, rows, D.reshape(1)

    def cls_ce_bwd(self, logits, labels, lse, rows, den, go, weight=None, ignore_index=-100, label_smoothing=0.0,
                   labels_b=None, lam=None):
        x, w, q, D = self._cls_terms(logits, labels, weight, ignore_index, label_smoothing, labels_b, lam)
        wq = w * q
        d = wq.sum(1, keepdim=True) * torch.exp(x - lse[:, None]) - wq
        d = torch.where(q.sum(1, keepdim=True) != 0, d, torch.zeros_like(d))   # rows without a kept label: exact zeros
        g = (go if go is not None else 1.0) / D
        return d * g if float(D) != 0 else torch.zeros_like(d)

    @staticmethod
    def _pix_keep(labels, K, ignore_index):
        return (labels != ignore_index) & (labels >= 0) & (labels < K)

    def pixel_ce_fwd(self, logits, labels, weight=None, ignore_index=-100):
        x = logits.to(self.dt)
        K = x.shape[1]
        keep = self._pix_keep(labels, K, ignore_index)
        lab = torch.where(keep, labels, torch.full_like(labels, ignore_index))   # out of range: ignored
        w = weight.to(self.dt) if weight is not None else None
        loss = F.cross_entropy(x, lab, weight=w, ignore_index=ignore_index)
        lse = torch.logsumexp(x, 1).reshape(-1)
        wt = w[labels.clamp(0, K - 1)] if w is not None else torch.ones_like(lse).view(labels.shape)
        den = (wt * keep).sum().reshape(1)
        return loss, lse, den

    def pixel_ce_bwd(self, logits, labels, lse, den, go, weight=None, ignore_index=-100):
        x = logits.to(self.dt)
        N, K, H, W = x.shape
        keep = self._pix_keep(labels, K, ignore_index)
        t = labels.clamp(0, K - 1)
        p = torch.exp(x - lse.view(N, 1, H, W))
        p = p - F.one_hot(t, K).permute(0, 3, 1, 2).to(self.dt)
        g = (go if go is not None else 1.0) / den
        if weight is not None:
            g = g * weight.to(self.dt)[t]
        else:
            g = g * torch.ones_like(lse).view(labels.shape)
        d = torch.where(keep.unsqueeze(1), p * g.unsqueeze(1), torch.zeros((), dtype=self.dt, device=x.device))
        out = torch.empty_like(logits, dtype=self.dt)
        out.copy_(d)
        return out

    def seg_counts(self, logits, labels, ignore_index=-100):
        N, K = logits.shape[:2]
        keep = self._pix_keep(labels, K, ignore_index).flatten(1)
        pred = logits.argmax(1).flatten(1)
        t = labels.clamp(0, K - 1).flatten(1)
        cls = torch.arange(K, device=logits.device).view(1, K, 1)
        p = (pred.unsqueeze(1) == cls) & keep.unsqueeze(1)
        g = (t.unsqueeze(1) == cls) & keep.unsqueeze(1)
        return torch.stack([(p & g).sum(2), p.sum(2), g.sum(2)], 2).to(torch.int64)

    def head_dgrad_bn(self, dl: Act, K, wT, ldw, dx: Act, fuse):
        """dx[m, c] = sum_k dl[m, k] * wT[c * ldw + k], ReLU-masked by relu(BN(z)); BN-backward partials."""
        d = dl.nhwc()[..., :K].to(self.dt)
        w = wT.reshape(-1, ldw)[:dx.C, :K].to(self.dt)
        zz = fuse.z.nhwc().to(self.dt)
        keep = (zz * fuse.scale + fuse.shift) > 0
        dx.nhwc().copy_((d @ w.t()) * keep)
        v = dx.nhwc().to(self.dt)
        return torch.stack([v.sum((0, 1, 2)), (v * zz).sum((0, 1, 2))]).unsqueeze(0)

    def _dice_terms(self, I, P, T, smooth, sel, dice_weight):
        """Soft Dice from the per-(sample, class) sums [N, C]: (1 - mean dice over the selected classes, the
        gradient table [N, C, 2] = {A, B} of dice_weight * that loss)."""
        U, num = P + T + smooth, 2 * I + smooth
        cnt = I.shape[0] * sel.sum()
        s = dice_weight / cnt
        tab = torch.stack([-2 * s / U * sel, s * num / (U * U) * sel], 2)
        return 1 - (num / U * sel).sum() / cnt, tab

    def pixel_ce_dice_fwd(self, logits, labels, weight=None, ignore_index=-100, ce_weight=1.0, dice_weight=1.0,
                          smooth=1.0, include_background=True):
        x = logits.to(self.dt)
        N, K, H, W = x.shape
        keep = self._pix_keep(labels, K, ignore_index).unsqueeze(1)
        lse = torch.logsumexp(x, 1)
        p = torch.exp(x - lse.unsqueeze(1)) * keep
        oh = F.one_hot(labels.clamp(0, K - 1), K).permute(0, 3, 1, 2).to(self.dt) * keep
        sel = torch.ones(K, dtype=self.dt, device=x.device)
        if not include_background:
            sel[0] = 0
        dl, tab = self._dice_terms((p * oh).flatten(2).sum(2), p.flatten(2).sum(2), oh.flatten(2).sum(2), smooth, sel,
                                   dice_weight)
        loss = dice_weight * dl
        den = torch.zeros(1, dtype=self.dt, device=x.device)
        if ce_weight != 0:   # a weight of 0 leaves the term out: no NaN from an all-ignored batch
            ce, _, den = self.pixel_ce_fwd(logits, labels, weight, ignore_index)
            loss = loss + ce_weight * ce
        return loss, lse.reshape(-1), den, tab

    def pixel_ce_dice_bwd(self, logits, labels, lse, den, tab, go, weight=None, ignore_index=-100, ce_weight=1.0):
        x = logits.to(self.dt)
        N, K, H, W = x.shape
        keep = self._pix_keep(labels, K, ignore_index).unsqueeze(1)
        t = labels.clamp(0, K - 1)
        p = torch.exp(x - lse.view(N, 1, H, W))
        oh = F.one_hot(t, K).permute(0, 3, 1, 2).to(self.dt)
        go = go if go is not None else 1.0
        g = tab[..., 0].view(N, K, 1, 1) * oh + tab[..., 1].view(N, K, 1, 1)
        d = p * (g - (p * g).sum(1, keepdim=True)) * go
        if ce_weight != 0:
            w = weight.to(self.dt)[t] if weight is not None else torch.ones_like(lse).view(labels.shape)
            d = d + (p - oh) * (w * (ce_weight * go / den)).unsqueeze(1)
        out = torch.empty_like(logits, dtype=self.dt)
        out.copy_(torch.where(keep, d, torch.zeros((), dtype=self.dt, device=x.device)))
        return out

    def bce_dice_fwd(self, logits, target, bce_weight=1.0, dice_weight=1.0, smooth=1.0):
        x, t = logits.to(self.dt).flatten(1), target.to(self.dt).flatten(1)
        p = torch.sigmoid(x)
        sel = torch.ones(1, dtype=self.dt, device=x.device)
        dl, tab = self._dice_terms((p * t).sum(1, keepdim=True), p.sum(1, keepdim=True), t.sum(1, keepdim=True), smooth,
                                   sel, dice_weight)
        loss = dice_weight * dl
        if bce_weight != 0:
            loss = loss + bce_weight * F.binary_cross_entropy_with_logits(x, t)
        return loss, tab.reshape(-1, 2)

    def bce_dice_bwd(self, logits, target, tab, go, bce_weight=1.0):
        x, t = logits.to(self.dt).flatten(1), target.to(self.dt).flatten(1)
        p = torch.sigmoid(x)
        go = go if go is not None else 1.0
        d = p * (1 - p) * (tab[:, :1] * t + tab[:, 1:]) * go
        if bce_weight != 0:
            d = d + (p - t) * (bce_weight * go / x.numel())
        return d.view(logits.shape)

    def bce_fwd(self, logits, target):
        return F.binary_cross_entropy_with_logits(logits.to(self.dt), target.to(self.dt))

    def bce_bwd(self, logits, target, go):
        return (torch.sigmoid(logits.to(self.dt)) - target) * (go if go is not None else 1.0) / logits.numel()

    def argmax_correct(self, logits, labels):
        return (logits.argmax(1) == labels).sum().to(torch.int32).view(1)

    def dice(self, logits, target):
        pred = (logits.reshape(target.shape) > 0).to(self.dt)
        inter = (pred * target).flatten(1).sum(1)
        uni = pred.flatten(1).sum(1) + target.flatten(1).sum(1)
        return torch.where(uni > 0, (2 * inter + 1e-8) / (uni + 1e-8), torch.ones_like(uni))

    def sgd(self, p, g, m, lr, momentum, dampening, wd, nesterov, first, skip_flag=None):
        if skip_flag is not None and float(skip_flag.reshape(-1)[0]) != 0:
            return
        d = g + wd * p if wd != 0 else g.clone()
        if momentum != 0:
            if first:
                m.copy_(d)
            else:
                m.mul_(momentum).add_(d, alpha=1 - dampening)
            d = d + momentum * m if nesterov else m
        p.add_(d, alpha=-lr)

    def adam(self, p, g, m, v, lr, b1, b2, eps, wd, adamw, bc1, bc2, clip=None, tstep=None, clip_writeback=False):
        coef = 1.0
        if clip is not None:
            if float(clip[1]) != 0:
                return
            coef = clip[0]
        if tstep is not None:   # tstep = updates applied so far; advanced only when this one is applied
            t = float(tstep.reshape(-1)[0]) + 1
            bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
            tstep.add_(1)
        gin = g
        g = g * coef
        if clip_writeback and float(coef) != 1.0:   # the clipped gradients stay visible (torch's in-place clip)
            gin.copy_(g)
        if wd != 0:
            if adamw:
                p.mul_(1 - lr * wd)
            else:
                g = g + wd * p
        m.lerp_(g, 1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = v.sqrt() / (bc2 ** 0.5) + eps
        p.addcdiv_(m, denom, value=-lr / bc1)

    def grad_norm(self, g, max_norm, norm_out, coef_out):
        n = g.double().pow(2).sum().sqrt().to(self.dt)
        norm_out.reshape(-1)[0] = n
        coef_out[0] = torch.clamp(max_norm / (n + 1e-6), max=1.0)
        coef_out[1] = 0.0 if torch.isfinite(n) else 1.0
        if coef_out.numel() >= 4:
            coef_out[2] = 1.0
            coef_out[3] = coef_out[1]

    def scale_(self, x, coef):
        x.mul_(coef[0])

    # layer-wise optimizers: a per-tensor loop in the backend's dtype over the same tables (the host lists
    # of plan.seg), writing the same table: tab = [lr, bc1, bc2, skip, grad norm, first, next bc1, next bc2, ratio[T]]
    def lars(self, p, g, m, plan, step, skip_flag, lr, momentum, wd, nesterov, tc, eps, sched):
        s, tab = plan.seg, plan.tab
        views = [(i, slice(o, o + n)) for i, (o, n) in enumerate(zip(s.offsets, s.numels))]
        gn = sum((g[sl].double().pow(2).sum() for _, sl in views), torch.zeros((), dtype=torch.float64,
                                                                               device=g.device)).sqrt()
        tab[4] = gn
        if (skip_flag is not None and float(skip_flag.reshape(-1)[0]) != 0) or not bool(torch.isfinite(gn)):
            tab[3] = 1.0
            return
        done = float(step.reshape(-1)[0])
        lr_t = layerwise_lr(lr, done, sched)
        first = done == 0
        for i, sl in views:
            w, gi = p[sl], g[sl]
            fl = plan.flag_words[i]
            wdi = 0.0 if fl & 1 else wd
            r = 1.0
            if not fl & 2:
                wn, gnorm = w.pow(2).sum().sqrt(), gi.pow(2).sum().sqrt()
                if float(wn) > 0 and float(gnorm) > 0:
                    r = tc * wn / (gnorm + wdi * wn + eps)
            d = (gi + wdi * w) * r
            if momentum != 0:
                mi = m[sl]
                if first:
                    mi.copy_(d)
                else:
                    mi.mul_(momentum).add_(d)
                d = d + momentum * mi if nesterov else mi
            w.add_(d, alpha=-lr_t)
            tab[8 + i] = r
        tab[0], tab[3], tab[5] = lr_t, 0.0, float(first)
        step.add_(1)

    def lamb(self, p, g, m, v, plan, step, clip, lr, b1, b2, eps, wd, sched):
        s, tab = plan.seg, plan.tab
        coef = 1.0
        if clip is not None:
            if float(clip[1]) != 0:
                tab[3] = 1.0
                return
            coef = clip[0].to(g.dtype)
        done = float(step.reshape(-1)[0])
        lr_t = layerwise_lr(lr, done, sched)
        bc1, bc2 = 1 - b1 ** (done + 1), 1 - b2 ** (done + 1)
        for i, (o, n) in enumerate(zip(s.offsets, s.numels)):
            sl = slice(o, o + n)
            w, gi, mi, vi = p[sl], g[sl] * coef, m[sl], v[sl]
            fl = plan.flag_words[i]
            mi.lerp_(gi, 1 - b1)
            vi.mul_(b2).addcmul_(gi, gi, value=1 - b2)
            u = (mi / bc1) / (vi.sqrt() / (bc2 ** 0.5) + eps)
            if wd != 0 and not fl & 1:
                u = u + wd * w
            r = 1.0
            if not fl & 2:
                wn, un = w.pow(2).sum().sqrt(), u.pow(2).sum().sqrt()
                if float(wn) > 0 and float(un) > 0:
                    r = wn / un
            w.sub_(u * (lr_t * r))
            tab[8 + i] = r
        tab[0], tab[1], tab[2], tab[3], tab[5] = lr_t, bc1, bc2, 0.0, float(done == 0)
        tab[6], tab[7] = 1 - b1 ** (done + 2), 1 - b2 ** (done + 2)   # the next update's
        step.add_(1)

    # weight EMA: the decision of ema.hip's ema_decide on host copies of the same state vector, the update in
    # the buffers' dtype (fp64 arenas average in fp64; state[3] then holds omd rounded to fp32)
    def ema_update(self, e, w, eb, b, state, skip_flag, counter, every, warmup, decay, advance=True):
        if not 0.0 <= decay < 1.0 or every < 1:
            raise RuntimeError("ema_update: decay must be in [0, 1) and every >= 1")
        if e.numel() != w.numel() or (eb is None) != (b is None) or (eb is not None and eb.numel() != b.numel()):
            raise RuntimeError("ema_update: mismatched lengths")
        st = state.tolist()
        cnt = float(counter.reshape(-1)[0]) if counter is not None else None
        applied = not (skip_flag is not None and float(skip_flag.reshape(-1)[0]) != 0) and \
            not (cnt is not None and cnt == st[2])
        fire = applied and (st[0] + 1) % every == 0
        omd = 1.0 - (min(decay, (1 + st[1]) / (10 + st[1])) if warmup else decay)
        if fire:
            omd = torch.tensor(omd, dtype=e.dtype).item()
            # the product rounded on its own: add_(alpha=) fuses it in torch's vector loop and not in its tail, so
            # the result would depend on how the elements are split over launches
            e.add_((w - e).mul_(omd))
            if eb is not None and eb.numel():
                eb.add_((b - eb).mul_(omd))
        if not advance:
            return
        if fire:
            state[1] += 1
            state[3] = omd
        if applied:
            state[0] += 1
        if cnt is not None:
            state[2] = cnt
        state[4] = float(fire)

    def ema_swap(self, a, b, a2=None, b2=None):
        for x, y in ((a, b), (a2, b2)):
            if x is not None:
                t = x.clone()
                x.copy_(y)
                y.copy_(t)

    def fill_(self, t, v):
        t.fill_(v)

    def add_i64_(self, t, v):
        t.add_(v)

    def gather_(self, dst, src, idx, accumulate=False):
        d, sv = dst.view(-1)[:idx.numel()], src.reshape(-1)
        v = torch.where(idx >= 0, sv[idx.clamp_min(0)], torch.zeros((), dtype=sv.dtype, device=sv.device))
        if accumulate:
            d.add_(v)
        else:
            d.copy_(v)


def layerwise_lr(base, done, sched):
    """The learning rate of update number ``done`` + 1 (``done`` updates applied so far) under
    sched = (kind, warmup_steps, total_steps, min_lr, power); kind 0 constant, 1 cosine, 2
    polynomial.  seg_finish_kernel computes the same on the device."""
    import math

    kind, warm, total, min_lr, power = sched
    if done < warm:
        return base * (done + 1) / warm
    if kind == 0:
        return base
    q = min(1.0, (done - warm) / max(1.0, total - warm))
    f = 0.5 * (1 + math.cos(math.pi * q)) if kind == 1 else (1 - q) ** power
    return min_lr + (base - min_lr) * f


def make_backend(device, dtype=torch.float32, precision: str = "bf16") -> "NativeBackend | RefBackend":
    """GPU: the native gfx950 kernels with bf16 activations (default) or, ``precision='fp32'`` (the
    apps' ``--precision fp32``), the same kernels instantiated for fp32 activations and weights.
    ``precision='ref'`` on GPU: the torch reference backend in the parameters' dtype (numerics
    oracle, e.g. fp64 against the fp32 kernels).  CPU: the
    reference backend in the parameters' dtype."""
    device = torch.device(device)
    if device.type == "cuda":
        if precision == "ref":
            return RefBackend(device, dtype)
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be bf16 or fp32, got {precision!r}")
        return NativeBackend(device, torch.float32 if precision == "fp32" else torch.bfloat16)
    return RefBackend(device, dtype)
