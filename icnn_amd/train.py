"""Training step of the PICNNs on the device.

    surrogate_grad  the parameter gradient of the reference's surrogate F = c E + <dE/dy, v> over every trainable
                    variable (multi-label-cls/icnn_ebundle.py:148-156; with v absent the RL critic's c-weighted energy,
                    RL/src/icnn.py:90-109): HIP kernels of be_train_fc.hip through icnn_be_fc_surrogate_grad.  For the
                    conv PICNN of the completion experiment (completion/icnn_ebundle.py:129-140) be_train_conv.hip
                    through icnn_be_conv_surrogate_grad.
    TFAdam          tf.train.AdamOptimizer's update rule on device tensors (torch plumbing, not a kernel).

One training step of the multi-label experiment:
    solve -> bundle_entropy.implicit_feed -> surrogate_grad -> TFAdam.step -> picnn.project -> model.repack
and of the completion experiment the same with ConvModel.context, a conv solve and implicit_feed(..., "mse").
"""
import ctypes as C
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib
from .bundle_entropy import ImplicitFeed
from .picnn import CONV_FCS, CONV_LAYERS, ConvModel, ConvSpec, FCModel, FCSpec


def _conv_grad_layout(spec: ConvSpec) -> List[Tuple[str, tuple]]:
    out, cin = [], 1
    for l, (nf, k, s) in enumerate(CONV_LAYERS):
        out += [("u%d/W" % l, (k, k, cin, nf)), ("u%d/b" % l, (nf,)), ("u%d/bn/gamma" % l, (nf,)), ("u%d/bn/beta" % l, (nf,))]
        if l > 0:
            out += [("z%d_zu_u/W" % l, (3, 3, cin, cin)), ("z%d_zu_u/b" % l, (cin,)), ("z%d_zu_proj/W" % l, (k, k, cin, nf))]
        out += [("z%d_yu_u/W" % l, (3, 3, cin, 1)), ("z%d_yu_u/b" % l, (1,)), ("z%d_yu/W" % l, (k, k, 1, nf)),
                ("z%d_y_red/W" % l, (k, k, 1, 1)), ("z%d_y_red/b" % l, (1,)), ("z%d_u/W" % l, (k, k, cin, nf)),
                ("z%d_u/b" % l, (nf,))]
        cin = nf
    flat, fch = spec.flat_dim, CONV_FCS[0]
    out += [("u3/W", (flat, fch)), ("u3/b", (fch,)), ("u3/bn/gamma", (fch,)), ("u3/bn/beta", (fch,)), ("u4/W", (fch, 1)),
            ("u4/b", (1,))]
    prev = flat
    for l, sz in zip((3, 4), CONV_FCS):
        out += [("z%d_zu_u/W" % l, (prev, prev)), ("z%d_zu_u/b" % l, (prev,)), ("z%d_zu_proj/W" % l, (prev, sz)),
                ("z%d_u/W" % l, (prev, sz)), ("z%d_u/b" % l, (sz,))]
        prev = sz
    return out


def grad_layout(spec) -> List[Tuple[str, tuple]]:
    """(name, shape) of every variable of the packed gradient, in the order include/icnn_be.h documents (the order of
    picnn.init_params' keys for an FCSpec, of picnn.init_conv_params' for a ConvSpec)."""
    if isinstance(spec, ConvSpec):
        return _conv_grad_layout(spec)
    L, n, w = len(spec.szs), spec.n_labels, spec.widths
    out = []
    prev = spec.n_features
    for i in range(L):
        out += [("u%d/W" % i, (prev, spec.szs[i])), ("u%d/b" % i, (spec.szs[i],))]
        if i < L - 1 and spec.batchnorm:
            out += [("u%d/bn/gamma" % i, (spec.szs[i],)), ("u%d/bn/beta" % i, (spec.szs[i],))]
        prev = spec.szs[i]
    for i in range(L + 1):
        in_u = spec.n_features if i == 0 else spec.szs[i - 1]
        if i > 0:
            out += [("z%d_zu_u/W" % i, (in_u, w[i - 1])), ("z%d_zu_u/b" % i, (w[i - 1],)),
                    ("z%d_zu_proj/W" % i, (w[i - 1], w[i]))]
        out += [("z%d_yu_u/W" % i, (in_u, n)), ("z%d_yu_u/b" % i, (n,)), ("z%d_yu/W" % i, (n, w[i])),
                ("z%d_u/W" % i, (in_u, w[i])), ("z%d_u/b" % i, (w[i],))]
    return out


def unpack_grad(spec, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Views of the packed gradient under the reference's variable names and [in, out] shapes."""
    out, at = {}, 0
    for name, shape in grad_layout(spec):
        size = int(np.prod(shape))
        out[name] = flat[at:at + size].view(shape)
        at += size
    if at != flat.numel():
        raise ValueError("packed gradient has %d floats, the layout %d" % (flat.numel(), at))
    return out


def grad_floats(model) -> int:
    if isinstance(model, ConvModel):
        return int(model._lib.icnn_be_conv_grad_floats(C.byref(model.c_model), C.byref(model.c_ctx)))
    return int(model._lib.icnn_be_fc_grad_floats(C.byref(model.c_model), C.byref(model.c_ctx)))


def surrogate_grad(model, x: torch.Tensor, feed_or_rows, row_offset=None, F_rows=None, bn_updates=0) -> Dict[str, torch.Tensor]:
    """Gradient of sum_r [ c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r> ] over every trainable variable of `model`,
    keyed like picnn.init_params(spec) -- for a ConvModel like picnn.init_conv_params(spec), x [B, H, W, 1] already
    h-flipped (completion/icnn_ebundle.py:215).

    feed_or_rows: an ImplicitFeed (bundle_entropy.implicit_feed: rows grouped by sample, in sample order), or (y, c) --
    the RL critic, one row per sample and no v -- or (y, v, c) with `row_offset` (int32 [B+1]: rows of sample j are
    row_offset[j] .. row_offset[j+1]-1).  BatchNorm runs over the feed rows, each sample counted once per row, as the
    reference's x_ = fd_xs.  F_rows: optional float32 [R] tensor that receives F_r.  bn_updates = k > 0 also folds those
    BatchNorm statistics k times into model.bn_stats (1: what the reference's train_step does); the gradient is the same.
    Enqueued on the current stream without any host synchronisation (capturable in a CUDA graph)."""
    spec, dev = model.spec, model.device
    conv = isinstance(model, ConvModel)
    x = x.to(dev, torch.float32).contiguous()
    B = x.shape[0]
    if conv:
        assert tuple(x.shape[1:]) == (spec.H, spec.W, 1)
        if getattr(model, "c_ctx", None) is None:
            model.repack_context(model.params)
    else:
        assert x.shape[1] == spec.n_features
    v = None
    if isinstance(feed_or_rows, ImplicitFeed):
        y, v, c = feed_or_rows.y, feed_or_rows.v, feed_or_rows.c
        if row_offset is None:         # rows of sample j are contiguous and in sample order (implicit_feed emits them so)
            sample = feed_or_rows.sample.to(dev, torch.int32).contiguous()
            row_offset = torch.searchsorted(sample, torch.arange(B + 1, dtype=torch.int32, device=dev), out_int32=True)
    elif len(feed_or_rows) == 2:
        y, c = feed_or_rows
        if row_offset is None:
            row_offset = torch.arange(B + 1, dtype=torch.int32, device=dev)
    else:
        y, v, c = feed_or_rows
        if row_offset is None:
            raise ValueError("(y, v, c) rows need row_offset")
    y = torch.as_tensor(y).to(dev, torch.float64).contiguous()
    y = y.view(y.shape[0], -1)                 # conv feeds may come as images [R, H, W, 1]
    c = torch.as_tensor(c).to(dev, torch.float64).contiguous().view(-1)
    if v is not None:
        v = torch.as_tensor(v).to(dev, torch.float64).contiguous()
        v = v.view(v.shape[0], -1)
        assert v.shape == y.shape
    R = y.shape[0]
    assert y.shape == (R, spec.n_labels) and c.shape == (R,)
    row_offset = torch.as_tensor(row_offset).to(dev, torch.int32).contiguous()
    if row_offset.shape != (B + 1,):
        raise ValueError("row_offset has shape %s, the batch needs (%d,)" % (tuple(row_offset.shape), B + 1))
    bn_updates = int(bn_updates)
    if bn_updates < 0:
        raise ValueError("bn_updates must be >= 0, got %d" % bn_updates)
    entry = "icnn_be_conv_surrogate_grad" if conv else "icnn_be_fc_surrogate_grad"
    grad = torch.empty(grad_floats(model), dtype=torch.float32, device=dev)
    if R == 0:
        return unpack_grad(spec, grad.zero_())
    n_work = int(getattr(model._lib, entry + "_work_floats")(C.byref(model.c_model), C.byref(model.c_ctx), B, R))
    if n_work == 0:
        raise ValueError("%s: shape rejected (batch %d, rows %d)" % (entry, B, R))
    work = torch.empty(n_work, dtype=torch.float32, device=dev)
    if F_rows is not None:
        assert F_rows.dtype == torch.float32 and F_rows.shape == (R,) and F_rows.is_contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    mv = model._c_bn()
    _lib.check(getattr(model._lib, entry + "_bn")(
        C.byref(model.c_model), C.byref(model.c_ctx), x.data_ptr(), B, row_offset.data_ptr(), R, y.data_ptr(),
        None if v is None else v.data_ptr(), c.data_ptr(), grad.data_ptr(),
        None if F_rows is None else F_rows.data_ptr(), work.data_ptr(), C.byref(mv), bn_updates, C.c_void_p(stream)), entry)
    return unpack_grad(spec, grad)


class TFAdam:
    """tf.train.AdamOptimizer's update (the reference's optimiser, icnn_ebundle.py:153, RL/src/icnn.py:107):
        t += 1;  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)
        m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  theta -= lr_t m / (sqrt(v) + eps)
    -- eps outside the bias correction, unlike torch.optim.Adam.  `params`: dict name -> tensor, updated in place."""

    def __init__(self, params: Dict[str, torch.Tensor], lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        self.params = params
        self.lr, self.beta1, self.beta2, self.eps = lr, beta1, beta2, eps
        self.t = 0
        self.m = {k: torch.zeros_like(p) for k, p in params.items()}
        self.v = {k: torch.zeros_like(p) for k, p in params.items()}

    @torch.no_grad()
    def step(self, grads: Dict[str, torch.Tensor]):
        self.t += 1
        lr_t = self.lr * math.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        for k, p in self.params.items():
            g = grads[k].to(p.dtype)
            m, v = self.m[k], self.v[k]
            m.mul_(self.beta1).add_(g, alpha=1.0 - self.beta1)
            v.mul_(self.beta2).addcmul_(g, g, value=1.0 - self.beta2)
            p.sub_(lr_t * m / (v.sqrt() + self.eps))
