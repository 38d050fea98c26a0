"""Back-optimisation inference of the PICNNs: unrolled momentum gradient descent on y.

The reference's second inference method (multi-label-cls/icnn-back.py:120-133, completion/icnn.back.py:136-147) runs
n_iter steps of
    v_{k+1} = mu v_k - lr dE/dy(x, y_k),    y_{k+1} = y_k - mu v_k + (1+mu) v_{k+1}       (v_0 = 0)
inside the graph and trains by differentiating through them.  `solve` runs the loop on the device (be_gd.hip through
icnn_be_fc_gd / icnn_be_conv_gd), bit-identical to a loop of model.fg plus the float32 update; the training gradient through
the unroll is train.unrolled_grad, which needs the trajectory y_0 .. y_{K-1} and `coefficients`.

Reference defaults: multi-label lr 0.01, momentum 0.3, nIter 30, y0 = 0.5; completion lr 0.01, momentum 0.9, nGdIter 30,
y0 = meanY.
"""
import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib


def coefficients(n_iter: int, lr: float, momentum: float) -> np.ndarray:
    """dy_K / dg_k of the recurrence, k = 0 .. K-1 (float64): -lr S_{K-k} with S_m = 1 + mu + ... + mu^m.  The adjoint of y
    is the same at every step (E is piecewise linear in y), so the parameter gradient of L(y_K) is
    sum_k grad_theta <dE/dy(x, y_k), coefficients[k] * dL/dy_K>."""
    K = int(n_iter)
    if K < 1:
        raise ValueError("n_iter must be >= 1, got %d" % K)
    lr, mu = float(lr), float(momentum)
    S = np.cumsum(mu ** np.arange(K + 1, dtype=np.float64))          # S[m] = 1 + mu + ... + mu^m
    return -lr * S[K - np.arange(K)]


def solve(model, ctx: torch.Tensor, y0, n_iter: int, lr: float, momentum: float, trajectory: bool = False,
          energy: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """n_iter steps of momentum GD on y from y0 for every sample of `ctx` (the model's x-only context [B, ctx_width]).

    y0: a scalar, an [n] row or a [B, n] array / tensor (a ConvModel also takes images [B, H, W, 1]); rounded to float32 on
    entry like a feed.  Returns (y, traj, energy): y float64 [B, n] = y_K (float32 values); traj float64 [B, n_iter, n] =
    y_0 .. y_{K-1} when `trajectory`, else None; energy float32 [B] = E(y_K) when `energy`, else None.  Enqueued on the
    current stream without any host synchronisation (capturable in a CUDA graph when y0 is a scalar or a device tensor)."""
    spec, dev = model.spec, model.device
    n = spec.n_labels
    K = int(n_iter)
    assert ctx.dtype == torch.float32 and ctx.is_contiguous() and ctx.dim() == 2 and ctx.shape[1] == spec.ctx_width
    B = ctx.shape[0]
    if torch.is_tensor(y0):
        y0 = y0.to(dev, torch.float64)
    elif np.ndim(y0) == 0:                     # a scalar start (the multi-label scripts' 0.5): no host-to-device copy
        y0 = torch.full((B, n), float(y0), dtype=torch.float64, device=dev)
    else:
        y0 = torch.as_tensor(np.asarray(y0, np.float64), device=dev)
    if y0.dim() > 2:
        y0 = y0.reshape(y0.shape[0], -1)       # conv images [B, H, W, 1]
    y0 = y0.expand(B, n).contiguous()
    y = torch.empty(B, n, dtype=torch.float64, device=dev)
    traj = torch.empty(B, K, n, dtype=torch.float64, device=dev) if trajectory else None
    f = torch.empty(B, dtype=torch.float32, device=dev) if energy else None
    ws = torch.empty(max(int(model._lib.icnn_be_gd_workspace_bytes(B, n)), 1), dtype=torch.uint8, device=dev)
    model.reserve(B)
    entry = model.gd_entry
    _lib.check(getattr(model._lib, entry)(
        C.byref(model.c_model), ctx.data_ptr(), y0.data_ptr(), B, K, float(lr), float(momentum), y.data_ptr(),
        None if traj is None else traj.data_ptr(), None if f is None else f.data_ptr(), ws.data_ptr(), model._stream()),
        entry)
    return y, traj, f
