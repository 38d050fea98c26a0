"""Solver comparison on the device: projected gradient descent on the entropy-scaled objective E(x, y) - H(y), the
objective's traces, and the bundle's lower bound.

The reference compares its solvers in multi-label-cls/ebundle-vs-gd.py and completion/ebundle-iter.py: the bundle-entropy
solve with a callback that records mean(E - H(y)) per iteration, against bamos_opt.pgd.solve_batch on the same objective at
lr 0.1, 0.01 and 0.001 with minIter == maxIter.  bamos_opt is not part of the reference tree, so the PGD iteration is defined
here -- PARITY UNPINNED: from y_0 = clip(y0, lo, hi), n_iter times
    yf      = float64(float32(y_k))                          what the float32 energy is fed
    E, g    = the model's float32 energy and dE/dy at yf     (the operations of model.fg)
    e_k     = float64(E) + sum_j [yf log yf + (1 - yf) log(1 - yf)]
    y_{k+1} = clip(y_k - lr ((float64(g) + log yf) - log(1 - yf)), lo, hi)
in float64.  The scripts start inside the box [1e-6, 1 - 1e-6] (their `proj`), so clipping y0 changes nothing for them and
keeps the logarithms finite.  The stopping rule of solve_batch never fires in those scripts and is not built.

    solve(model, ctx, y0, n_iter, lr)      the loop (be_pgd.hip through icnn_be_fc_pgd / icnn_be_conv_pgd)
    objective(model, ctx, y)               E - H(y) at given points
    bundle_trace(result)                   E - H per iteration of a finished fused bundle solve, without a host round trip
    dual_bound(result)                     the bundle's lower bound of min_y E - H
    gap(model, ctx, result)                objective(y*) - dual_bound: the solve's own duality gap
"""
import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

LO, HI = 1e-6, 1.0 - 1e-6                   # the scripts' proj (ebundle-vs-gd.py:116-117)


def _entry(model):
    entry = getattr(model, "pgd_entry", None)          # stated by the model class, next to gd_entry (picnn.py)
    if entry is None:
        raise TypeError("pgd serves FCModel and ConvModel, not %s" % type(model).__name__)
    return entry


def solve(model, ctx: torch.Tensor, y0, n_iter: int, lr: float, lo: float = LO, hi: float = HI, trace: bool = True,
          final: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """n_iter iterations of PGD on E - H from clip(y0, lo, hi) for every sample of `ctx` (the model's x-only context
    [B, ctx_width]).

    y0: a scalar, an [n] row or a [B, n] array / tensor (a ConvModel also takes images [B, H, W, 1]).  Returns
    (y, obj, obj_final): y float64 [B, n] = y_K; obj float64 [n_iter, B] = e_k, the objective before each update, when
    `trace`, else None; obj_final float64 [B] = e_K from one more evaluation when `final`, else None.  Always n_iter
    iterations; samples are independent.  Enqueued on the current stream without any host synchronisation (capturable in a
    CUDA graph when y0 is a scalar or a device tensor)."""
    spec, dev = model.spec, model.device
    n = spec.n_labels
    K = int(n_iter)
    lr, lo, hi = float(lr), float(lo), float(hi)
    if K < 1:
        raise ValueError("n_iter must be >= 1, got %d" % K)
    if not np.isfinite(lr):
        raise ValueError("lr must be finite, got %r" % lr)
    if not (0.0 < np.float32(lo) and np.float32(hi) < 1.0 and lo < hi):
        raise ValueError("the box needs 0 < float32(lo), float32(hi) < 1 and lo < hi, got [%r, %r]" % (lo, hi))
    if getattr(spec, "action_box", False):
        raise ValueError("pgd.solve does not serve an action_box model")
    entry = _entry(model)
    assert ctx.dtype == torch.float32 and ctx.is_contiguous() and ctx.dim() == 2 and ctx.shape[1] == spec.ctx_width
    B = ctx.shape[0]
    if torch.is_tensor(y0):
        y0 = y0.to(dev, torch.float64)
    elif np.ndim(y0) == 0:                     # a scalar start (the multi-label script's 0.5): no host-to-device copy
        y0 = torch.full((B, n), float(y0), dtype=torch.float64, device=dev)
    else:
        y0 = torch.as_tensor(np.asarray(y0, np.float64), device=dev)
    if y0.dim() > 2:
        y0 = y0.reshape(y0.shape[0], -1)       # conv images [B, H, W, 1]
    y0 = y0.expand(B, n).contiguous()
    y = torch.empty(B, n, dtype=torch.float64, device=dev)
    obj = torch.empty(K, B, dtype=torch.float64, device=dev) if trace else None
    fin = torch.empty(B, dtype=torch.float64, device=dev) if final else None
    ws = torch.empty(max(int(model._lib.icnn_be_pgd_workspace_bytes(B, n)), 1), dtype=torch.uint8, device=dev)
    model.reserve(B)
    _lib.check(getattr(model._lib, entry)(
        C.byref(model.c_model), ctx.data_ptr(), y0.data_ptr(), B, K, lr, lo, hi, y.data_ptr(),
        None if obj is None else obj.data_ptr(), None if fin is None else fin.data_ptr(), ws.data_ptr(), model._stream()),
        entry)
    return y, obj, fin


def entropy_objective(E: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """float64(E) - H(y) per sample for E float32 [B] and y float64 [B, n] on the device (icnn_be_entropy_objective): the
    scripts' `es - entr(x)`, an element whose entropy term is NaN counting 0 like theirs."""
    assert E.dtype == torch.float32 and y.dtype == torch.float64 and y.dim() == 2 and E.shape == (y.shape[0],)
    assert E.is_cuda and y.is_cuda
    E, y = E.contiguous(), y.contiguous()
    B, n = y.shape
    out = torch.empty(B, dtype=torch.float64, device=y.device)
    stream = C.c_void_p(torch.cuda.current_stream(y.device).cuda_stream)
    _lib.check(_lib.load().icnn_be_entropy_objective(E.data_ptr(), y.data_ptr(), B, n, out.data_ptr(), stream),
               "icnn_be_entropy_objective")
    return out


def objective(model, ctx: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """E(x, y) - H(y), float64 [B]: one model.fg (which rounds y to float32 like a feed) plus the entropy of y itself."""
    _entry(model)
    y = y.to(model.device, torch.float64)
    y = y.reshape(y.shape[0], -1).contiguous()
    E, _ = model.fg(ctx, y)
    return entropy_objective(E, y)


def _state(result):
    st = getattr(result, "state", None)
    if st is None or not hasattr(st, "c_state"):
        raise TypeError("a native BundleResult is needed (solveBatch(..., native=True) or FusedSolver.solve)")
    return st


def bundle_trace(result) -> Tuple[torch.Tensor, torch.Tensor]:
    """(obj float64 [T, B], calls int32 [1]) of a finished FUSED solve, variants 'dual' and 'pdipm': obj[t, u] is what a
    callback(t, f, x) recording f - entr(x) would have seen for sample u at outer iteration t -- a sample that left the loop
    keeps its iterate and its last energy --, calls the number of callback invocations; rows at or beyond it are NaN.  The
    device form of the callback replay of bundle_entropy.solveBatch: nothing is copied to the host."""
    st = _state(result)
    if st.variant == "rl":
        raise ValueError("bundle_trace serves variants 'dual' and 'pdipm': the 'rl' callback has no x")
    if st.n_iter > st.T:
        raise ValueError("bundle_trace needs nIter <= %d active slots per iteration (beyond it the slots are recycled and "
                         "hold no per-iteration history)" % _lib.MAX_SLOTS)
    dev = st.y.device
    obj = torch.empty(st.T, st.B, dtype=torch.float64, device=dev)
    calls = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(st.lib.icnn_be_bundle_trace(C.byref(st.c_state), obj.data_ptr(), calls.data_ptr(), st.stream()),
               "icnn_be_bundle_trace")
    return obj, calls


def dual_bound(result) -> torch.Tensor:
    """float64 [B]: lam . h - sum_j log(1 + exp(-a_j)) with a = G^T lam over each sample's active cuts -- a lower bound of
    min_y E - H for multipliers on the simplex, since every cut under-estimates the convex E.  -inf for a
    sample without a cut."""
    st = _state(result)
    out = torch.empty(st.B, dtype=torch.float64, device=st.y.device)
    _lib.check(st.lib.icnn_be_dual_bound(C.byref(st.c_state), out.data_ptr(), st.stream()), "icnn_be_dual_bound")
    return out


def gap(model, ctx: torch.Tensor, result) -> torch.Tensor:
    """objective(y*) - dual_bound, float64 [B]: how far the solve's y* can be above the minimum of E - H."""
    return objective(model, ctx, _state(result).y) - dual_bound(result)
