"""Training step of the PICNNs on the device.

    surrogate_grad  the parameter gradient of the reference's surrogate F = c E + <dE/dy, v> over every trainable
                    variable (multi-label-cls/icnn_ebundle.py:148-156; with v absent the RL critic's c-weighted energy,
                    RL/src/icnn.py:90-109): HIP kernels of be_train_fc.hip through icnn_be_fc_surrogate_grad.  For the
                    conv PICNN of the completion experiment (completion/icnn_ebundle.py:129-140) be_train_conv.hip
                    through icnn_be_conv_surrogate_grad, for the FICNN be_train_ficnn.hip through
                    icnn_be_ficnn_surrogate_grad.  The model classes state their entries, leading descriptors and input
                    shape themselves (picnn._DeviceWeights); grad_layout is each spec's own (picnn.FCSpec / ConvSpec,
                    ficnn.FICNNSpec).
    TFAdam          tf.train.AdamOptimizer's update rule on device tensors (torch plumbing, not a kernel).
    DeviceAdam      the same update, the reference's proj and the repack of every copy the kernels read, in one launch of
                    be_train_update.hip (icnn_be_param_update) over a flat theta; the model's packed weights live in one
                    device buffer (the arena) that the update writes in place.
    FollowerWeights the same theta and arena without optimiser state, for a model another launch writes (the RL agent's
                    target network, rl_train.CriticTrainer).

    _Trainer        what the trainers below and ficnn.GDTrainer share round their step(): batch buffers, context buffers, the
                    start point (_start_point), the test phase's checks, the views of the optimiser's theta.  It lives in
                    icnn_amd.flat with the argument checks and macro_f1; the names stay importable from here.

    BundleTrainer   one whole iteration of the bundle-entropy training loops without a host wait (capturable): context,
                    fused solve, FeedPlan (be_train_bundle.hip: row offsets, row count, fg evaluations, status OR, loss, F1
                    tallies), BatchNorm folds with a device count, PaddedFeed, surrogate_grad(rows_dev=), DeviceAdam.step
                    (DESIGN.md §15); the start point y0, the scripts' test phase as evaluate() and the device-side skip of
                    the update on a solver error (icnn_be_step_gate, icnn_be_param_update_gated, icnn_be_gated_copy;
                    DESIGN.md §18).

    unrolled_grad   the parameter gradient of a loss of y_K through the unrolled momentum-GD inference of gd.solve (the
                    back-optimisation scripts, multi-label-cls/icnn-back.py, completion/icnn.back.py): one surrogate_grad
                    over the trajectory's rows with c = 0 and v = coefficient x dL/dy_K.

    UnrolledGDTrainer  one whole back-optimisation training step without a host wait (capturable): context, gd.solve with its
                    trajectory, a fused feed of be_train_gd.hip (loss, dL/dy_K times the step coefficients, row offsets),
                    surrogate_grad, DeviceAdam.step; and the scripts' test phase as evaluate().  GDTrainer is that step on an
                    FC PICNN (icnn_be_gd_feed with its F1 tallies, icnn_be_gd_eval), ConvGDTrainer on the
                    completion model (completion/icnn.back.py:131-165, 210-254) with the loss mean((255 (y_K - t))^2) and
                    its feed on a two-dimensional grid (icnn_be_gd_feed_px).

    BestKeeper, DeviceDataset, StepLog, EpochRunner  the epoch level (icnn_amd.epoch), re-exported here.

One training step of the multi-label experiment:
    solve -> bundle_entropy.implicit_feed -> surrogate_grad(flat=True) -> DeviceAdam.step
or, for a caller that updates the weights itself,
    solve -> bundle_entropy.implicit_feed -> surrogate_grad -> TFAdam.step -> picnn.project -> model.repack
and of the completion experiment the same with ConvModel.context, a conv solve and implicit_feed(..., "mse").
"""
import ctypes as C
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib, gd
from .bundle_entropy import FusedSolver, ImplicitFeed
from .flat import _eval_batch, _non_negative, _positive, _start_point, _ticket, _Trainer, _TrainF1, macro_f1  # noqa: F401
from .picnn import ConvModel, FCModel


def grad_layout(spec) -> List[Tuple[str, tuple]]:
    """(name, shape) of every variable of the packed gradient, in the order include/icnn_be.h documents (the order of
    picnn.init_params' keys for an FCSpec, of picnn.init_conv_params' for a ConvSpec, of ficnn.init_params' for a FICNNSpec);
    each spec keeps its own."""
    return spec.grad_layout()


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
    return int(getattr(model._lib, model.grad_floats_entry)(*model._descriptors()))


def surrogate_grad(model, x: torch.Tensor, feed_or_rows, row_offset=None, F_rows=None, bn_updates=0, flat=False,
                   rows_dev=None, out=None, work=None):
    """Gradient of sum_r [ c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r> ] over every trainable variable of `model`,
    keyed like picnn.init_params(spec) -- for a ConvModel like picnn.init_conv_params(spec), x [B, H, W, 1] already
    h-flipped (completion/icnn_ebundle.py:215).

    feed_or_rows: an ImplicitFeed (bundle_entropy.implicit_feed: rows grouped by sample, in sample order), or (y, c) --
    the RL critic, one row per sample and no v -- or (y, v, c) with `row_offset` (int32 [B+1]: rows of sample j are
    row_offset[j] .. row_offset[j+1]-1).  BatchNorm runs over the feed rows, each sample counted once per row, as the
    reference's x_ = fd_xs.  F_rows: optional float32 [R] tensor that receives F_r.  bn_updates = k > 0 also folds those
    BatchNorm statistics k times into model.bn_stats (1: what the reference's train_step does); the gradient is the same.
    flat=True: the packed float32 [grad_floats] tensor itself (grad_layout order, what DeviceAdam.step takes) instead of the
    dict of views.  Enqueued on the current stream without any host synchronisation (capturable in a CUDA graph).

    rows_dev: an int32 device tensor (one element) holding the TRUE row count of a fixed-capacity feed -- y.shape[0] is then
    the capacity R_cap, row_offset[B] equals the count, and the rows behind it are padding (finite y, v = 0, c = 0:
    icnn_be_feed_pad) that contributes exactly nothing; BatchNorm normalises by the true count, so bn_stats and F_rows
    [0, count) are the compact call's bits, and a count of 0 gives a zero gradient and leaves bn_stats alone.  out / work:
    caller-owned float32 buffers (grad_floats(model); surrogate_work_floats(model, B, R)) for a step that allocates nothing."""
    spec, dev = model.spec, model.device
    x = x.to(dev, torch.float32).contiguous()
    B = x.shape[0]
    model.check_x(x)
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
    entry = model.grad_entry
    if not model.grad_takes_stats:                      # the FICNN's one entry: no moving statistics, no rows_dev form
        if bn_updates:
            raise ValueError("a FICNN has no BatchNorm statistics to fold (bn_updates=%d)" % bn_updates)
        if rows_dev is not None or out is not None or work is not None:
            raise ValueError("rows_dev / out / work are for the PICNN entries: icnn_be_ficnn_surrogate_grad has no such form")
    if rows_dev is not None and (not torch.is_tensor(rows_dev) or rows_dev.dtype != torch.int32 or rows_dev.numel() != 1
                                 or not rows_dev.is_cuda):
        raise ValueError("rows_dev is one int32 on the device")
    grad = torch.empty(grad_floats(model), dtype=torch.float32, device=dev) if out is None else out
    assert grad.shape == (grad_floats(model),) and grad.dtype == torch.float32 and grad.is_contiguous()
    if R == 0:
        return grad.zero_() if flat else unpack_grad(spec, grad.zero_())
    n_work = surrogate_work_floats(model, B, R, dev=rows_dev is not None)
    if work is None:
        work = torch.empty(n_work, dtype=torch.float32, device=dev)
    assert work.dtype == torch.float32 and work.numel() >= n_work
    if F_rows is not None:
        assert F_rows.dtype == torch.float32 and F_rows.shape == (R,) and F_rows.is_contiguous()
    args = [*model._descriptors(), x.data_ptr(), B, row_offset.data_ptr(), R, y.data_ptr(),
            None if v is None else v.data_ptr(), c.data_ptr(), grad.data_ptr(),
            None if F_rows is None else F_rows.data_ptr(), work.data_ptr()]
    stream = model._stream()
    if not model.grad_takes_stats:
        _lib.check(getattr(model._lib, entry)(*args, stream), entry)
        return grad if flat else unpack_grad(spec, grad)
    mv = model._c_bn()
    if rows_dev is None:
        _lib.check(getattr(model._lib, entry + "_bn")(*args, C.byref(mv), bn_updates, stream), entry)
    else:
        _lib.check(getattr(model._lib, entry + "_dev")(*args, C.byref(mv), bn_updates, rows_dev.data_ptr(), stream),
                   entry + "_dev")
    return grad if flat else unpack_grad(spec, grad)


def surrogate_work_floats(model, batch, rows, dev=False) -> int:
    """floats of surrogate_grad's workspace for `model` at (batch, rows); dev: of the rows_dev form (PICNNs only: a FICNN
    has no such entry), which is larger (its forward products keep split-K partials for any plan).  Raises on a shape the
    library rejects"""
    entry = model.grad_entry + ("_dev" if dev else "")
    n_work = int(getattr(model._lib, entry + "_work_floats")(*model._descriptors(), batch, rows))
    if n_work == 0:
        raise ValueError("%s: shape rejected (batch %d, rows %d)" % (entry, batch, rows))
    return n_work


_COEF_CACHE: Dict[tuple, torch.Tensor] = {}


def unrolled_coefficients(n_iter, lr, momentum, device) -> torch.Tensor:
    """gd.coefficients(n_iter, lr, momentum) as a float64 [1, K, 1] device tensor, uploaded once per (K, lr, momentum,
    device) -- call it before capturing a graph that runs unrolled_grad"""
    K = int(n_iter)
    key = (K, float(lr), float(momentum), str(device))
    coef = _COEF_CACHE.get(key)
    if coef is None:
        coef = torch.from_numpy(gd.coefficients(K, lr, momentum)).to(device).view(1, K, 1)
        _COEF_CACHE[key] = coef
    return coef


def unrolled_grad(model, x: torch.Tensor, traj: torch.Tensor, ybar: torch.Tensor, lr: float, momentum: float, bn_updates=0,
                  flat=False):
    """Gradient of L(y_K) over every trainable variable of `model` when y_K = gd.solve(model, context(x), y0, K, lr, momentum)
    -- the back-optimisation training step.  traj: float64 [B, K, n] (gd.solve(..., trajectory=True)), ybar = dL/dy_K
    [B, n] (ConvModel: x, traj and ybar may carry the image shape).  E is piecewise linear in y, so the adjoint of y is the
    same at every step and the gradient is sum_k grad_theta <dE/dy(x, y_k), coefficients[k] ybar>: one surrogate_grad over
    the B K rows (sample-major, row_offset[j] = K j) with c = 0.  Each sample has the same multiplicity K, so BatchNorm over
    those rows has the statistics of the reference's per-call batch, and the x-only backward runs once.

    bn_updates is passed through.  Read as written, the reference's train_step executes K calls of f on its path to the
    loss (E(y_0) .. E(y_{K-1}), each with its own BatchNorm of the batch) and would fold the statistics once per call, K
    times; TensorFlow's graph optimiser may merge those identical x-only subgraphs, so that count is not pinned down.  flat: as surrogate_grad.  No host synchronisation once the step coefficients of (K, lr, momentum)
    are on the device (the first call per triple uploads them: make it before capturing a CUDA graph)."""
    dev = model.device
    spec = model.spec
    n = spec.n_labels
    B = traj.shape[0]
    traj = traj.to(dev, torch.float64).reshape(B, -1, n)
    K = traj.shape[1]
    ybar = ybar.to(dev, torch.float64).reshape(B, 1, n)
    coef = unrolled_coefficients(K, lr, momentum, dev)
    y = traj.reshape(B * K, n)
    v = (coef * ybar).reshape(B * K, n)
    c = torch.zeros(B * K, dtype=torch.float64, device=dev)
    row_offset = torch.arange(0, (B + 1) * K, K, dtype=torch.int32, device=dev)
    return surrogate_grad(model, x, (y, v, c), row_offset=row_offset, bn_updates=bn_updates, flat=flat)


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


# --------------------------------------------------------------------------------------------- #
# Device-side update: the weight arena, the map from theta into it, and DeviceAdam
# --------------------------------------------------------------------------------------------- #
ARENA_ALIGN = 64            # floats: every sub-buffer of the arena starts on a 256-byte boundary
INDEX_LIMIT = 1 << 24       # float(j + 1) is exact for j + 1 <= 2^24


def index_params(layout) -> Dict[str, np.ndarray]:
    """The index image of a parameter layout ((name, shape) list, grad_layout order): entry j of the flat theta holds
    float(j + 1), so that what the host packers make of it says which theta index landed where (0: padding)."""
    total = sum(int(np.prod(shape)) for _, shape in layout)
    if total > INDEX_LIMIT:
        raise ValueError("%d parameters: the index image float(j + 1) is exact only up to 2^24 = %d" % (total, INDEX_LIMIT))
    idx = np.arange(1, total + 1, dtype=np.int64).astype(np.float32)
    out, at = {}, 0
    for name, shape in layout:
        size = int(np.prod(shape))
        out[name] = idx[at:at + size].reshape(shape)
        at += size
    return out


def arena_offsets(parts) -> Tuple[List[int], int]:
    """Float offset of every part of model.arena_parts in the arena (each 256-byte aligned) and the arena's size."""
    offs, at = [], 0
    for _, _, a in parts:
        offs.append(at)
        at += -(-a.size // ARENA_ALIGN) * ARENA_ALIGN
    return offs, at


def arena_image(model, params) -> Tuple[np.ndarray, list, List[int]]:
    """Host image of the arena for `params`: the host packers' output (icnn_be_*_pack, the stage concatenations, gamma /
    beta) at arena_offsets, zeros elsewhere.  Returns (image, parts, offsets)."""
    parts = model.arena_parts(params)
    offs, total = arena_offsets(parts)
    img = np.zeros(total, np.float32)
    for (_, _, a), off in zip(parts, offs):
        img[off:off + a.size] = np.asarray(a, np.float32).reshape(-1)
    return img, parts, offs


class ParamMap:
    """Where every entry of the flat theta sits in the arena, built once per model shape through the host packers fed
    the index image: dest[dest_off[j]:dest_off[j + 1]] are the arena float offsets holding a copy of theta[j] (CSR,
    int32).  proj: the [begin, end) ranges of theta that picnn.project clamps."""

    def __init__(self, model):
        layout = grad_layout(model.spec)
        self.n = sum(int(np.prod(shape)) for _, shape in layout)
        img, parts, self.offsets = arena_image(model, index_params(layout))
        self.arena_floats = img.size
        if self.arena_floats >= 1 << 31:
            raise ValueError("arena of %d floats: int32 offsets do not reach" % self.arena_floats)
        src = img.astype(np.int64)
        if not (np.array_equal(src.astype(np.float32), img) and src.min() >= 0 and src.max() <= self.n):
            raise AssertionError("the host packers changed an index value: the arena is not a copy of theta")
        src -= 1                                       # -1: padding
        pos = np.nonzero(src >= 0)[0]
        order = np.argsort(src[pos], kind="stable")
        self.dest = pos[order].astype(np.int32)
        counts = np.bincount(src[pos], minlength=self.n)
        self.dest_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.max_fanout = int(counts.max())
        self.proj, at = [], 0
        for name, shape in layout:
            size = int(np.prod(shape))
            if "proj" in name and name.endswith("/W"):
                self.proj.append((at, at + size))
            at += size

    def scatter(self, theta) -> np.ndarray:
        """The arena of a flat float32 theta as the kernel writes it (NumPy; padding zero)."""
        out = np.zeros(self.arena_floats, np.float32)
        src = np.repeat(np.arange(self.n), np.diff(self.dest_off))
        out[self.dest] = np.asarray(theta, np.float32)[src]
        return out


def adam_lr_t(lr, beta1, beta2, t) -> float:
    """TFAdam's bias-corrected step size, float64 from the step count (DeviceAdam rounds it once to float32)"""
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def _host(params) -> Dict[str, np.ndarray]:
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, np.float32)) for k, v in params.items()}


class _ArenaOwner:
    """What a device-resident weight set is made of: the flat float32 theta in grad_layout order, the ParamMap of the model,
    and the arena that the model's descriptors point into once attached."""

    def _attach(self, model, max_proj=None):
        if model._optimizer is not None:
            raise RuntimeError("the model is already attached to a DeviceAdam")
        self.model, self.spec, self.device = model, model.spec, model.device
        self.layout = grad_layout(self.spec)
        self.map = ParamMap(model)
        self.n = self.map.n
        if self.n != grad_floats(model):
            raise AssertionError("grad_layout has %d floats, the library's gradient %d" % (self.n, grad_floats(model)))
        if max_proj is not None and len(self.map.proj) > max_proj:
            raise ValueError("%d proj weights, the kernel takes %d ranges" % (len(self.map.proj), max_proj))
        dev = self.device
        self.theta = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.dest_off = torch.from_numpy(self.map.dest_off).to(dev)
        self.dest = torch.from_numpy(self.map.dest).to(dev)
        buf = torch.zeros(self.map.arena_floats + ARENA_ALIGN, dtype=torch.float32, device=dev)
        lead = (-buf.data_ptr() % 256) // 4           # device allocations are aligned already; host ones to 64 bytes
        self.arena = buf[lead:lead + self.map.arena_floats]
        assert self.arena.data_ptr() % 256 == 0
        params = _host(model.params)
        self.load(params)
        model._use_arena(self, self.arena, model.arena_parts(params), self.map.offsets)

    def params(self) -> Dict[str, torch.Tensor]:
        """device views of theta under the reference's names and shapes"""
        return unpack_grad(self.spec, self.theta)

    def host_params(self) -> Dict[str, np.ndarray]:
        """theta as a NumPy dict (one copy; synchronises): checkpoints, or a fresh FCModel / ConvModel"""
        flat = self.theta.cpu().numpy()
        return {name: t.numpy().copy() for name, t in unpack_grad(self.spec, torch.from_numpy(flat)).items()}

    def load(self, params):
        """Replace theta by `params` (host arrays or device tensors keyed like grad_layout) and rewrite the arena from
        them through the host packers."""
        host = _host(params)
        missing = [name for name, _ in self.layout if name not in host]
        if missing:
            raise KeyError("parameters missing: %s" % missing)
        flat = np.concatenate([np.asarray(host[name], np.float32).reshape(-1) for name, _ in self.layout])
        if flat.size != self.n:
            raise ValueError("parameters hold %d floats, the model %d" % (flat.size, self.n))
        self.theta.copy_(torch.from_numpy(flat))
        self.arena.copy_(torch.from_numpy(arena_image(self.model, host)[0]))


class FollowerWeights(_ArenaOwner):
    """The weights of a model that another launch writes -- the RL agent's target network, which the critic's update
    moves by a soft (Polyak) step (rl_train.CriticTrainer, icnn_be_rl_critic_update): theta and an arena of its own as
    DeviceAdam keeps them, no optimiser state.  Constructing one ATTACHES the model the same way: its descriptors point
    into the arena for good and its `params` are live device views of theta."""

    def __init__(self, model):
        self._attach(model)


class DeviceAdam(_ArenaOwner):
    """tf.train.AdamOptimizer (TFAdam's rule) + the reference's proj + the repack of the model, on the device, one launch
    per step (icnn_be_param_update).  theta, m, v are flat float32 device tensors in grad_layout order; the step count
    lives on the device and every launch advances it, so a captured step replayed k times is k steps.

    Constructing one ATTACHES the model: its packed weights move into one persistent device buffer (the arena) that
    c_model.wpack and every c_ctx pointer reference from then on, so solves, contexts and gradients captured in a graph keep
    reading the current weights.  An attached model's `params` are live device views of theta; its repack, repack_context
    and clamp raise (use load; m, v and the step count are kept)."""

    def __init__(self, model, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        self.lr, self.beta1, self.beta2, self.eps = float(lr), float(beta1), float(beta2), float(eps)
        self._attach(model, max_proj=_lib.MAX_PROJ_RANGES)
        self.m = torch.zeros_like(self.theta)
        self.v = torch.zeros_like(self.theta)
        self.step_count = torch.zeros(2, dtype=torch.int32, device=self.device)     # updates done, ticket
        a = _lib.ParamUpdateArgs()
        a.n, a.theta, a.m, a.v = self.n, self.theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        a.dest_off, a.dest, a.arena = self.dest_off.data_ptr(), self.dest.data_ptr(), self.arena.data_ptr()
        a.arena_floats, a.step = self.arena.numel(), self.step_count.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.beta1, self.beta2, self.eps
        a.n_proj = len(self.map.proj)
        for i, (b, e) in enumerate(self.map.proj):
            a.proj_begin[i], a.proj_end[i] = b, e
        self._args = a

    @property
    def t(self) -> int:
        """updates done (reads the device counter: synchronises)"""
        return int(self.step_count[0].item())

    def step(self, grad, go=None):
        """One update with `grad`: the flat float32 [n] tensor surrogate_grad(..., flat=True) returns, or its dict form.
        Enqueued on the current stream, no host synchronisation (capturable).  go: an int32 device tensor (one element,
        icnn_be_step_gate's gate[0]); the update happens only where it is non-zero when the launch runs, and a launch that
        finds 0 changes nothing, the step count included (icnn_be_param_update_gated)."""
        if go is not None and (not torch.is_tensor(go) or go.dtype != torch.int32 or go.numel() != 1 or not go.is_cuda):
            raise ValueError("go is one int32 on the device")
        if isinstance(grad, dict):
            grad = torch.cat([grad[name].reshape(-1) for name, _ in self.layout])
        grad = grad.to(self.device, torch.float32)
        if grad.shape != (self.n,):
            raise ValueError("gradient of shape %s, the model has %d parameters" % (tuple(grad.shape), self.n))
        if not grad.is_contiguous() or grad.data_ptr() % 16:
            grad = grad.clone()
        self._args.grad = grad.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if go is not None:
            _lib.check(self.model._lib.icnn_be_param_update_gated(C.byref(self._args), go.data_ptr(), C.c_void_p(stream)),
                       "icnn_be_param_update_gated")
            return
        _lib.check(self.model._lib.icnn_be_param_update(C.byref(self._args), C.c_void_p(stream)), "icnn_be_param_update")


# --------------------------------------------------------------------------------------------- #
# The bundle-entropy training step as one device step
# --------------------------------------------------------------------------------------------- #
class FeedPlan:
    """The device-side plan of a training feed (icnn_be_feed_plan, be_train_bundle.hip) at one batch size and loss: from a
    finished solve and the targets, row_offset [B+1], counts = (rows, fg evaluations, OR of the status words), the loss
    (float64) and, for "xent", the per-example F1 tallies [B, 3] -- all device tensors, allocated here once."""

    def __init__(self, state, loss):
        if loss not in _lib.LOSS:
            raise ValueError("loss must be 'xent' or 'mse', got %r" % (loss,))
        self.state, self.loss_name = state, loss
        B, dev = state.B, state.y.device
        self.row_offset = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(3, dtype=torch.int32, device=dev)
        self.rows, self.fg_evals, self.status_or = self.counts[0:1], self.counts[1:2], self.counts[2:3]
        self.loss = torch.zeros((), dtype=torch.float64, device=dev)
        self.f1_tallies = torch.zeros(B, 3, dtype=torch.int32, device=dev) if loss == "xent" else None
        self._work = _ticket(state.lib.icnn_be_feed_plan_work_bytes(B), dev)

    def run(self, true_y):
        """enqueue the plan for the state's current contents and true_y (float64 [B, n] device tensor); no host wait"""
        st = self.state
        assert true_y.dtype == torch.float64 and true_y.is_contiguous() and true_y.shape == (st.B, st.n) and true_y.is_cuda
        _lib.check(st.lib.icnn_be_feed_plan(C.byref(st.c_state), true_y.data_ptr(), _lib.LOSS[self.loss_name],
                                            self.row_offset.data_ptr(), self.counts.data_ptr(), self.loss.data_ptr(),
                                            None if self.f1_tallies is None else self.f1_tallies.data_ptr(),
                                            self._work.data_ptr(), st.stream()), "icnn_be_feed_plan")
        return self


class PaddedFeed:
    """A training feed of fixed capacity R_cap = B x (the state's slot count): a sample keeps at most that many cuts active,
    so every feed of the state fits.  fill() writes rows [0, R) exactly as bundle_entropy.implicit_feed does and the padding
    [R, R_cap): y = 0.5, v = 0, c = 0.  `scale` (tests) multiplies the capacity."""

    def __init__(self, state, scale=1):
        B, n, dev = state.B, state.n, state.y.device
        self.state, self.row_cap = state, int(scale) * B * state.T
        R = self.row_cap
        self.y = torch.full((R, n), 0.5, dtype=torch.float64, device=dev)
        self.v = torch.zeros(R, n, dtype=torch.float64, device=dev)
        self.c = torch.zeros(R, dtype=torch.float64, device=dev)
        self.sample = torch.zeros(R, dtype=torch.int32, device=dev)

    def fill(self, plan: FeedPlan, true_y):
        st = self.state
        if st.B == 0:
            return self
        _lib.check(st.lib.icnn_be_implicit_feed(C.byref(st.c_state), true_y.data_ptr(), _lib.LOSS[plan.loss_name],
                                                plan.row_offset.data_ptr(), self.y.data_ptr(), self.v.data_ptr(),
                                                self.c.data_ptr(), self.sample.data_ptr(), st.stream()), "icnn_be_implicit_feed")
        _lib.check(st.lib.icnn_be_feed_pad(plan.rows.data_ptr(), st.B, st.n, self.row_cap, self.y.data_ptr(), self.v.data_ptr(),
                                           self.c.data_ptr(), self.sample.data_ptr(), st.stream()), "icnn_be_feed_pad")
        return self


class BundleTrainer(_Trainer, _TrainF1):
    """One iteration of the bundle-entropy training loops (multi-label-cls/icnn_ebundle.py:208-250 with loss "xent" on a
    picnn.FCModel; completion/icnn_ebundle.py with loss "mse" on a picnn.ConvModel) at one batch size, all of it enqueued
    on the current stream without a host wait, so a step can be captured in a CUDA graph:

        context (batch statistics) -> FusedSolver.solve from y0 -> FeedPlan -> BatchNorm folds for the solve's fg
        evaluations (models with BatchNorm) -> PaddedFeed -> surrogate_grad(bn_updates=1, rows_dev=) -> DeviceAdam.step

    Constructing one ATTACHES the model to its DeviceAdam and allocates every buffer; step allocates nothing.  After a step
    the device tensors loss (float64, what the reference prints as l_yN / the squared error), f1_tallies ("xent": int32 [B,
    3], see macro_f1), rows, fg_evals, status_or (int32 [1] each) and grad (the flat gradient) hold its results; read them
    after a synchronisation of your choosing.

    y0: the start point of every solve -- a scalar (0.5, the multi-label script), an [n] row (the completion script's
    meanY, completion/icnn_ebundle.py:223-227), an image [H, W, 1] or a [B, n] array (images [B, H, W, 1] too); set_y0
    replaces it, outside a capture.

    skip_on_error=False: the update is NOT skipped on a solver error as the reference's completion loop does on LinAlgError;
    call raise_on_error() and reload the weights if you need that.  skip_on_error=True: the skip happens on the device
    (DESIGN.md §18).  Behind the plan icnn_be_step_gate turns status_or into the words went (int32 [1]: 1 when no sample has
    ST_SINGULAR, ST_NONFINITE, ST_UNFINISHED or ST_OVERFLOW set) and skipped (int32 [1]: the running count of steps that did
    not go, the reference's nErrors; giving up after some number of them stays the caller's policy, read it when you read the
    loss).  The feed, the gradient and the loss of such a step are still computed and may be garbage; its update is
    icnn_be_param_update_gated and its BatchNorm folds are undone from a shadow (icnn_be_gated_copy), so theta, m, v, the
    arena, the step count and model.bn_stats are bit for bit what they were before the step.  The model's moving statistics
    move into one buffer for that (model.flatten_bn_stats()).

    eval_batch = E also allocates the scripts' test phase (multi-label-cls/icnn_ebundle.py:257-277,
    completion/icnn_ebundle.py:264-300): evaluate(x, true_y) runs the context in eval_bn mode without a fold, a solve of its
    own from y0 and a plan of its own on exactly E samples; it returns the float64 device scalar eval_loss, keeps y_eval and,
    for "xent", eval_f1_tallies (eval_macro_f1() reads them), and changes no weight, optimiser state, statistic or result of
    the training step.  eval_bn=None is what each script does at test time: "batch" for an FCModel (the multi-label script
    keeps is_training(True), :259), "moving" for a ConvModel (the completion script sets is_training(False), :266).  A [B, n]
    y0 serves the test phase only when E = B."""
    # what each script trains and tests with: (the model it serves, its loss, the BatchNorm mode of its test phase)
    _SCRIPTS = ((FCModel, "xent", "batch"), (ConvModel, "mse", "moving"))
    _no_tallies = "F1 tallies exist for loss 'xent' only"
    _no_eval_tallies = "F1 tallies exist for loss 'xent' and a trainer constructed with eval_batch only"

    def __init__(self, model, batch, n_iter=10, loss="xent", variant="pdipm", lr=1e-3, y0=0.5, eval_batch=None, eval_bn=None,
                 skip_on_error=False):
        if loss not in _lib.LOSS:
            raise ValueError("loss must be 'xent' or 'mse', got %r" % (loss,))
        script = [s for s in self._SCRIPTS if isinstance(model, s[0])]
        if not script:
            raise TypeError("BundleTrainer serves picnn.FCModel and picnn.ConvModel, got %s" % type(model).__name__)
        _, want, script_bn = script[0]
        if loss != want:
            raise ValueError("a %s trains with loss %r, got %r" % (type(model).__name__, want, loss))
        if variant not in ("dual", "pdipm"):
            raise ValueError("variant must be 'dual' or 'pdipm' (the rl variant does not record n_iters), got %r" % (variant,))
        self.batch = _positive("batch", batch)
        self.eval_batch = _eval_batch(eval_batch)
        if eval_bn is None:
            eval_bn = script_bn
        if eval_bn not in _lib.BN_MODE:
            raise ValueError("eval_bn must be 'batch' or 'moving', got %r" % (eval_bn,))
        self.eval_bn, self.skip_on_error = eval_bn, bool(skip_on_error)
        self.model, self.spec, self.device = model, model.spec, model.device
        self.n_iter, self.loss_name, self.variant, self.lr = int(n_iter), loss, variant, float(lr)
        self.has_bn = model.has_bn
        self.opt = DeviceAdam(model, lr=lr)
        B, E, dev, n = self.batch, self.eval_batch, self.device, self.spec.n_labels
        model.reserve(max(B, E or 0))                   # grown here, never inside a capture
        self.solver = FusedSolver(model, B, self.n_iter, variant)
        st = self.solver.state
        self.plan = FeedPlan(st, loss)
        self.feed = PaddedFeed(st)
        self.x = torch.zeros((B,) + model.x_shape, dtype=torch.float32, device=dev)
        self.true_y = torch.zeros(B, n, dtype=torch.float64, device=dev)
        self.ctx, self._ctx_work = self._context_buffers(B)
        self._ctx_fold = torch.empty_like(self.ctx) if self.has_bn else None
        self.grad = torch.zeros(self.opt.n, dtype=torch.float32, device=dev)
        self._grad_work = torch.empty(surrogate_work_floats(model, B, self.feed.row_cap, dev=True), dtype=torch.float32, device=dev)
        self.loss, self.f1_tallies = self.plan.loss, self.plan.f1_tallies
        self.rows, self.fg_evals, self.status_or = self.plan.rows, self.plan.fg_evals, self.plan.status_or
        self.row_offset = self.plan.row_offset
        self.went = self.skipped = self._gate = self._bn_live = self._bn_shadow = None
        if self.skip_on_error:
            self._gate = torch.zeros(3, dtype=torch.int32, device=dev)              # go, folds, skipped
            self.went, self.skipped = self._gate[0:1], self._gate[2:3]
            if self.has_bn:
                self._bn_live = model.flatten_bn_stats()
                self._bn_shadow = torch.empty_like(self._bn_live)
        self.y_eval = self.eval_loss = self.eval_f1_tallies = None
        if E is not None:
            self.eval_solver = FusedSolver(model, E, self.n_iter, variant)
            self.eval_plan = FeedPlan(self.eval_solver.state, loss)
            self.x_eval = torch.zeros((E,) + model.x_shape, dtype=torch.float32, device=dev)
            self.true_y_eval = torch.zeros(E, n, dtype=torch.float64, device=dev)
            self.ctx_eval, self._ctx_work_eval = self._context_buffers(E)
            self.y_eval, self.eval_loss = self.eval_solver.y, self.eval_plan.loss
            self.eval_f1_tallies = self.eval_plan.f1_tallies
        self.y0 = self.y0_eval = None                   # float64 [B, n] / [E, n] once a start point is not a scalar
        self._y0_scalar = 0.5
        self.set_y0(y0)

    def set_y0(self, y0):
        """The start point of step() and evaluate(): a scalar, an [n] row, an image [H, W, 1] or a [B, n] array ([B, H, W, 1]
        too).  A copy from the host: call it outside a capture (a captured step keeps the KIND of start point it was captured
        with: a scalar fills, anything else is copied from the tensors this call writes)."""
        n = self.spec.n_labels
        y0 = _start_point(y0, n, self.batch, self.eval_batch, self.device)
        if isinstance(y0, float):                       # the solver's fill_, as before there was a y0
            self._y0_scalar = y0
            return
        if self.eval_batch is not None:
            if self.y0_eval is None:
                self.y0_eval = torch.empty(self.eval_batch, n, dtype=torch.float64, device=self.device)
            self.y0_eval.copy_(y0.expand(self.eval_batch, n))
        if self.y0 is None:
            self.y0 = torch.empty(self.batch, n, dtype=torch.float64, device=self.device)
        self.y0.copy_(y0.expand(self.batch, n))
        self._y0_scalar = None

    def _infer(self, x=None, true_y=None):
        """the first half of step(): the copies, the context, the solve from y0 and the plan"""
        self._put(self.x, x)
        self._put(self.true_y, true_y)
        self.model.context(self.x, out=self.ctx, work=self._ctx_work)
        self.solver.solve(self.ctx, self.y0 if self._y0_scalar is None else self._y0_scalar)
        self.plan.run(self.true_y)

    def _learn(self):
        """the second half of step(): the gate (skip_on_error), the BatchNorm folds, the feed, the gradient and the update,
        all from what the plan left on the device"""
        model, lib, gated = self.model, self.model._lib, self.skip_on_error
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if gated:
            _lib.check(lib.icnn_be_step_gate(self.plan.counts.data_ptr(), _lib.ST_ERROR_MASK, self._gate.data_ptr(), stream),
                       "icnn_be_step_gate")
            if self.has_bn:
                self._bn_shadow.copy_(self._bn_live)
        if self.has_bn:
            model.context(self.x, bn_updates=self.fg_evals, out=self._ctx_fold, work=self._ctx_work)
        self.feed.fill(self.plan, self.true_y)
        surrogate_grad(model, self.x, (self.feed.y, self.feed.v, self.feed.c), row_offset=self.row_offset, bn_updates=1,
                       flat=True, rows_dev=self.rows, out=self.grad, work=self._grad_work)
        self.opt.step(self.grad, go=self.went)
        if gated and self.has_bn:                       # a step that did not go folds nothing
            _lib.check(lib.icnn_be_gated_copy(self._bn_live.data_ptr(), self._bn_shadow.data_ptr(), self._bn_live.numel(),
                                              self.went.data_ptr(), 0, stream), "icnn_be_gated_copy")

    def step(self, x=None, true_y=None) -> torch.Tensor:
        """One iteration on (x, true_y [B, n]); None keeps the batch of the previous call (graph replay).  Returns the loss at
        y* (before the update), a float64 device scalar."""
        self._infer(x, true_y)
        self._learn()
        return self.loss

    def evaluate(self, x=None, true_y=None) -> torch.Tensor:
        """The test phase on exactly eval_batch samples (x, true_y shaped as for step; None keeps the previous ones): the loss
        at y* of a solve from y0 with the context in eval_bn mode, a float64 device scalar (eval_loss); y_eval keeps y* and
        eval_f1_tallies ("xent") the tallies.  Nothing is updated and no statistic is folded.  No host wait (capturable)."""
        self._require_eval()
        self._put(self.x_eval, x)
        self._put(self.true_y_eval, true_y)
        self.model.context(self.x_eval, bn=self.eval_bn, out=self.ctx_eval, work=self._ctx_work_eval)
        self.eval_solver.solve(self.ctx_eval, self.y0_eval if self._y0_scalar is None else self._y0_scalar)
        self.eval_plan.run(self.true_y_eval)
        return self.eval_loss

    def raise_on_error(self):
        """BundleResult.raise_on_error from status_or (reads it: one wait).  The OR names no sample."""
        bits = int(self.status_or.item())
        if bits & _lib.ST_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix (a sample of the last step)")
        if bits & _lib.ST_NONFINITE:
            raise FloatingPointError("non-finite value in the bundle of a sample of the last step")
        if bits & _lib.ST_UNFINISHED:
            raise RuntimeError("a sample is still behind after the finishing rounds of a time-sliced solve "
                               "(ICNN_BE_ST_UNFINISHED)")
        if bits & _lib.ST_OVERFLOW:
            raise MemoryError("the active bundle of a sample outgrew the cuts one workgroup can stage")


# --------------------------------------------------------------------------------------------- #
# The back-optimisation training step and test phase as one device step each
# --------------------------------------------------------------------------------------------- #
class UnrolledGDTrainer(_Trainer):
    """What GDTrainer and ConvGDTrainer share: the buffers of a back-optimisation step at one batch size, and

        step()      context (batch statistics) -> gd.solve(trajectory=True) from the start point -> self._feed(traj): the
                    loss, the rows v = coefficient x dL/dy_K, c = 0, row_offset -> surrogate_grad over the B K trajectory
                    rows -> DeviceAdam.step
        evaluate()  context in self.eval_bn mode -> gd.solve without a trajectory -> self._eval_feed(): eval_loss

    all enqueued on the current stream without a host wait.  Constructing one ATTACHES the model to its DeviceAdam and
    allocates every buffer (x is model.x_shape per sample, t [B, n] float32).  A subclass supplies the two feed entries, the
    bytes of their workspaces (_feed_work_bytes), the start point of either phase (_start) and eval_bn."""

    def __init__(self, model, batch, n_iter, lr, momentum, adam_lr, bn_updates, eval_batch):
        self.batch, self.n_iter = int(batch), int(n_iter)
        if self.batch < 1 or self.n_iter < 1:
            raise ValueError("batch and n_iter must be >= 1")
        self.bn_updates = _non_negative("bn_updates", bn_updates)
        self.eval_batch = _eval_batch(eval_batch)
        self.model, self.spec, self.device = model, model.spec, model.device
        self.lr, self.momentum = float(lr), float(momentum)
        self.opt = DeviceAdam(model, lr=adam_lr)
        B, K, E, n, dev = self.batch, self.n_iter, self.eval_batch, self.spec.n_labels, self.device
        model.reserve(max(B, E or 0))                   # grown here, never inside a capture
        self._coef = unrolled_coefficients(K, self.lr, self.momentum, dev)         # uploaded now, not inside a capture
        self.scale = float(np.float32(1.0) / np.float32(B * n))
        self.x = torch.zeros((B,) + model.x_shape, dtype=torch.float32, device=dev)
        self.t = torch.zeros(B, n, dtype=torch.float32, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.y = None                                   # gd.solve's own y_K tensor, from the first step on
        self.ctx, self._ctx_work = self._context_buffers(B)
        self.v_rows = torch.zeros(B * K, n, dtype=torch.float64, device=dev)
        self.c_rows = torch.zeros(B * K, dtype=torch.float64, device=dev)
        self.row_offset = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        self._feed_work = _ticket(self._feed_work_bytes(B, False), dev)
        self.grad = torch.zeros(self.opt.n, dtype=torch.float32, device=dev)
        self._grad_work = torch.empty(surrogate_work_floats(model, B, B * K), dtype=torch.float32, device=dev)
        self.y_eval = self.eval_loss = None
        if E is not None:
            self.x_eval = torch.zeros((E,) + model.x_shape, dtype=torch.float32, device=dev)
            self.t_eval = torch.zeros(E, n, dtype=torch.float32, device=dev)
            self.eval_loss = torch.zeros((), dtype=torch.float32, device=dev)
            self.ctx_eval, self._ctx_work_eval = self._context_buffers(E)
            self._feed_work_eval = _ticket(self._feed_work_bytes(E, True), dev)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def step(self, x=None, t=None) -> torch.Tensor:
        """One step on (x [B, *model.x_shape] -- a ConvModel's already h-flipped --, t [B, n] or images); None keeps the batch
        of the previous call (graph replay).  Returns the loss before the update, a float32 device scalar."""
        self._put(self.x, x)
        self._put(self.t, t)
        model, B, K, n = self.model, self.batch, self.n_iter, self.spec.n_labels
        model.context(self.x, out=self.ctx, work=self._ctx_work)
        self.y, traj, _ = gd.solve(model, self.ctx, self._start(False), K, self.lr, self.momentum, trajectory=True)
        self._feed(traj)
        surrogate_grad(model, self.x, (traj.view(B * K, n), self.v_rows, self.c_rows), row_offset=self.row_offset,
                       bn_updates=self.bn_updates, flat=True, out=self.grad, work=self._grad_work)
        self.opt.step(self.grad)
        return self.loss

    def evaluate(self, x=None, t=None) -> torch.Tensor:
        """The test phase on exactly eval_batch samples (x, t shaped as for step; None keeps the previous ones): the loss at
        y_K of the unrolled GD from the start point with the context in eval_bn mode, a float32 device scalar (eval_loss);
        y_eval keeps y_K.  Nothing is updated and no statistic is folded.  No host wait (capturable)."""
        self._require_eval()
        self._put(self.x_eval, x)
        self._put(self.t_eval, t)
        self.model.context(self.x_eval, bn=self.eval_bn, out=self.ctx_eval, work=self._ctx_work_eval)
        self.y_eval = gd.solve(self.model, self.ctx_eval, self._start(True), self.n_iter, self.lr, self.momentum)[0]
        self._eval_feed()
        return self.eval_loss


class GDTrainer(UnrolledGDTrainer, _TrainF1):
    """One training step of the back-optimisation scripts on a picnn.FCModel (synthetic-cls/icnn.py:117-139 with
    picnn.synthetic_spec(); multi-label-cls/icnn-back.py with the loss mean((y_K - t)^2)) at one batch size, all of it enqueued
    on the current stream without a host wait, so a step can be captured in a CUDA graph:

        context (batch statistics) -> gd.solve(trajectory=True) from y0 -> icnn_be_gd_feed (be_train_gd.hip: the loss, the
        rows v = coefficient x dL/dy_K, c = 0, row_offset, F1 tallies) -> surrogate_grad over the B K trajectory rows ->
        DeviceAdam.step (TF-Adam and the reference's proj)

    which is train.unrolled_grad with its torch elementwise launches folded into one kernel: the rows are the same bits, so
    grad and the update are those of the hand-composed step.  Constructing one ATTACHES the model to its DeviceAdam and
    allocates x, t, loss, the feed rows, the gradient and the gradient's workspace.  step() returns the loss (before the
    update, as the reference's sess.run returns it) as a float32 device scalar.  After a step the device tensors loss, grad
    (flat), y (y_K, float64 [B, n]) and, with f1=True, f1_tallies (int32 [B, 3], see macro_f1) hold its results; read them
    after a synchronisation of your choosing.

    bn_updates is passed to surrogate_grad: k > 0 folds the BatchNorm statistics of the step k times into model.bn_stats (the
    caveat of unrolled_grad applies: the reference's graph calls f K times on its way to the loss, and whether TensorFlow
    merges those identical x-only subgraphs is not pinned down, so the count is the caller's).

    eval_batch = E also allocates the script's test phase (multi-label-cls/icnn-back.py:208-216): evaluate(x, t)
    runs the context in eval_bn mode, gd.solve from y0 without a trajectory and the loss-only form of the feed
    (icnn_be_gd_eval, be_train_epoch.hip) on exactly E samples; it returns the float32 device scalar eval_loss, keeps y_eval
    and, with f1=True, eval_f1_tallies (eval_macro_f1() reads them), and changes no weight, optimiser state, statistic or
    result tensor of the training step.  eval_bn=None is what the script does at test time: "moving" (it sets
    is_training(False), :210); a model without BatchNorm ignores it."""
    _no_tallies = "F1 tallies are kept with f1=True only"
    _no_eval_tallies = "F1 tallies exist for a trainer constructed with f1=True and eval_batch only"

    def __init__(self, model, batch, n_iter=30, lr=0.01, momentum=0.9, adam_lr=1e-3, y0=0.5, bn_updates=0, f1=False,
                 eval_batch=None, eval_bn=None):
        if not isinstance(model, FCModel):
            name = model.__name__ if isinstance(model, type) else type(model).__name__
            raise TypeError("train.GDTrainer serves picnn.FCModel (ficnn.GDTrainer trains a FICNNModel), got %s" % name)
        if eval_bn is None:
            eval_bn = "moving"
        if eval_bn not in _lib.BN_MODE:
            raise ValueError("eval_bn must be 'batch' or 'moving', got %r" % (eval_bn,))
        super().__init__(model, batch, n_iter, lr, momentum, adam_lr, bn_updates, eval_batch)
        self.eval_bn = eval_bn if model.has_bn else "batch"         # without BatchNorm there is one context
        self.y0 = float(y0)
        B, E, dev = self.batch, self.eval_batch, self.device
        self.f1_tallies = torch.zeros(B, 3, dtype=torch.int32, device=dev) if f1 else None
        self.eval_f1_tallies = torch.zeros(E, 3, dtype=torch.int32, device=dev) if f1 and E is not None else None

    def _feed_work_bytes(self, rows, eval):
        lib = self.model._lib
        return lib.icnn_be_gd_eval_work_bytes(rows) if eval else lib.icnn_be_gd_feed_work_bytes(rows)

    def _start(self, eval):
        return self.y0

    def _feed(self, traj):
        _lib.check(self.model._lib.icnn_be_gd_feed(self.y.data_ptr(), self.t.data_ptr(), self._coef.data_ptr(), self.batch,
                                                   self.spec.n_labels, self.n_iter, self.scale, self.v_rows.data_ptr(),
                                                   self.c_rows.data_ptr(), self.row_offset.data_ptr(), self.loss.data_ptr(),
                                                   None if self.f1_tallies is None else self.f1_tallies.data_ptr(),
                                                   self._feed_work.data_ptr(), self._stream()), "icnn_be_gd_feed")

    def _eval_feed(self):
        _lib.check(self.model._lib.icnn_be_gd_eval(self.y_eval.data_ptr(), self.t_eval.data_ptr(), self.eval_batch,
                                                   self.spec.n_labels, self.eval_loss.data_ptr(),
                                                   None if self.eval_f1_tallies is None else self.eval_f1_tallies.data_ptr(),
                                                   self._feed_work_eval.data_ptr(), self._stream()), "icnn_be_gd_eval")


class ConvGDTrainer(UnrolledGDTrainer):
    """One training step of completion/icnn.back.py (:131-165 the graph, :210-239 the loop) on a picnn.ConvModel at one batch
    size, with the loss mean((pixel_scale (y_K - t))^2) of :149, all of it enqueued on the current stream without a host wait,
    so a step can be captured in a CUDA graph:

        context (batch statistics) -> gd.solve(trajectory=True) from y0 -> icnn_be_gd_feed_px (be_train_gd.hip: the loss, the
        rows v = coefficient x dL/dy_K, c = 0, row_offset) -> surrogate_grad over the B K trajectory rows -> DeviceAdam.step

    which is train.unrolled_grad with its torch elementwise launches folded into one kernel: the rows are the same bits, so
    grad and the update are those of the hand-composed step.  x is [B, H, W, 1]; its horizontal flip (icnn.back.py:220) is
    the CALLER's, as for ConvModel.context.  y0: a scalar, an [n] row (the reference's meanY), an image [H, W, 1] or a [B, n]
    array (images [B, H, W, 1] too); set_y0 replaces it, outside a capture.

    Constructing one ATTACHES the model to its DeviceAdam and allocates x, t, y0, the context, loss, the feed rows, the
    gradient and the workspaces.  step() returns the loss (before the update, as the reference's sess.run returns it) as a
    float32 device scalar.  After a step the device tensors loss, grad (flat), y (y_K, float64 [B, n]) and traj (y_0 .. y_{K-1},
    float64 [B, K, n]) hold its results; read them after a synchronisation of your choosing.  bn_updates is passed to surrogate_grad (unrolled_grad's caveat on
    the count applies).

    eval_batch = E also allocates the test phase (icnn.back.py:241-253): evaluate(x, t) runs the context with the MOVING
    BatchNorm statistics, gd.solve from y0 without a trajectory and the loss-only form of the feed on exactly E samples; it
    returns the float32 device scalar eval_loss, keeps y_eval, and changes no weight, optimiser state or statistic.  A
    [B, n] y0 serves the test phase only when E = B."""
    eval_bn = "moving"                                  # the script's test phase sets is_training(False)

    def __init__(self, model, batch, n_iter=30, lr=0.01, momentum=0.9, adam_lr=1e-3, y0=0.5, pixel_scale=255.0, bn_updates=0,
                 eval_batch=None):
        if not isinstance(model, ConvModel):
            name = model.__name__ if isinstance(model, type) else type(model).__name__
            raise TypeError("train.ConvGDTrainer serves picnn.ConvModel (train.GDTrainer trains an FCModel), got %s" % name)
        super().__init__(model, batch, n_iter, lr, momentum, adam_lr, bn_updates, eval_batch)
        self.px = float(np.float32(pixel_scale))
        self.traj = None                                # gd.solve's own trajectory tensor, from the first step on
        B, E, n, dev = self.batch, self.eval_batch, self.spec.n_labels, self.device
        self.y0 = torch.zeros(B, n, dtype=torch.float64, device=dev)
        if E is not None:
            self.y0_eval = torch.zeros(E, n, dtype=torch.float64, device=dev)
        self.set_y0(y0)

    def set_y0(self, y0):
        """The start point of step() and evaluate(): a scalar, an [n] row, an image [H, W, 1] or a [B, n] array ([B, H, W, 1]
        too).  A copy from the host: call it outside a capture."""
        n = self.spec.n_labels
        y0 = _start_point(y0, n, self.batch, self.eval_batch, self.device)
        y0 = torch.as_tensor(y0, dtype=torch.float64, device=self.device)      # a scalar is expanded like a row
        if self.eval_batch is not None:
            self.y0_eval.copy_(y0.expand(self.eval_batch, n))
        self.y0.copy_(y0.expand(self.batch, n))

    def _feed_work_bytes(self, rows, eval):
        return self.model._lib.icnn_be_gd_feed_px_work_bytes(rows, self.spec.n_labels, self.n_iter)

    def _start(self, eval):
        return self.y0_eval if eval else self.y0

    def _feed_px(self, y, t, B, loss, work, rows):
        v, c, off, coef = ((self.v_rows.data_ptr(), self.c_rows.data_ptr(), self.row_offset.data_ptr(), self._coef.data_ptr())
                           if rows else (None, None, None, None))
        # scale is 1 / (B n) of the TRAINING batch: the loss-only form does not read it
        _lib.check(self.model._lib.icnn_be_gd_feed_px(y.data_ptr(), t.data_ptr(), coef, B, self.spec.n_labels, self.n_iter,
                                                      self.scale, self.px, v, c, off, loss.data_ptr(), work.data_ptr(),
                                                      self._stream()), "icnn_be_gd_feed_px")

    def _feed(self, traj):
        self.traj = traj                                # kept: y_0 .. y_{K-1} of the last step
        self._feed_px(self.y, self.t, self.batch, self.loss, self._feed_work, True)

    def _eval_feed(self):
        self._feed_px(self.y_eval, self.t_eval, self.eval_batch, self.eval_loss, self._feed_work_eval, False)


# the epoch level names the trainers above, so its module is imported behind them; its classes are re-exported here
from .epoch import BestKeeper, DeviceDataset, EpochRunner, StepLog  # noqa: E402, F401
