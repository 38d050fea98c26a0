"""The fully input-convex network (FICNN) of the synthetic classification experiment on the device.

synthetic-cls/icnn.py:213-234 (f_ficnn), with xy = concat(x, y) and tflearn fully_connected layers:

    for i, sz in enumerate(szs + [1]):
        a_i = xy @ z_x{i}/W + z_x{i}/b  (+ z_{i-1} @ z_z{i}_proj/W  for i > 0, no bias)
        if sz != 1: z_i = relu(a_i)
    return flatten(z)

The last layer never reassigns z, so the reference returns the last HIDDEN layer and tf.gradients(E, y) sums over it:
head="sum" (the default) is that energy, E = sum_k z_{L-1,k}; its head variables exist and get no gradient.
head="linear" is the paper's FICNN, E = a_L.  Both are jointly convex in (x, y) once the proj weights are >= 0.

    FICNNModel   the packed weights and the C descriptor: context(x) (be_ficnn.hip, one f32-MFMA GEMM), fg(ctx, y)
                 (ficnn_fg_kernel), solveBatch(f=model) through icnn_be_solve_ficnn, gd.solve through icnn_be_ficnn_gd,
                 train.surrogate_grad / unrolled_grad through icnn_be_ficnn_surrogate_grad, and the arena hooks that
                 train.DeviceAdam attaches to
    GDTrainer    the script's whole training step (:117-139, :189-194) as enqueued work
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib, gd, picnn, train
from .flat import _positive, _Trainer
from .picnn import _DeviceWeights, _host_ptr, _trunc_normal


@dataclass(frozen=True)
class FICNNSpec:
    """Shape of one FICNN: `szs` are the hidden widths (the reference's [200, 200]; the scalar layer is appended)."""
    n_features: int
    n_labels: int
    szs: tuple
    head: str = "sum"

    def __post_init__(self):
        if self.head not in _lib.FICNN_HEAD:
            raise ValueError("head must be 'sum' or 'linear', got %r" % (self.head,))

    @property
    def widths(self) -> List[int]:
        return list(self.szs) + [1]

    @property
    def n_layers(self) -> int:
        return len(self.szs) + 1

    @property
    def evaluated(self) -> int:
        """layers whose pre-activation reaches E: the hidden ones, and the scalar one for head 'linear'"""
        return len(self.szs) + (1 if self.head == "linear" else 0)

    @property
    def ctx_offsets(self) -> List[int]:
        w, offs, o = self.widths, [], 0
        for i in range(self.evaluated):
            offs.append(o)
            o += w[i]
        return offs

    @property
    def ctx_width(self) -> int:
        return sum(self.widths[:self.evaluated])

    def grad_layout(self) -> List[Tuple[str, tuple]]:
        return grad_layout(self)


def synthetic_spec(head="sum") -> FICNNSpec:
    """synthetic-cls defaults: 2-d points, one label, hidden layers [200, 200] (icnn.py:217)"""
    return FICNNSpec(2, 1, (200, 200), head)


def grad_layout(spec: FICNNSpec) -> List[Tuple[str, tuple]]:
    """(name, shape) of every variable in the order of tf.trainable_variables() (include/icnn_be.h)."""
    out, w = [], spec.widths
    for i in range(spec.n_layers):
        out += [("z_x%d/W" % i, (spec.n_features + spec.n_labels, w[i])), ("z_x%d/b" % i, (w[i],))]
        if i > 0:
            out.append(("z_z%d_proj/W" % i, (w[i - 1], w[i])))
    return out


def init_params(spec: FICNNSpec, seed=0) -> Dict[str, np.ndarray]:
    """tflearn's defaults: truncated normal std 0.02, zero biases (makeCvx is a separate step: make_convex)."""
    rng = np.random.RandomState(seed)
    p = {}
    for name, shape in grad_layout(spec):
        p[name] = np.zeros(shape, np.float32) if name.endswith("/b") else _trunc_normal(rng, shape, 0.02)
    return p


def make_convex(params):
    """reference `makeCvx` (icnn.py:145): |W| / 10 on every 'proj' weight"""
    return picnn.make_convex(params, 10.0)


def project(params):
    """reference `proj` (icnn.py:146): max(W, 0) on every 'proj' weight"""
    return picnn.project(params)


class FICNNModel(_DeviceWeights):
    """Device-resident FICNN: every weight the kernels read packed into one buffer (context rows, MFMA fragments of the
    y- and z-weights in both orientations, head vectors) and the C descriptor.  Re-create, call `repack`, or attach a
    train.DeviceAdam after every weight update."""
    solve_entry, gd_entry = "icnn_be_solve_ficnn", "icnn_be_ficnn_gd"
    grad_entry, grad_floats_entry = "icnn_be_ficnn_surrogate_grad", "icnn_be_ficnn_grad_floats"

    def __init__(self, spec: FICNNSpec, params, device="cuda"):
        self.spec = spec
        self.device = torch.device(device)
        self._lib = _lib.load()
        m = _lib.FicnnModel()
        m.n_features, m.n, m.n_layers = spec.n_features, spec.n_labels, spec.n_layers
        for i, w in enumerate(spec.widths):
            m.width[i] = w
        m.head = _lib.FICNN_HEAD[spec.head]
        m.ctx_width = spec.ctx_width
        m.wpack = None
        self.c_model = m
        n_floats = self._lib.icnn_be_ficnn_pack_floats(C.byref(m))
        if n_floats == 0:
            raise ValueError("model shape rejected by libicnn_be (layer count / widths / LDS budget)")
        self.n_pack_floats = int(n_floats)
        self.repack(params)

    def _descriptors(self):
        return (C.byref(self.c_model),)

    def check_x(self, x):
        assert x.dim() == 2 and x.shape[1] == self.spec.n_features

    # ---- weights -------------------------------------------------------------------------------------------
    def _pack_host(self, params) -> np.ndarray:
        """icnn_be_ficnn_pack of params: the host image of wpack (a copy of parameter elements, zeros elsewhere)"""
        L1, ptr = self.spec.n_layers, _host_ptr(params)
        wx = (C.c_void_p * L1)(*[ptr("z_x%d/W" % i) for i in range(L1)])
        b = (C.c_void_p * L1)(*[ptr("z_x%d/b" % i) for i in range(L1)])
        wz = (C.c_void_p * L1)(*([None] + [ptr("z_z%d_proj/W" % i) for i in range(1, L1)]))
        host = np.empty(self.n_pack_floats, dtype=np.float32)
        _lib.check(self._lib.icnn_be_ficnn_pack(C.byref(self.c_model), wx, b, wz, host.ctypes.data), "icnn_be_ficnn_pack")
        return host

    def arena_parts(self, params):
        """the weight-arena hooks of train.DeviceAdam: one buffer, the pack"""
        return [("wpack", 0, self._pack_host(params))]

    # ---- evaluation ----------------------------------------------------------------------------------------
    def context(self, x: torch.Tensor) -> torch.Tensor:
        """x-only context rows [B, ctx_width] (c_i = x Wx_i + b_i) of x [B, n_features]; current stream."""
        x = x.to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        self.check_x(x)
        ctx = torch.empty(B, self.spec.ctx_width, dtype=torch.float32, device=self.device)
        work = torch.empty(max(int(self._lib.icnn_be_ficnn_context_work_floats(C.byref(self.c_model), B)), 1),
                           dtype=torch.float32, device=self.device)
        _lib.check(self._lib.icnn_be_ficnn_context(C.byref(self.c_model), x.data_ptr(), B, ctx.data_ptr(), work.data_ptr(),
                                                   self._stream()), "icnn_be_ficnn_context")
        return ctx

    def fg(self, ctx: torch.Tensor, y: torch.Tensor, finished=None):
        """E[B] float32 and dE/dy[B, n] float32 at y (float64 [B, n]) on the current stream (rows with finished != 0 are
        not written: use fg_into to keep their previous values)."""
        B = y.shape[0]
        assert y.dtype == torch.float64 and y.is_contiguous() and ctx.is_contiguous()
        assert ctx.shape == (B, self.spec.ctx_width) and ctx.dtype == torch.float32
        f = torch.empty(B, dtype=torch.float32, device=self.device)
        g = torch.empty(B, self.spec.n_labels, dtype=torch.float32, device=self.device)
        self.fg_into(ctx, y, f, g, finished)
        return f, g

    def fg_into(self, ctx, y, f, g, finished=None):
        """fg writing into caller buffers f [B] / g [B, n] (float32): rows with finished != 0 keep what they hold"""
        B = y.shape[0]
        assert f.dtype == g.dtype == torch.float32 and f.shape == (B,) and g.shape == (B, self.spec.n_labels)
        if finished is not None:
            assert finished.dtype == torch.int32 and finished.shape == (B,)
        _lib.check(self._lib.icnn_be_ficnn_fg(C.byref(self.c_model), ctx.data_ptr(), y.data_ptr(), B, f.data_ptr(),
                                              g.data_ptr(), None if finished is None else finished.data_ptr(),
                                              self._stream()), "icnn_be_ficnn_fg")


def surrogate_grad(model: FICNNModel, x: torch.Tensor, row_offset: torch.Tensor, y: torch.Tensor, v, c: torch.Tensor,
                   F_rows=None, flat=False):
    """train.surrogate_grad for a FICNNModel (icnn_be_ficnn_surrogate_grad); arguments already on the device."""
    rows = (y, c) if v is None else (y, v, c)
    return train.surrogate_grad(model, x, rows, row_offset=row_offset, F_rows=F_rows, flat=flat)


class GDTrainer(_Trainer):
    """The synthetic-cls training step (icnn.py:117-139, :189-194) at one batch size, all of it enqueued on the device:
    context, gd.solve(trajectory=True) from y0 = 0.5, the loss mean((y_K - t)^2) over B n and its adjoint
    ybar = float32(1/(B n)) (2 (y_K - t)) (TensorFlow's _MeanGrad / _SquareGrad), train.unrolled_grad, then DeviceAdam.step
    (TF-Adam and the reference's proj).  Constructing one ATTACHES the model to its DeviceAdam.  step() returns the loss
    (before the update, as the reference's sess.run returns it) as a float32 device scalar; no host synchronisation, so a
    step can be captured in a CUDA graph."""

    def __init__(self, model: FICNNModel, batch: int, n_iter=30, lr=0.01, momentum=0.9, adam_lr=1e-3, y0=0.5):
        self.model, self.spec, self.device = model, model.spec, model.device
        self.batch = _positive("batch", batch)
        self.n_iter, self.lr, self.momentum, self.y0 = int(n_iter), float(lr), float(momentum), float(y0)
        self.opt = train.DeviceAdam(model, lr=adam_lr)
        B, dev = self.batch, self.device
        self.x = torch.zeros(B, self.spec.n_features, dtype=torch.float32, device=dev)
        self.t = torch.zeros(B, self.spec.n_labels, dtype=torch.float32, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.inv_count = float(np.float32(1.0) / np.float32(B * self.spec.n_labels))
        train.unrolled_coefficients(self.n_iter, self.lr, self.momentum, dev)      # uploaded now, not inside a capture

    def step(self, x=None, t=None) -> torch.Tensor:
        """One step on (x [B, n_features], t [B, n]); None keeps the batch of the previous call (graph replay)."""
        self._put(self.x, x)
        self._put(self.t, t)
        ctx = self.model.context(self.x)
        yK, traj, _ = gd.solve(self.model, ctx, self.y0, self.n_iter, self.lr, self.momentum, trajectory=True)
        d = yK.to(torch.float32) - self.t
        self.loss.copy_(torch.mean(d * d))
        ybar = (d * 2.0) * self.inv_count
        grad = train.unrolled_grad(self.model, self.x, traj, ybar.to(torch.float64), self.lr, self.momentum, flat=True)
        self.opt.step(grad)
        return self.loss
