"""The feed-forward baseline of the multi-label experiment on the device: the model and the training loop of
multi-label-cls/ff.py around icnn_be_ff_* (icnn_amd/csrc/be_ff.hip), all float32.

L = len(layer_sizes) hidden layers; w_0 = n_features:
    a_i = relu(h_{i-1} W_i + b_i),  h_i = (a_i - mu_i) gamma_i / sqrt(sigma2_i + 1e-5) + beta_i,  h_0 = x
    yhat = sigmoid(h_L W_o + b_o),  loss = -sum y log(yhat + 1e-10) - sum (1 - y) log(1 - yhat + 1e-10)   (a SUM)
One flat float32 vector theta: for i = 1..L  W_i [w_{i-1}, w_i], b_i, gamma_i, beta_i;  then W_o [w_L, n_labels], b_o.
In training mode (mu, sigma2) are the batch mean and the biased batch variance, and a step folds them once into the moving
pair of every layer (decay 0.9); in inference mode the moving pair normalises and nothing is written.  One step, enqueued on
the current stream without a host synchronisation (a captured step replayed k times is k steps), 2 L + 4 launches:
    L layer forwards, the head (yhat, loss, tallies, d loss / d logits), L layer backwards, the weight gradients, one TF-Adam
    (lr 1e-3, betas 0.9 / 0.999, eps 1e-8) over theta, the fold
"""
import ctypes as C
import dataclasses
from typing import Dict, Tuple

import numpy as np
import torch

from . import _lib
from . import flat as _flat

BN_EPS = 1e-5


@dataclasses.dataclass(frozen=True)
class FFSpec:
    n_features: int
    n_labels: int
    layer_sizes: Tuple[int, ...] = (600,)

    def __post_init__(self):
        object.__setattr__(self, "layer_sizes", tuple(int(w) for w in self.layer_sizes))


def bibtex_ff_spec() -> FFSpec:
    """ff.py's defaults on Bibtex: 1836 features, 159 labels, one hidden layer of 600"""
    return FFSpec(1836, 159, (600,))


def layout(spec):
    """[(name, shape)] of the variables in the order of the flat vector"""
    out, w_in = [], spec.n_features
    for i, w in enumerate(spec.layer_sizes, 1):
        out += [("W%d" % i, (w_in, w)), ("b%d" % i, (w,)), ("gamma%d" % i, (w,)), ("beta%d" % i, (w,))]
        w_in = w
    return out + [("Wo", (w_in, spec.n_labels)), ("bo", (spec.n_labels,))]


def n_floats(spec) -> int:
    return _flat.n_floats(layout(spec))


def flatten(spec, params) -> np.ndarray:
    return _flat.flatten(layout(spec), params)


def unflatten(spec, flat) -> Dict[str, np.ndarray]:
    return _flat.unflatten(layout(spec), flat)


def init_params(spec, seed) -> Dict[str, np.ndarray]:
    """ff.py:114-126 with NumPy's stream, drawn in the order of the flat vector: W and b of a layer uniform in
    +-1/sqrt(the layer's OUTPUT width) (the logits layer: n_labels), gamma ~ N(1, 0.002), beta = 0; float32."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in layout(spec):
        if name[0] in "Wb" and not name.startswith("beta"):
            r = 1.0 / np.sqrt(shape[-1])
            out[name] = rng.uniform(-r, r, shape).astype(np.float32)
        elif name.startswith("gamma"):
            out[name] = (1.0 + 0.002 * rng.standard_normal(shape)).astype(np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


def _widths(spec):
    return (C.c_int * _lib.FF_MAX_LAYERS)(*spec.layer_sizes)


def _dims(spec):
    return (spec.n_features, spec.n_labels, len(spec.layer_sizes), _widths(spec))


class FFModel:
    """The flat theta on the device, the moving statistics bn_stats {"mean<i>", "var<i>"} of hidden layer i + 1 (mean 0,
    variance 1 at the start) and bn_decay.  params: a dict of named arrays or a flat vector; None: init_params(spec, seed)."""
    has_bn = True

    def __init__(self, spec, params=None, seed=0, device="cuda", bn_decay=0.9):
        if not 1 <= len(spec.layer_sizes) <= _lib.FF_MAX_LAYERS:
            raise ValueError("1 to %d hidden layers, got %d" % (_lib.FF_MAX_LAYERS, len(spec.layer_sizes)))
        if not 0.0 <= bn_decay <= 1.0:
            raise ValueError("bn_decay must lie in [0, 1], got %r" % (bn_decay,))
        self.spec, self.device, self.bn_decay = spec, torch.device(device), float(bn_decay)
        self._lib = _lib.load()
        n = C.c_longlong()
        if self._lib.icnn_be_ff_param_floats(*_dims(spec), C.byref(n)) != 0:
            raise ValueError("sizes beyond what the feed-forward kernels support: %r" % (spec,))
        self.n = int(n.value)
        assert self.n == n_floats(spec)
        self.theta = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.bn_stats = {}
        for i, w in enumerate(spec.layer_sizes):
            self.bn_stats["mean%d" % i] = torch.zeros(w, dtype=torch.float32, device=self.device)
            self.bn_stats["var%d" % i] = torch.ones(w, dtype=torch.float32, device=self.device)
        self.load(init_params(spec, seed) if params is None else params)

    def load(self, params):
        """copy a dict of named arrays (or a flat vector) into the existing theta"""
        _flat.copy_into(self.theta, layout(self.spec), params, "theta")

    def host_params(self) -> Dict[str, np.ndarray]:
        return unflatten(self.spec, self.theta.cpu().numpy())

    def work(self, batch) -> torch.Tensor:
        """a zeroed workspace for `batch` rows"""
        nbytes = self._lib.icnn_be_ff_work_bytes(int(batch), *_dims(self.spec))
        if nbytes == 0:
            raise ValueError("batch must be >= 1, got %r" % (batch,))
        return torch.zeros(nbytes // 4, dtype=torch.float32, device=self.device)

    def args(self, batch, work) -> "_lib.FfArgs":
        """the descriptor of this model at one batch size, without data and optimiser pointers"""
        a = _lib.FfArgs()
        a.batch, a.n_features, a.n_labels, a.n_layers = int(batch), self.spec.n_features, self.spec.n_labels, len(self.spec.layer_sizes)
        a.width = _widths(self.spec)
        a.theta, a.work = self.theta.data_ptr(), work.data_ptr()
        for i in range(a.n_layers):
            a.mv.mean[i] = self.bn_stats["mean%d" % i].data_ptr()
            a.mv.var[i] = self.bn_stats["var%d" % i].data_ptr()
        a.mv.decay = self.bn_decay
        a.lr, a.beta1, a.beta2, a.eps, a.bn_eps = 1e-3, 0.9, 0.999, 1e-8, BN_EPS
        return a

    def predict(self, x, bn="moving") -> torch.Tensor:
        """yhat [B, n_labels] for x [B, n_features] float32 on the device; bn "moving" (inference mode, any B) or "batch" (the
        statistics of this batch, 2 <= B <= 512).  Nothing of the model is written.  No host synchronisation."""
        if bn not in _lib.BN_MODE:
            raise ValueError("bn must be 'batch' or 'moving', got %r" % (bn,))
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2 and x.shape[1] == self.spec.n_features and x.is_cuda
        work = self.work(x.shape[0])
        out = torch.empty(x.shape[0], self.spec.n_labels, dtype=torch.float32, device=self.device)
        a = self.args(x.shape[0], work)
        a.x, a.yhat = x.data_ptr(), out.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self._lib.icnn_be_ff_forward(C.byref(a), _lib.BN_MODE[bn], stream), "icnn_be_ff_forward")
        return out


class FFTrainer(_flat.SupervisedTrainer, _flat._TrainF1):
    """model, Adam's state and the whole training step at one batch size.  step() returns the loss at the weights the step
    began with: the trainer's 0-d float32 device tensor `loss`; yhat [B, n_labels] and f1_tallies [B, 3] (tp, fp, fn per
    example; macro_f1() reads them) are those of the same forward.  eval_batch = E also allocates the script's test phase
    (ff.py:187-196): evaluate(x, true_y) runs inference mode on exactly E samples into eval_loss, eval_yhat, eval_f1_tallies and
    changes nothing else.  grad holds the last step's flat gradient, work_view(name) the pieces of the workspace
    (_lib.FF_WORK).  x is [B, n_features] and true_y [B, n_labels]."""
    _no_tallies = "the feed-forward trainer always keeps its tallies"
    _entry, _key, _work_names, _step_ints = "icnn_be_ff_", "ff", _lib.FF_WORK, _lib.FF_STEP_INTS
    _fields = ("x", "true_y", "yhat", "loss", "f1_tallies")
    _eval_fields = ("x_eval", "true_y_eval", "eval_yhat", "eval_loss", "eval_f1_tallies")
    _extra = ("lr",)
    _layout, _dims = staticmethod(layout), staticmethod(_dims)

    def __init__(self, model, batch, lr=1e-3, eval_batch=None):
        if not isinstance(model, FFModel):
            raise TypeError("ff.FFTrainer serves ff.FFModel, got %s" % type(model).__name__)
        if not 2 <= int(batch) <= _lib.FF_MAX_BATCH:
            raise ValueError("batch must lie in [2, %d], got %r" % (_lib.FF_MAX_BATCH, batch))
        self.lr = float(lr)
        super().__init__(model, int(batch), _flat._eval_batch(eval_batch))

    def _buffers(self, rows):
        f32, dev, spec = torch.float32, self.device, self.spec
        return (torch.zeros(rows, spec.n_features, dtype=f32, device=dev), torch.zeros(rows, spec.n_labels, dtype=f32, device=dev),
                torch.zeros(rows, spec.n_labels, dtype=f32, device=dev), torch.zeros((), dtype=f32, device=dev),
                torch.zeros(rows, 3, dtype=torch.int32, device=dev))

    def forward(self, bn="batch"):
        """icnn_be_ff_forward alone on the trainer's buffers: the workspace, yhat, loss, f1_tallies"""
        _lib.check(self.lib.icnn_be_ff_forward(C.byref(self._args), _lib.BN_MODE[bn], self._stream()), "icnn_be_ff_forward")

    def work_view(self, name, eval=False) -> torch.Tensor:
        """a live view of one piece of the workspace (of evaluate()'s with eval=True): "a<i>", "h<i>", "dz<i>" [B, width],
        "stat<i>" [2, width] (mu, sigma2), "dlogit" [B, n_labels]"""
        B = self.eval_batch if eval else self.batch
        work = self.eval_work if eval else self.work
        at = (self._offsets(B) if eval else self.work_offsets)[name]
        if name == "dlogit":
            rows, width = B, self.spec.n_labels
        else:
            width = self.spec.layer_sizes[int(name[-1])]
            rows = 2 if name.startswith("stat") else B
        return work[at:at + rows * width].view(rows, width)
