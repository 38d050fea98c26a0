"""The FCN baseline of the completion experiment on the device: the model and the training loop of
completion/baseline.py around icnn_be_fcn_* (icnn_amd/csrc/be_fcn.hip), all float32.

On single-channel images [B, H, W] (torch's [B, 1, H, W]):
    conv1..3  3x3, stride 2, dilation 2, padding 2 (1 -> k, k -> k, k -> k): output i reads inputs 2i-2, 2i, 2i+2, so conv1
              reads only the even rows and columns of x -- the reference's behaviour, kept
    up1..3    transposed 3x3, stride 2, padding 1, output_padding 1 (k -> k): out[o] += in[i] w[t], o = 2i - 1 + t
    up4       transposed 1x1 (k -> 1);  ReLU behind every layer but up4;  yhat = up4's output
    loss = mean((pixel_scale (yhat - t))^2);  torch.optim.Adam(lr 1e-4): eps OUTSIDE the bias correction
One flat float32 vector theta in the order and layouts of torch's model.parameters() (a state_dict loads by concatenation):
conv<i>.weight [k, Cin, 3, 3], conv<i>.bias, up<i>.weight [Cin, Cout, 3, 3], up<i>.bias, up4.weight [k, 1, 1, 1], up4.bias.
The reference transposes its 64 x 32 images to 32 x 64; every kernel, stride, dilation and padding is square, so the net on
the untransposed images is the same family with transposed 3x3 kernels, and H = 64, W = 32 serves the data set as it is.
One step, enqueued on the current stream without a host synchronisation, is 16 launches: conv1, five gather products, the head
(up4, loss, d yhat), five data gradients, the weight-gradient partials, the channel sums, their reduction, Adam.
"""
import ctypes as C
import dataclasses
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import flat as _flat

LAYERS = ("conv1", "conv2", "conv3", "up1", "up2", "up3", "up4")


@dataclasses.dataclass(frozen=True)
class FCNSpec:
    H: int
    W: int
    k: int = 32


def olivetti_fcn_spec() -> FCNSpec:
    """baseline.py's FCN(k=32) on the left halves of the Olivetti faces as DeviceDataset holds them: 64 rows of 32 pixels"""
    return FCNSpec(64, 32, 32)


def layout(spec):
    """[(name, shape)] of the variables in the order of the flat vector: torch's names and layouts"""
    k, out = spec.k, []
    for name in LAYERS:
        if name == "up4":
            shape = (k, 1, 1, 1)
        elif name == "conv1":
            shape = (k, 1, 3, 3)
        else:
            shape = (k, k, 3, 3)
        out += [(name + ".weight", shape), (name + ".bias", (shape[1] if name == "up4" else k,))]
    return out


def n_floats(spec) -> int:
    return _flat.n_floats(layout(spec))


def flatten(spec, params) -> np.ndarray:
    return _flat.flatten(layout(spec), params)


def unflatten(spec, flat) -> Dict[str, np.ndarray]:
    return _flat.unflatten(layout(spec), flat)


def fan_in(name, shape) -> int:
    """torch's: weight.size(1) x kh x kw, so the transposed convolutions count their OUTPUT channels"""
    return shape[1] * shape[2] * shape[3]


def init_params(spec, seed) -> Dict[str, np.ndarray]:
    """torch's default of both layer kinds with NumPy's stream, drawn in the order of the flat vector: weight and bias of a
    layer uniform in +-1/sqrt(fan_in); float32.  Not bit-equal to torch.manual_seed."""
    rng = np.random.RandomState(seed)
    out, r = {}, 0.0
    for name, shape in layout(spec):
        if name.endswith(".weight"):
            r = 1.0 / np.sqrt(fan_in(name, shape))
        out[name] = rng.uniform(-r, r, shape).astype(np.float32)
    return out


def _dims(spec):
    return (int(spec.H), int(spec.W), int(spec.k))


class FCNModel:
    """The flat theta on the device.  params: a dict of torch-named arrays (a state_dict's tensors as arrays) or a flat vector;
    None: init_params(spec, seed)."""

    def __init__(self, spec, params=None, seed=0, device="cuda"):
        self.spec, self.device = spec, torch.device(device)
        self._lib = _lib.load()
        n = C.c_longlong()
        if self._lib.icnn_be_fcn_param_floats(*_dims(spec), C.byref(n)) != 0:
            raise ValueError("sizes beyond what the FCN kernels support (k a multiple of 16 in [16, %d], H and W multiples of 8 "
                             "in [8, %d]): %r" % (_lib.FCN_MAX_K, _lib.FCN_MAX_HW, spec))
        self.n = int(n.value)
        assert self.n == n_floats(spec)
        self.theta = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.load(init_params(spec, seed) if params is None else params)

    def load(self, params):
        """copy a dict of torch-named arrays (or a flat vector) into the existing theta"""
        if isinstance(params, dict):
            params = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in params.items()}
        _flat.copy_into(self.theta, layout(self.spec), params, "theta")

    load_state_dict = load

    def host_params(self) -> Dict[str, np.ndarray]:
        return unflatten(self.spec, self.theta.cpu().numpy())

    def work(self, batch) -> torch.Tensor:
        """a zeroed workspace for `batch` images"""
        nbytes = self._lib.icnn_be_fcn_work_bytes(int(batch), *_dims(self.spec))
        if nbytes == 0:
            raise ValueError("batch must lie in [1, %d], got %r" % (_lib.FCN_MAX_EVAL_BATCH, batch))
        return torch.zeros(nbytes // 4, dtype=torch.float32, device=self.device)

    def args(self, batch, work) -> "_lib.FcnArgs":
        """the descriptor of this model at one batch size, without data and optimiser pointers"""
        a = _lib.FcnArgs()
        a.batch, a.H, a.W, a.k = int(batch), self.spec.H, self.spec.W, self.spec.k
        a.theta, a.work = self.theta.data_ptr(), work.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps, a.pixel_scale = 1e-4, 0.9, 0.999, 1e-8, 255.0
        return a

    def predict(self, x) -> torch.Tensor:
        """yhat [B, H * W] for x [B, H, W] (or [B, H, W, 1], [B, H * W]) float32 on the device, without targets.  Nothing of
        the model is written.  No host synchronisation."""
        assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
        B = x.shape[0]
        assert x.numel() == B * self.spec.H * self.spec.W
        work = self.work(B)
        out = torch.empty(B, self.spec.H * self.spec.W, dtype=torch.float32, device=self.device)
        a = self.args(B, work)
        a.x, a.yhat = x.data_ptr(), out.data_ptr()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self._lib.icnn_be_fcn_forward(C.byref(a), stream), "icnn_be_fcn_forward")
        return out


class FCNTrainer(_flat.SupervisedTrainer):
    """model, Adam's state and the whole training step at one batch size.  step() returns the loss at the weights the step
    began with: the trainer's 0-d float32 device tensor `loss`; yhat [B, H * W] is that of the same forward.  eval_batch = E
    also allocates the script's test phase (baseline.py:102-108): evaluate(x, t) runs forward and loss on exactly E images
    into eval_loss and y_eval and changes nothing else.  grad holds the last step's flat gradient, work_view(name) the pieces of
    the workspace (_lib.FCN_WORK).  x is [B, H, W, 1] and t [B, H * W], the buffers of ConvGDTrainer."""
    _entry, _key, _work_names, _step_ints = "icnn_be_fcn_", "fcn", _lib.FCN_WORK, _lib.FCN_STEP_INTS
    _fields = ("x", "t", "yhat", "loss")
    _eval_fields = ("x_eval", "t_eval", "y_eval", "eval_loss")
    _extra = ("lr", "pixel_scale")
    _layout, _dims = staticmethod(layout), staticmethod(_dims)

    def __init__(self, model, batch, lr=1e-4, pixel_scale=255.0, eval_batch=None):
        if not isinstance(model, FCNModel):
            raise TypeError("fcn.FCNTrainer serves fcn.FCNModel, got %s" % type(model).__name__)
        if not 1 <= int(batch) <= _lib.FCN_MAX_BATCH:
            raise ValueError("batch must lie in [1, %d], got %r" % (_lib.FCN_MAX_BATCH, batch))
        eval_batch = _flat._eval_batch(eval_batch, most=_lib.FCN_MAX_EVAL_BATCH)
        if not pixel_scale > 0:
            raise ValueError("pixel_scale must be positive, got %r" % (pixel_scale,))
        self.lr, self.pixel_scale = float(lr), float(pixel_scale)
        super().__init__(model, int(batch), eval_batch)

    def _buffers(self, rows):
        f32, dev, H, W = torch.float32, self.device, self.spec.H, self.spec.W
        return (torch.zeros(rows, H, W, 1, dtype=f32, device=dev), torch.zeros(rows, H * W, dtype=f32, device=dev),
                torch.zeros(rows, H * W, dtype=f32, device=dev), torch.zeros((), dtype=f32, device=dev))

    def piece_shape(self, name, batch):
        """the shape of a piece of the workspace that holds images: "h<i>", "dz<i>" [B, h, w, k], "dy" [B, H, W]"""
        H, W, k = self.spec.H, self.spec.W, self.spec.k
        if name == "dy":
            return (batch, H, W)
        div = (2, 4, 8, 4, 2, 1)[int(name[-1])]
        return (batch, H // div, W // div, k)

    def work_view(self, name, eval=False) -> torch.Tensor:
        """a live view of one piece of the workspace (of evaluate()'s with eval=True): see piece_shape; "wpart", "lpart" and
        "ctl" come flat up to the next piece"""
        B = self.eval_batch if eval else self.batch
        work = self.eval_work if eval else self.work
        offsets = self._offsets(B) if eval else self.work_offsets
        at = offsets[name]
        if name in ("wpart", "lpart", "ctl"):
            later = [o for o in offsets.values() if o > at]
            return work[at:min(later) if later else work.numel()]
        shape = self.piece_shape(name, B)
        return work[at:at + int(np.prod(shape))].view(shape)
