"""What the trainers share, and no trainer of its own: this module imports none of them.

The flat-vector trainers (ddpg.py, naf.py, ff.py, fcn.py; checkpoint.FLAT_TRAINERS): a net is ONE float32 vector, the
variables of a layout [(name, shape)] end to end, each in C order; the kernels read that vector as it lies.  Every layout
stays with its module; here are the vector's arithmetic and the scaffold of a trainer around a C descriptor (FlatTrainer),
with ReplayTrainer for the two RL agents and SupervisedTrainer for the two supervised baselines.

Every trainer with a batch (train.py, ficnn.py, ff.py, fcn.py, rl_train.py): the argument checks, the start point, the batch
and context buffers (_Trainer), the test phase's checks (_eval_batch, _Trainer._require_eval) and the F1 of the tallies
(macro_f1, _TrainF1).
"""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import _lib


def n_floats(layout) -> int:
    return sum(int(np.prod(shape)) for _, shape in layout)


def flatten(layout, params, prefix="") -> np.ndarray:
    """the flat float32 vector of a dict of named arrays; prefix: what an error puts in front of the variable's name"""
    parts = []
    for name, shape in layout:
        a = np.asarray(params[name], np.float32)
        if a.shape != shape:
            raise ValueError("%s%s: shape %s, expected %s" % (prefix, name, a.shape, shape))
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def _pieces(layout, flat, shaped):
    out, at = {}, 0
    for name, shape in layout:
        n = int(np.prod(shape))
        out[name] = shaped(flat[at:at + n], shape)
        at += n
    return out


def unflatten(layout, flat) -> Dict[str, np.ndarray]:
    """copies of the variables inside a flat vector"""
    return _pieces(layout, flat, lambda piece, shape: np.asarray(piece).reshape(shape).copy())


def views(layout, tensor) -> Dict[str, torch.Tensor]:
    """live views of the variables inside a flat tensor"""
    return _pieces(layout, tensor, lambda piece, shape: piece.view(shape))


def copy_into(tensor, layout, params, what, prefix=""):
    """Copy a dict of named arrays (flatten's arguments) or a flat vector into the existing flat tensor.  what: the name of
    the tensor in the error of a wrong length."""
    flat = flatten(layout, params, prefix) if isinstance(params, dict) else np.asarray(params, np.float32)
    if flat.shape != (tensor.numel(),):
        raise ValueError("%s: %s values, expected %d" % (what, flat.shape, tensor.numel()))
    tensor.copy_(torch.from_numpy(np.ascontiguousarray(flat)))


# --------------------------------------------------------------------------------------------- #
# What the trainers share round their step(): argument checks, buffers, the start point, the optimiser's views
# --------------------------------------------------------------------------------------------- #
_NO_EVAL = "evaluate() needs a trainer constructed with eval_batch"


def _positive(name, value) -> int:
    value = int(value)
    if value < 1:
        raise ValueError("%s must be >= 1" % name)
    return value


def _non_negative(name, value) -> int:
    value = int(value)
    if value < 0:
        raise ValueError("%s must be >= 0, got %d" % (name, value))
    return value


def _eval_batch(eval_batch, most=None):
    """a trainer's eval_batch argument: None (no test phase) or an int >= 1, at most `most` where the kernels set a limit"""
    if eval_batch is None:
        return None
    eval_batch = int(eval_batch)
    if most is None and eval_batch < 1:
        raise ValueError("eval_batch must be >= 1, got %d" % eval_batch)
    if most is not None and not 1 <= eval_batch <= most:
        raise ValueError("eval_batch must lie in [1, %d], got %d" % (most, eval_batch))
    return eval_batch


def _ticket(n_bytes, device) -> torch.Tensor:
    """the workspace of a feed kernel, zeroed once: it holds the ticket its blocks count themselves with"""
    return torch.zeros((int(n_bytes) + 7) // 8, dtype=torch.float64, device=device)


def _start_point(y0, n, batch, eval_batch, device):
    """A trainer's start point y0 -- a scalar, an [n] row, an image [H, W, 1] or a [B, n] array ([B, H, W, 1] too) -- as a
    Python float (a scalar) or a float64 tensor on `device` that expands to [rows, n]: [n], or [B, n], which serves the
    test phase only when eval_batch == batch."""
    y0 = torch.as_tensor(y0, dtype=torch.float64)
    if y0.dim() == 0:
        return float(y0)
    y0 = y0.to(device)
    if y0.dim() >= 3 and y0.numel() % n == 0:           # an image, or one per sample
        y0 = y0.reshape(-1, n)
    if y0.dim() == 2 and y0.shape[0] == 1:
        y0 = y0[0]
    if y0.dim() > 2 or y0.shape[-1] != n or (y0.dim() == 2 and y0.shape[0] != batch):
        raise ValueError("y0 is a scalar, an [n] row, an [H, W, 1] image or a [B, n] array (n = %d, B = %d), got %s"
                         % (n, batch, tuple(y0.shape)))
    if eval_batch is not None and y0.dim() == 2 and eval_batch != batch:
        raise ValueError("a per-sample y0 [B, n] serves evaluate() only when eval_batch == batch")
    return y0


def macro_f1(tallies) -> float:
    """util.macroF1 of the reference from per-example tallies [B, 3] (tp, fp, fn over the labels of each example, prediction
    y >= 0.5): that function transposes both arrays before sklearn's f1_score(average='macro'), so sklearn's classes are the
    EXAMPLES and the macro average runs over them -- mean over examples of 2 tp / (2 tp + fp + fn), 0 where the denominator
    is 0 (an example without a positive label or prediction).  Host arithmetic; a device tensor is copied (one wait)."""
    t = tallies.detach().cpu().numpy() if torch.is_tensor(tallies) else np.asarray(tallies)
    t = t.reshape(-1, 3).astype(np.float64)
    if t.shape[0] == 0:
        return 0.0
    den = 2.0 * t[:, 0] + t[:, 1] + t[:, 2]
    f1 = np.where(den > 0, 2.0 * t[:, 0] / np.where(den > 0, den, 1.0), 0.0)
    return float(f1.mean())


class _Trainer:
    """The scaffolding of a trainer that owns `model`, `device` and the DeviceAdam `opt`; its pipeline is its own step()."""

    def _put(self, buf, value):
        """copy a batch into its preallocated buffer; None keeps what the buffer holds (graph replay)"""
        if value is not None:
            buf.copy_(torch.as_tensor(value).to(self.device, buf.dtype).reshape(buf.shape))

    def _context_buffers(self, batch):
        """(ctx, work) of model.context(x, out=, work=) at this batch size"""
        return (torch.empty(batch, self.spec.ctx_width, dtype=torch.float32, device=self.device),
                torch.empty(self.model.context_work_floats(batch), dtype=torch.float32, device=self.device))

    def _require_eval(self):
        """the refusal of evaluate() on a trainer without a test phase"""
        if self.eval_batch is None:
            raise ValueError(_NO_EVAL)

    @property
    def t_steps(self) -> int:
        return self.opt.t

    def params(self) -> Dict[str, torch.Tensor]:
        return self.opt.params()

    def host_params(self) -> Dict[str, np.ndarray]:
        return self.opt.host_params()


class _TrainF1:
    """macro_f1() and eval_macro_f1() of the trainers that keep the per-example tallies f1_tallies and eval_f1_tallies; where
    they were not asked for they are None, and _no_tallies / _no_eval_tallies say when they exist."""
    _no_eval_tallies = _NO_EVAL

    def macro_f1(self) -> float:
        """the train F1 of the last step (util.macroF1; one wait)"""
        if self.f1_tallies is None:
            raise ValueError(self._no_tallies)
        return macro_f1(self.f1_tallies)

    def eval_macro_f1(self) -> float:
        """the test F1 of the last evaluate() (util.macroF1; one wait)"""
        if self.eval_f1_tallies is None:
            raise ValueError(self._no_eval_tallies)
        return macro_f1(self.eval_f1_tallies)


# --------------------------------------------------------------------------------------------- #
# The flat-vector trainers
# --------------------------------------------------------------------------------------------- #
class FlatTrainer:
    """The scaffold of a trainer whose C entries take (descriptor, stream): `lib`, `device`, the descriptor `_args`, Adam's
    state in dicts `m` and `v` of flat tensors and the device step counts `step_count`."""

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, args=None):
        _lib.check(getattr(self.lib, name)(C.byref(self._args if args is None else args), self._stream()), name)

    def _work_offsets(self, entry, names, *dims) -> Dict[str, int]:
        """{piece: offset in floats} of a workspace from its icnn_be_*_work_offsets entry"""
        off = (C.c_longlong * len(names))()
        _lib.check(getattr(self.lib, entry)(*dims, C.byref(off)), entry)
        return dict(zip(names, (int(x) for x in off)))

    def _reset_adam(self):
        """Adam's moments and every step count back to zero"""
        for t in (*self.m.values(), *self.v.values(), self.step_count):
            t.zero_()


class ReplayTrainer(FlatTrainer):
    """What DDPGTrainer and NAFTrainer share: the minibatch buffers, named and typed as rl_train.CriticTrainer's so that
    rl_agent.ReplayMemory.sample_into fills them, and a step in three parts behind the entries `_entry` + chain / grads / update
    / step / act.  The class sets `_entry`, `spec` (dimO, dimA, l1, l2), `batch` and `theta`."""

    def _dims(self):
        s = self.spec
        return (s.dimO, s.dimA, s.l1, s.l2)

    def _minibatch_buffers(self):
        B, f32, dev = self.batch, torch.float32, self.device
        self.obs = torch.zeros(B, self.spec.dimO, dtype=f32, device=dev)
        self.ob2 = torch.zeros_like(self.obs)
        self.act = torch.zeros(B, self.spec.dimA, dtype=torch.float64, device=dev)
        self.rew = torch.zeros(B, dtype=f32, device=dev)
        self.term = torch.zeros(B, dtype=torch.uint8, device=dev)

    # ---- the step and its parts ----
    def chain(self):
        """the chain entry alone on the trainer's buffers: the per-sample part, into the workspace"""
        self._call(self._entry + "chain")

    def grads(self):
        """the grads entry alone: the flat gradients from the workspace the chain left"""
        self._call(self._entry + "grads")

    def update(self):
        """the update entry alone: the nets and targets from the flat gradients, and loss_q"""
        self._call(self._entry + "update")

    def step_buffers(self) -> torch.Tensor:
        """One step on what the trainer's obs / act / rew / ob2 / term hold.  Returns loss_q at the pre-update weights: the
        trainer's 0-d float32 device tensor, which the next step overwrites.  No host synchronisation."""
        self._call(self._entry + "step")
        return self.loss

    def step(self, obs, act, rew, ob2, term) -> torch.Tensor:
        """step_buffers() on the minibatch (obs [B, dimO], act [B, dimA], rew [B], ob2 [B, dimO], term [B] bool)"""
        for buf, value in ((self.obs, obs), (self.act, act), (self.rew, rew), (self.ob2, ob2), (self.term, term)):
            buf.copy_(torch.as_tensor(value).reshape(buf.shape))
        return self.step_buffers()

    def _act(self, which, obs, out) -> torch.Tensor:
        """the policy net theta[which] at obs [B', dimO] float32 on the device: float32 [B', dimA]; no host synchronisation"""
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.spec.dimO and obs.is_cuda
        if out is None:
            out = torch.empty(obs.shape[0], self.spec.dimA, dtype=torch.float32, device=self.device)
        entry = self._entry + "act"
        _lib.check(getattr(self.lib, entry)(*self._dims(), self.theta[which].data_ptr(), obs.data_ptr(), obs.shape[0],
                                            out.data_ptr(), self._stream()), entry)
        return out


class SupervisedTrainer(FlatTrainer, _Trainer):
    """What ff.FFTrainer and fcn.FCNTrainer share: model, Adam's state and the whole training step at one batch size behind
    the entries `_entry` + forward / backward / grads / update / step / eval, and the same buffers again for the test phase
    when eval_batch is given.  The class sets
        _entry, _key            the entry prefix ("icnn_be_ff_") and the key of the dicts theta, m, v ("ff")
        _work_names, _step_ints the _lib names of the workspace's pieces and the ints of step_count
        _fields                 the data fields of the args struct in order; the training buffers are attributes of these names
        _eval_fields            the attributes that hold the test phase's buffer of each field (the outputs, from the third on,
                                are None without a test phase)
        _extra                  the attributes copied into the args fields of their names (lr, pixel_scale): set before __init__
        _layout, _dims          the module's layout(spec) and _dims(spec)
    and _buffers(rows): zeroed tensors for `rows` samples, one per field."""

    def __init__(self, model, batch, eval_batch):
        self.batch, self.eval_batch = batch, eval_batch
        self.model, self.spec, self.device, self.lib = model, model.spec, model.device, model._lib
        n, dev, f32, k = model.n, self.device, torch.float32, self._key
        for name, buf in zip(self._fields, self._buffers(batch)):
            setattr(self, name, buf)
        # dicts of flat vectors, as the other flat trainers keep them (checkpoint.py)
        self.theta = {k: model.theta}
        self.m = {k: torch.zeros(n, dtype=f32, device=dev)}
        self.v = {k: torch.zeros(n, dtype=f32, device=dev)}
        self.grad = torch.zeros(n, dtype=f32, device=dev)
        self.step_count = torch.zeros(self._step_ints, dtype=torch.int32, device=dev)
        self.work = model.work(batch)
        self.work_offsets = self._offsets(batch)
        self._args = self._describe(batch, self.work, self._fields)
        for name in self._eval_fields[2:]:
            setattr(self, name, None)
        if eval_batch is not None:
            for name, buf in zip(self._eval_fields, self._buffers(eval_batch)):
                setattr(self, name, buf)
            self.eval_work = model.work(eval_batch)
            self._eval_args = self._describe(eval_batch, self.eval_work, self._eval_fields)

    def _offsets(self, batch):
        return self._work_offsets(self._entry + "work_offsets", self._work_names, batch, *self._dims(self.spec))

    def _describe(self, batch, work, names):
        """the args struct at one batch size: the data fields point at the attributes `names`"""
        a, k = self.model.args(batch, work), self._key
        for field, name in zip(self._fields, names):
            setattr(a, field, getattr(self, name).data_ptr())
        a.m, a.v, a.grad, a.step = self.m[k].data_ptr(), self.v[k].data_ptr(), self.grad.data_ptr(), self.step_count.data_ptr()
        for field in self._extra:
            setattr(a, field, getattr(self, field))
        return a

    # ---- the step and its parts ----
    def forward(self):
        """the forward entry alone on the trainer's buffers: the workspace, yhat, loss"""
        self._call(self._entry + "forward")

    def backward(self):
        self._call(self._entry + "backward")

    def grads(self):
        self._call(self._entry + "grads")

    def update(self):
        self._call(self._entry + "update")

    def step(self, x=None, target=None) -> torch.Tensor:
        """One step on (x, target), shaped as the first two buffers of _fields; None keeps what a buffer holds (graph
        replay).  Returns the loss at the weights the step began with."""
        self._put(getattr(self, self._fields[0]), x)
        self._put(getattr(self, self._fields[1]), target)
        self._call(self._entry + "step")
        return self.loss

    def evaluate(self, x=None, target=None) -> torch.Tensor:
        """The test phase on exactly eval_batch samples: eval_loss (returned) and the other outputs of _eval_fields.  Nothing
        of the model, the optimiser or the training step's results is written.  No host wait (capturable)."""
        self._require_eval()
        self._put(getattr(self, self._eval_fields[0]), x)
        self._put(getattr(self, self._eval_fields[1]), target)
        self._call(self._entry + "eval", self._eval_args)
        return self.eval_loss

    # ---- parameters ----
    @property
    def t_steps(self) -> int:
        """updates done (synchronises)"""
        return int(self.step_count[0].item())

    def params(self) -> Dict[str, torch.Tensor]:
        """live views of the variables inside theta"""
        return views(self._layout(self.spec), self.model.theta)

    def host_params(self) -> Dict[str, np.ndarray]:
        return self.model.host_params()

    def load(self, params, reset=True):
        """Copy a dict of named arrays (or a flat vector) into the existing theta.  reset: Adam's moments and the step count
        back to zero.  The moving statistics of a model that has them stay.  Synchronises."""
        self.model.load(params)
        if reset:
            self._reset_adam()
