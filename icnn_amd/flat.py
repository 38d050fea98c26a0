"""What the flat-vector trainers share (ddpg.py, naf.py, ff.py, fcn.py; checkpoint.FLAT_TRAINERS): a net is ONE float32
vector, the variables of a layout [(name, shape)] end to end, each in C order; the kernels read that vector as it lies.  Every
layout stays with its module; here are the vector's arithmetic and the scaffold of a trainer around a C descriptor.
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
