"""NAF on the device: the networks of RL/src/naf_nets_dm.py and the training step of RL/src/naf.py with
naf_bn False, around icnn_be_naf_* (icnn_amd/csrc/be_naf.hip).

Three nets "l", "u", "v", each one flat float32 vector in the order W1, b1, W2, b2, W3, b3, every W row-major [in][out], with
W1 [dimO, l1], W2 [l1, l2] and W3 [l2, dimA^2] (l), [l2, dimA] (u), [l2, 1] (v);  mlp(o) = relu(relu(o W1 + b1) W2 + b2) W3 + b3:
    l = mlp_l(obs) as a row-major [dimA, dimA] matrix; Lm its lower triangle with exp on the diagonal
    u = tanh(mlp_u(obs)),  h = (act - u) Lm,  A = -1/2 |h|^2,  q = mlp_v(obs) + A
"target_v" is V's target net; the target's advantage is the constant 0.  One step, enqueued on the current stream without a
host synchronisation (a captured step replayed k times is k steps):
    1. icnn_be_naf_chain   the per-sample part in one launch: target, the three forwards, the head, the backward chains
    2. icnn_be_naf_grads   the eighteen weight and bias gradients in one launch (one fma chain over the batch per element)
    3. icnn_be_naf_update  decay, ONE TF-Adam over the three nets, V's target from the NEW weights, loss_q
"""
import ctypes as C
import dataclasses
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import flat as _flat

NETS = ("l", "u", "v", "target_v")
TRAINED = ("l", "u", "v")


@dataclasses.dataclass(frozen=True)
class NAFSpec:
    dimO: int
    dimA: int
    l1: int
    l2: int


def layout(spec, which):
    """[(name, shape)] of the variables of net "l", "u" or "v" in the order of the flat vector"""
    if which not in TRAINED:
        raise ValueError("which must be 'l', 'u' or 'v', got %r" % (which,))
    o, l1, l2 = spec.dimO, spec.l1, spec.l2
    out = {"l": spec.dimA * spec.dimA, "u": spec.dimA, "v": 1}[which]
    return [("W1", (o, l1)), ("b1", (l1,)), ("W2", (l1, l2)), ("b2", (l2,)), ("W3", (l2, out)), ("b3", (out,))]


def n_floats(spec, which) -> int:
    return _flat.n_floats(layout(spec, which))


def flatten(spec, which, params) -> np.ndarray:
    """the flat float32 vector of a dict of named arrays"""
    return _flat.flatten(layout(spec, which), params, which + "/")


def unflatten(spec, which, flat) -> Dict[str, np.ndarray]:
    return _flat.unflatten(layout(spec, which), flat)


def init_params(dimO, dimA, l1, l2, seed, initstd=0.01):
    """naf_nets_dm.py:7-15 with NumPy's stream: {"l": {name: array}, "u": ..., "v": ..., "target_v": a copy of "v"}, float32.
    Every W a normal of std initstd cut at two standard deviations (a draw beyond is drawn again), every bias 0.  Drawn in
    the order of the flat vectors, l, u, v."""
    spec = NAFSpec(int(dimO), int(dimA), int(l1), int(l2))
    rng = np.random.RandomState(seed)
    out = {}
    for which in TRAINED:
        net = {}
        for name, shape in layout(spec, which):
            if name.startswith("W"):
                w = rng.standard_normal(shape)
                beyond = np.abs(w) > 2.0
                while beyond.any():
                    w[beyond] = rng.standard_normal(int(beyond.sum()))
                    beyond = np.abs(w) > 2.0
                net[name] = (initstd * w).astype(np.float32)
            else:
                net[name] = np.zeros(shape, np.float32)
        out[which] = net
    out["target_v"] = {k: v.copy() for k, v in out["v"].items()}
    return out


class NAFTrainer(_flat.ReplayTrainer):
    """The three nets, V's target, Adam's state and the whole training step at one minibatch size.  obs / act (float64) / rew
    / ob2 / term are named and typed as rl_train.CriticTrainer's, so rl_agent.ReplayMemory.sample_into fills them.  The nets
    start from init_params(seed).  grad["l" / "u" / "v"] hold the last step's gradients (before the decay term),
    work_view(name) the pieces of the chain's workspace (_lib.NAF_WORK).  chain() is icnn_be_naf_chain, grads() leaves the three
    gradients, update() moves the three nets and V's target."""
    _entry = "icnn_be_naf_"

    def __init__(self, dimO, dimA, l1=200, l2=200, batch=256, rate=1e-3, tau=0.01, discount=0.99, l2norm=1e-4, seed=0,
                 device="cuda", eps=1e-4, beta1=0.9, beta2=0.999, initstd=0.01):
        self.spec = NAFSpec(int(dimO), int(dimA), int(l1), int(l2))
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be positive, got %r" % (batch,))
        if not 0.0 <= tau <= 1.0:
            raise ValueError("tau must lie in [0, 1], got %r" % (tau,))
        self.lib = _lib.load()
        work_bytes = self.lib.icnn_be_naf_work_bytes(self.batch, *self._dims())
        if work_bytes == 0:
            raise ValueError("sizes beyond what the NAF kernels support: %r" % (self.spec,))
        n = [C.c_longlong() for _ in TRAINED]
        _lib.check(self.lib.icnn_be_naf_param_floats(*self._dims(), *[C.byref(x) for x in n]), "icnn_be_naf_param_floats")
        self.n = {w: int(x.value) for w, x in zip(TRAINED, n)}
        assert self.n == {w: n_floats(self.spec, w) for w in TRAINED}
        self.rate, self.tau, self.discount, self.l2norm = float(rate), float(tau), float(discount), float(l2norm)
        self.device = dev = torch.device(device)
        B, f32 = self.batch, torch.float32
        self._minibatch_buffers()
        # separately allocated vectors: the policy launch reads theta["u"] as a net of its own
        self.theta = {w: torch.zeros(self.n[w[-1]], dtype=f32, device=dev) for w in NETS}
        self.m = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in TRAINED}
        self.v = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in TRAINED}
        self.grad = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in TRAINED}
        self.step_count = torch.zeros(_lib.NAF_STEP_INTS, dtype=torch.int32, device=dev)
        self.loss = torch.zeros((), dtype=f32, device=dev)
        self.work = torch.zeros(work_bytes // 4, dtype=f32, device=dev)
        self.work_offsets = self._work_offsets("icnn_be_naf_work_offsets", _lib.NAF_WORK, B, *self._dims())
        a = _lib.NafArgs()
        a.batch, a.dimO, a.dimA, a.l1, a.l2 = (B,) + self._dims()
        a.obs, a.act, a.rew, a.ob2, a.term = (t.data_ptr() for t in (self.obs, self.act, self.rew, self.ob2, self.term))
        for w in TRAINED:
            setattr(a, "theta_" + w, self.theta[w].data_ptr())
            setattr(a, "m_" + w, self.m[w].data_ptr())
            setattr(a, "v_" + w, self.v[w].data_ptr())
            setattr(a, "grad_" + w, self.grad[w].data_ptr())
        a.target_v = self.theta["target_v"].data_ptr()
        a.step, a.loss, a.work = self.step_count.data_ptr(), self.loss.data_ptr(), self.work.data_ptr()
        a.rate, a.beta1, a.beta2 = self.rate, float(beta1), float(beta2)
        a.eps, a.tau, a.discount, a.l2norm = float(eps), self.tau, self.discount, self.l2norm
        self._args = a
        self.load(**init_params(*self._dims(), seed=seed, initstd=initstd))

    def work_view(self, name) -> torch.Tensor:
        """a live view of one piece of the workspace: [B, width] float32; "sq" float64 [tiles]"""
        s, B = self.spec, self.batch
        a, aa = s.dimA, s.dimA * s.dimA
        width = {"y": 1, "u": a, "l": aa, "ld": a, "h": a, "adv": 1, "q": 1, "td": 1, "h1l": s.l1, "h2l": s.l2, "h1u": s.l1,
                 "h2u": s.l2, "h1v": s.l1, "h2v": s.l2, "d3l": aa, "d2l": s.l2, "d1l": s.l1, "d3u": a, "d2u": s.l2, "d1u": s.l1,
                 "d3v": 1, "d2v": s.l2, "d1v": s.l1}
        at = self.work_offsets[name]
        if name == "sq":
            tiles = (B + 15) // 16
            return self.work[at:at + 2 * tiles].view(torch.float64)
        return self.work[at:at + B * width[name]].view(B, width[name])

    # ---- forward passes ----
    def policy(self, obs, out=None) -> torch.Tensor:
        """u(obs) for obs [B', dimO] float32 on the device: float32 [B', dimA] (icnn_be_naf_act; no host synchronisation)"""
        return self._act("u", obs, out)

    def q(self, obs, act) -> torch.Tensor:
        """q(obs, act) for obs [B', dimO] float32 and act [B', dimA] float64 on the device: float32 [B']"""
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.spec.dimO
        assert act.dtype == torch.float64 and act.is_contiguous() and act.shape == (obs.shape[0], self.spec.dimA)
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.icnn_be_naf_q(*self._dims(), *[self.theta[w].data_ptr() for w in TRAINED], obs.data_ptr(),
                                          act.data_ptr(), obs.shape[0], out.data_ptr(), self._stream()), "icnn_be_naf_q")
        return out

    # ---- parameters ----
    @property
    def t(self) -> int:
        """updates done (synchronises): one count, because one optimizer serves the three nets"""
        return int(self.step_count[0].item())

    def host_params(self, which) -> Dict[str, np.ndarray]:
        """the variables of "l", "u", "v" or "target_v" as a NumPy dict (synchronises)"""
        return unflatten(self.spec, which[-1], self.theta[which].cpu().numpy())

    def load(self, l=None, u=None, v=None, target_v=None, reset=True):
        """Copy dicts of named arrays (or flat vectors) into the existing tensors.  The target follows v when v is given and
        the target is not.  reset: Adam's moments and the step count back to zero.  Synchronises."""
        given = {"l": l, "u": u, "v": v, "target_v": target_v if target_v is not None else v}
        for which, params in given.items():
            if params is not None:
                _flat.copy_into(self.theta[which], layout(self.spec, which[-1]), params, which, which[-1] + "/")
        if reset:
            self._reset_adam()
