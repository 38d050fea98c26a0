"""DDPG on the device: the networks of RL/src/ddpg_nets_dm.py and the training step of RL/src/ddpg.py around
icnn_be_ddpg_* (icnn_amd/csrc/be_ddpg.hip).

A net is one flat float32 vector in the order W1, b1, W2, b2, W3, b3, every W row-major [in][out]:
    policy  a = tanh(relu(relu(o W1 + b1) W2 + b2) W3 + b3)          W1 [dimO, l1], W2 [l1, l2], W3 [l2, dimA]
    critic  q = relu([relu(o W1 + b1), a] W2 + b2) W3 + b3           W1 [dimO, l1], W2 [l1 + dimA, l2], W3 [l2, 1]
One step, enqueued on the current stream without a host synchronisation (a captured step replayed k times is k steps):
    1. icnn_be_ddpg_chain   the per-sample part in one launch: target, critic, policy, critic at pi(obs), both backward chains
    2. icnn_be_ddpg_grads   the twelve weight and bias gradients in one launch (one fma chain over the batch per element)
    3. icnn_be_ddpg_update  decay, TF-Adam on both nets, the targets from the NEW weights, loss_q
"""
import ctypes as C
import dataclasses
from typing import Dict

import numpy as np
import torch

from . import _lib
from . import flat as _flat

NETS = ("q", "p", "target_q", "target_p")


@dataclasses.dataclass(frozen=True)
class DDPGSpec:
    dimO: int
    dimA: int
    l1: int
    l2: int


def layout(spec, which):
    """[(name, shape)] of the variables of the policy (which "p") or the critic ("q") in the order of the flat vector"""
    o, a, l1, l2 = spec.dimO, spec.dimA, spec.l1, spec.l2
    if which == "p":
        return [("W1", (o, l1)), ("b1", (l1,)), ("W2", (l1, l2)), ("b2", (l2,)), ("W3", (l2, a)), ("b3", (a,))]
    if which == "q":
        return [("W1", (o, l1)), ("b1", (l1,)), ("W2", (l1 + a, l2)), ("b2", (l2,)), ("W3", (l2, 1)), ("b3", (1,))]
    raise ValueError("which must be 'p' or 'q', got %r" % (which,))


def n_floats(spec, which) -> int:
    return _flat.n_floats(layout(spec, which))


def flatten(spec, which, params) -> np.ndarray:
    """the flat float32 vector of a dict of named arrays"""
    return _flat.flatten(layout(spec, which), params, which + "/")


def unflatten(spec, which, flat) -> Dict[str, np.ndarray]:
    return _flat.unflatten(layout(spec, which), flat)


def init_params(dimO, dimA, l1, l2, seed, final_p=3e-3, final_q=3e-4):
    """ddpg_nets_dm.py:8-45 with NumPy's stream: {"p": {name: array}, "q": {name: array}}, float32.  Layers 1 and 2 uniform
    +-1/sqrt(fan-in), a bias with the fan-in of its weight; the last layer uniform +-final_p (policy) / +-final_q (critic), or
    +-1/sqrt(fan-in) where that is None.  Drawn in the order of the flat vectors, the policy first."""
    spec = DDPGSpec(int(dimO), int(dimA), int(l1), int(l2))
    rng = np.random.RandomState(seed)
    out = {}
    for which, final in (("p", final_p), ("q", final_q)):
        net, bound = {}, None
        for name, shape in layout(spec, which):
            if name.startswith("W"):
                bound = 1.0 / np.sqrt(shape[0])
                if name == "W3" and final is not None:
                    bound = float(final)
            net[name] = rng.uniform(-bound, bound, shape).astype(np.float32)
        out[which] = net
    return out


class DDPGTrainer(_flat.ReplayTrainer):
    """Both nets, both targets, Adam's state and the whole training step at one minibatch size.  obs / act (float64) / rew /
    ob2 / term are named and typed as rl_train.CriticTrainer's, so rl_agent.ReplayMemory.sample_into fills them.  The nets
    start from init_params(seed) with the targets as copies.  grad_q / grad_p hold the last step's gradients (before the decay
    term), work_view(name) the pieces of the chain's workspace (_lib.DDPG_WORK).  chain() is icnn_be_ddpg_chain, grads() leaves
    grad_q and grad_p, update() moves both nets and both targets."""
    _entry = "icnn_be_ddpg_"

    def __init__(self, dimO, dimA, l1=200, l2=200, batch=256, rate=1e-3, prate=1e-4, tau=0.01, discount=0.99, l2norm=1e-4,
                 pl2norm=0.0, seed=0, device="cuda", eps=1e-4, beta1=0.9, beta2=0.999):
        self.spec = DDPGSpec(int(dimO), int(dimA), int(l1), int(l2))
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("batch must be positive, got %r" % (batch,))
        if not 0.0 <= tau <= 1.0:
            raise ValueError("tau must lie in [0, 1], got %r" % (tau,))
        self.lib = _lib.load()
        np_, nq = C.c_longlong(), C.c_longlong()
        _lib.check(self.lib.icnn_be_ddpg_param_floats(*self._dims(), C.byref(np_), C.byref(nq)), "icnn_be_ddpg_param_floats")
        self.n = {"p": int(np_.value), "q": int(nq.value)}
        assert self.n == {w: n_floats(self.spec, w) for w in "pq"}
        self.rate, self.prate, self.tau, self.discount = float(rate), float(prate), float(tau), float(discount)
        self.l2norm, self.pl2norm = float(l2norm), float(pl2norm)
        self.device = dev = torch.device(device)
        B, f32 = self.batch, torch.float32
        self._minibatch_buffers()
        self.theta = {w: torch.zeros(self.n[w[-1]], dtype=f32, device=dev) for w in NETS}
        self.m = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in "pq"}
        self.v = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in "pq"}
        self.grad_q = torch.zeros(self.n["q"], dtype=f32, device=dev)
        self.grad_p = torch.zeros(self.n["p"], dtype=f32, device=dev)
        self.step_count = torch.zeros(_lib.DDPG_STEP_INTS, dtype=torch.int32, device=dev)
        self.loss = torch.zeros((), dtype=f32, device=dev)
        work_bytes = self.lib.icnn_be_ddpg_work_bytes(B, *self._dims())
        if work_bytes == 0:
            raise ValueError("sizes beyond what the DDPG kernels support: %r" % (self.spec,))
        self.work = torch.zeros(work_bytes // 4, dtype=f32, device=dev)
        self.work_offsets = self._work_offsets("icnn_be_ddpg_work_offsets", _lib.DDPG_WORK, B, *self._dims())
        a = _lib.DdpgArgs()
        a.batch, a.dimO, a.dimA, a.l1, a.l2 = (B,) + self._dims()
        a.obs, a.act, a.rew, a.ob2, a.term = (t.data_ptr() for t in (self.obs, self.act, self.rew, self.ob2, self.term))
        a.theta_q, a.theta_p = self.theta["q"].data_ptr(), self.theta["p"].data_ptr()
        a.target_q, a.target_p = self.theta["target_q"].data_ptr(), self.theta["target_p"].data_ptr()
        a.m_q, a.v_q, a.m_p, a.v_p = (t.data_ptr() for t in (self.m["q"], self.v["q"], self.m["p"], self.v["p"]))
        a.grad_q, a.grad_p = self.grad_q.data_ptr(), self.grad_p.data_ptr()
        a.step, a.loss, a.work = self.step_count.data_ptr(), self.loss.data_ptr(), self.work.data_ptr()
        a.rate, a.prate, a.beta1, a.beta2 = self.rate, self.prate, float(beta1), float(beta2)
        a.eps, a.tau, a.discount, a.l2norm, a.pl2norm = float(eps), self.tau, self.discount, self.l2norm, self.pl2norm
        self._args = a
        params = init_params(*self._dims(), seed=seed)
        self.load(p=params["p"], q=params["q"])

    def work_view(self, name) -> torch.Tensor:
        """a live view of one piece of the workspace: [B, width] float32; "sq" float64 [tiles]"""
        s, B = self.spec, self.batch
        width = {"a2": s.dimA, "y": 1, "q": 1, "td": 1, "a": s.dimA, "qpi": 1, "xa": s.l1 + s.dimA, "h2q": s.l2, "d3q": 1,
                 "d2q": s.l2, "d1q": s.l1, "h1p": s.l1, "h2p": s.l2, "h2c": s.l2, "d3p": s.dimA, "d2p": s.l2, "d1p": s.l1}
        at = self.work_offsets[name]
        if name == "sq":
            tiles = (B + 15) // 16
            return self.work[at:at + 2 * tiles].view(torch.float64)
        return self.work[at:at + B * width[name]].view(B, width[name])

    # ---- forward passes ----
    def policy(self, obs, out=None, which="p") -> torch.Tensor:
        """pi(obs) for obs [B', dimO] float32 on the device: float32 [B', dimA] (icnn_be_ddpg_act; no host synchronisation)"""
        return self._act(which, obs, out)

    def q(self, obs, act, which="q") -> torch.Tensor:
        """Q(obs, act) for obs [B', dimO] float32 and act [B', dimA] float64 on the device: float32 [B']"""
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.spec.dimO
        assert act.dtype == torch.float64 and act.is_contiguous() and act.shape == (obs.shape[0], self.spec.dimA)
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.icnn_be_ddpg_q(*self._dims(), self.theta[which].data_ptr(), obs.data_ptr(), act.data_ptr(),
                                           obs.shape[0], out.data_ptr(), self._stream()), "icnn_be_ddpg_q")
        return out

    # ---- parameters ----
    @property
    def t(self):
        """updates done: (the critic's, the policy's) (synchronises)"""
        c = self.step_count.cpu().numpy()
        return int(c[0]), int(c[1])

    def host_params(self, which) -> Dict[str, np.ndarray]:
        """the variables of "q", "p", "target_q" or "target_p" as a NumPy dict (synchronises)"""
        return unflatten(self.spec, which[-1], self.theta[which].cpu().numpy())

    def load(self, p=None, q=None, target_p=None, target_q=None, reset=True):
        """Copy dicts of named arrays (or flat vectors) into the existing tensors.  A target that is not given follows its net
        when that net is given.  reset: Adam's moments and both step counts back to zero.  Synchronises."""
        given = {"p": p, "q": q, "target_p": target_p if target_p is not None else p,
                 "target_q": target_q if target_q is not None else q}
        for which, params in given.items():
            if params is not None:
                _flat.copy_into(self.theta[which], layout(self.spec, which[-1]), params, which, which[-1] + "/")
        if reset:
            self._reset_adam()
