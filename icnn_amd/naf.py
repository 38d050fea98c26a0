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

bn=True is naf_bn True (icnn_be_naf_bn_*, icnn_amd/csrc/be_naf_bn.hip): a BatchNorm with a trainable beta and
no gamma in front of the first layer and between each hidden product and its ReLU,
    h0 = BN0(o),  h1 = relu(BN1(h0 W1 + b1)),  h2 = relu(BN2(h1 W2 + b2)),  mlp(o) = h2 W3 + b3
The flat vector of a net then carries beta0 [dimO], beta1 [l1], beta2 [l2] behind b3; "target_v" holds W and b alone, the
target pass reads V's betas.  Every net has moving pairs of its own (mv["l" / "u" / "v"], MOVING's layout).  A step runs the
four passes on batch statistics, trains the betas with the same Adam (no decay, not in loss_q's sum of squares, not in the
target) and folds the statistics into the moving pairs, V's twice (obs, then ob2); policy() and q() choose bn="moving" or
"batch".
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


def layout(spec, which, bn=False):
    """[(name, shape)] of the variables of net "l", "u" or "v" in the order of the flat vector; bn: with the three betas"""
    if which not in TRAINED:
        raise ValueError("which must be 'l', 'u' or 'v', got %r" % (which,))
    o, l1, l2 = spec.dimO, spec.l1, spec.l2
    out = {"l": spec.dimA * spec.dimA, "u": spec.dimA, "v": 1}[which]
    betas = [("beta0", (o,)), ("beta1", (l1,)), ("beta2", (l2,))] if bn else []
    return [("W1", (o, l1)), ("b1", (l1,)), ("W2", (l1, l2)), ("b2", (l2,)), ("W3", (l2, out)), ("b3", (out,))] + betas


def moving_layout(spec):
    """[(name, shape)] of one net's moving pairs in the order of its flat vector mv[which]"""
    o, l1, l2 = spec.dimO, spec.l1, spec.l2
    return [("mean0", (o,)), ("var0", (o,)), ("mean1", (l1,)), ("var1", (l1,)), ("mean2", (l2,)), ("var2", (l2,))]


def n_floats(spec, which, bn=False) -> int:
    return _flat.n_floats(layout(spec, which, bn))


def flatten(spec, which, params, bn=False) -> np.ndarray:
    """the flat float32 vector of a dict of named arrays"""
    return _flat.flatten(layout(spec, which, bn), params, which + "/")


def unflatten(spec, which, flat, bn=False) -> Dict[str, np.ndarray]:
    return _flat.unflatten(layout(spec, which, bn), flat)


def init_moving(spec) -> Dict[str, np.ndarray]:
    """fresh moving pairs: means 0, variances 1"""
    return {name: (np.ones if name.startswith("var") else np.zeros)(shape, np.float32) for name, shape in moving_layout(spec)}


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
    gradients, update() moves the three nets and V's target.  bn=True (the module's docstring): the entries are
    icnn_be_naf_bn_*, the flat vectors carry the betas, mv["l" / "u" / "v"] are the moving pairs (host_moving, load_moving), and
    step_buffers() also folds the batch statistics into them; update() alone does not."""
    _entry = "icnn_be_naf_"

    def __init__(self, dimO, dimA, l1=200, l2=200, batch=256, rate=1e-3, tau=0.01, discount=0.99, l2norm=1e-4, seed=0,
                 device="cuda", eps=1e-4, beta1=0.9, beta2=0.999, initstd=0.01, bn=False, bn_eps=1e-3, bn_decay=0.999):
        self.spec = NAFSpec(int(dimO), int(dimA), int(l1), int(l2))
        self.batch = int(batch)
        self.bn = bool(bn)
        if self.batch < 1:
            raise ValueError("batch must be positive, got %r" % (batch,))
        if self.bn and self.batch > _lib.NAF_BN_MAX_BATCH:
            raise ValueError("bn: batch at most %d, got %r" % (_lib.NAF_BN_MAX_BATCH, batch))
        if not 0.0 <= tau <= 1.0:
            raise ValueError("tau must lie in [0, 1], got %r" % (tau,))
        self.lib = _lib.load()
        if self.bn:
            self._entry = "icnn_be_naf_bn_"
        work_bytes = getattr(self.lib, self._entry + "work_bytes")(self.batch, *self._dims())
        if work_bytes == 0:
            raise ValueError("sizes beyond what the NAF kernels support: %r" % (self.spec,))
        n = [C.c_longlong() for _ in range(5 if self.bn else 3)]
        _lib.check(getattr(self.lib, self._entry + "param_floats")(*self._dims(), *[C.byref(x) for x in n]),
                   self._entry + "param_floats")
        self.n = {w: int(x.value) for w, x in zip(TRAINED, n)}
        assert self.n == {w: n_floats(self.spec, w, self.bn) for w in TRAINED}
        self.rate, self.tau, self.discount, self.l2norm = float(rate), float(tau), float(discount), float(l2norm)
        self.device = dev = torch.device(device)
        B, f32 = self.batch, torch.float32
        self._minibatch_buffers()
        # separately allocated vectors: the policy launch reads theta["u"] as a net of its own
        self.theta = {w: torch.zeros(n_floats(self.spec, "v") if w == "target_v" else self.n[w], dtype=f32, device=dev)
                      for w in NETS}
        self.m = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in TRAINED}
        self.v = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in TRAINED}
        self.grad = {w: torch.zeros(self.n[w], dtype=f32, device=dev) for w in TRAINED}
        self.step_count = torch.zeros(_lib.NAF_STEP_INTS, dtype=torch.int32, device=dev)
        self.loss = torch.zeros((), dtype=f32, device=dev)
        self.work = torch.zeros(work_bytes // 4, dtype=f32, device=dev)
        self.work_offsets = self._work_offsets(self._entry + "work_offsets", _lib.NAF_BN_WORK if self.bn else _lib.NAF_WORK,
                                               B, *self._dims())
        a = _lib.NafBnArgs() if self.bn else _lib.NafArgs()
        if self.bn:
            assert (int(n[3].value), int(n[4].value)) == (self.theta["target_v"].numel(), _flat.n_floats(moving_layout(self.spec)))
            self.bn_eps, self.bn_decay = float(bn_eps), float(bn_decay)
            # the moving pairs: state of their own, neither trained nor reset with Adam
            self.mv = {w: torch.zeros(int(n[4].value), dtype=f32, device=dev) for w in TRAINED}
            self._fwd_work = None            # policy() and q(): their workspace, allocated at the first call
            for w in TRAINED:
                setattr(a, "mv_" + w, self.mv[w].data_ptr())
            a.bn_eps, a.bn_decay = self.bn_eps, self.bn_decay
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
        if self.bn:
            self.load_moving(**{w: init_moving(self.spec) for w in TRAINED})

    def work_view(self, name) -> torch.Tensor:
        """a live view of one piece of the workspace: [B, width] float32; "sq" float64 [tiles].  bn: the pieces of
        _lib.NAF_BN_WORK, a pass's letter ("l", "u", "v", "t" the target at ob2) last: h0 / h1 / h2 the sites' outputs, xh1 / xh2
        the normalised pre-activations, d1 / d2 / d3 the deltas, stat the pass's (mu, var) in moving_layout's order"""
        s, B = self.spec, self.batch
        a, aa = s.dimA, s.dimA * s.dimA
        if self.bn:
            at = self.work_offsets[name]
            if name == "sq":
                return self.work[at:at + 2 * ((B + 15) // 16)].view(torch.float64)
            if name.startswith("stat"):
                return self.work[at:at + _flat.n_floats(moving_layout(s))]
            head = {"y": 1, "u": a, "l": aa, "ld": a, "h": a, "adv": 1, "q": 1, "td": 1, "d3l": aa, "d3u": a, "d3v": 1}
            layer = {"h0": s.dimO, "h1": s.l1, "h2": s.l2, "xh1": s.l1, "xh2": s.l2, "d1": s.l1, "d2": s.l2}
            width = head[name] if name in head else layer[name[:-1]]
            return self.work[at:at + B * width].view(B, width)
        width = {"y": 1, "u": a, "l": aa, "ld": a, "h": a, "adv": 1, "q": 1, "td": 1, "h1l": s.l1, "h2l": s.l2, "h1u": s.l1,
                 "h2u": s.l2, "h1v": s.l1, "h2v": s.l2, "d3l": aa, "d2l": s.l2, "d1l": s.l1, "d3u": a, "d2u": s.l2, "d1u": s.l1,
                 "d3v": 1, "d2v": s.l2, "d1v": s.l1}
        at = self.work_offsets[name]
        if name == "sq":
            tiles = (B + 15) // 16
            return self.work[at:at + 2 * tiles].view(torch.float64)
        return self.work[at:at + B * width[name]].view(B, width[name])

    # ---- forward passes ----
    def _forward_work(self, rows) -> torch.Tensor:
        """the ONE workspace of policy() and q(), allocated at the first call for the largest batch they take (a piece's offset
        depends on the rows of the call alone, so it serves every smaller one) and kept: a captured graph holds its address"""
        if not 1 <= rows <= _lib.NAF_BN_MAX_BATCH:
            raise ValueError("bn: between 1 and %d rows, got %d" % (_lib.NAF_BN_MAX_BATCH, rows))
        if self._fwd_work is None:
            nbytes = self.lib.icnn_be_naf_bn_work_bytes(_lib.NAF_BN_MAX_BATCH, *self._dims())
            self._fwd_work = torch.zeros(nbytes // 4, dtype=torch.float32, device=self.device)
        return self._fwd_work

    def _bn_mode(self, bn) -> int:
        if not self.bn:
            if bn is not None:
                raise ValueError("bn=%r: this trainer has no BatchNorm (bn=False)" % (bn,))
            return -1
        if bn not in (None, "moving", "batch"):
            raise ValueError("bn must be 'moving' or 'batch', got %r" % (bn,))
        return _lib.BN_MODE[bn or "moving"]

    def policy(self, obs, out=None, bn=None) -> torch.Tensor:
        """u(obs) for obs [B', dimO] float32 on the device: float32 [B', dimA] (icnn_be_naf_act; no host synchronisation).
        bn (a trainer with bn=True only; elsewhere anything but None raises): "moving", the default there, normalises with U's
        moving pairs, as act() of the reference does (naf.py:118, is_training False); "batch" with the statistics of these
        rows.  At most _lib.NAF_BN_MAX_BATCH rows."""
        mode = self._bn_mode(bn)
        if not self.bn:
            return self._act("u", obs, out)
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.spec.dimO and obs.is_cuda
        if out is None:
            out = torch.empty(obs.shape[0], self.spec.dimA, dtype=torch.float32, device=self.device)
        work = self._forward_work(obs.shape[0])
        _lib.check(self.lib.icnn_be_naf_bn_act(*self._dims(), self.theta["u"].data_ptr(), self.mv["u"].data_ptr(), self.bn_eps,
                                               mode, obs.data_ptr(), obs.shape[0], out.data_ptr(), work.data_ptr(),
                                               self._stream()), "icnn_be_naf_bn_act")
        return out

    def q(self, obs, act, bn=None) -> torch.Tensor:
        """q(obs, act) for obs [B', dimO] float32 and act [B', dimA] float64 on the device: float32 [B'].  bn: as policy()"""
        mode = self._bn_mode(bn)
        assert obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] == self.spec.dimO
        assert act.dtype == torch.float64 and act.is_contiguous() and act.shape == (obs.shape[0], self.spec.dimA)
        out = torch.empty(obs.shape[0], dtype=torch.float32, device=self.device)
        if self.bn:
            work = self._forward_work(obs.shape[0])
            _lib.check(self.lib.icnn_be_naf_bn_q(*self._dims(), *[self.theta[w].data_ptr() for w in TRAINED],
                                                 *[self.mv[w].data_ptr() for w in TRAINED], self.bn_eps, mode,
                                                 obs.data_ptr(), act.data_ptr(), obs.shape[0], out.data_ptr(), work.data_ptr(),
                                                 self._stream()), "icnn_be_naf_bn_q")
            return out
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
        return unflatten(self.spec, which[-1], self.theta[which].cpu().numpy(), self.bn and which != "target_v")

    def host_moving(self, which) -> Dict[str, np.ndarray]:
        """the moving pairs of "l", "u" or "v" as a NumPy dict mean0, var0, .. (bn=True; synchronises)"""
        return _flat.unflatten(moving_layout(self.spec), self.mv[which].cpu().numpy())

    def load_moving(self, l=None, u=None, v=None):
        """Copy dicts mean0, var0, .. (or flat vectors) into the existing moving pairs (bn=True).  Synchronises."""
        for which, pairs in (("l", l), ("u", u), ("v", v)):
            if pairs is not None:
                _flat.copy_into(self.mv[which], moving_layout(self.spec), pairs, "mv/" + which, which + "/")

    def load(self, l=None, u=None, v=None, target_v=None, reset=True):
        """Copy dicts of named arrays (or flat vectors) into the existing tensors.  The target follows v when v is given and
        the target is not.  reset: Adam's moments and the step count back to zero.  Synchronises.  bn=True: a dict without
        betas gets zeros for them; the target takes W and b alone."""
        given = {"l": l, "u": u, "v": v, "target_v": target_v if target_v is not None else v}
        for which, params in given.items():
            if params is None:
                continue
            if not self.bn:
                _flat.copy_into(self.theta[which], layout(self.spec, which[-1]), params, which, which[-1] + "/")
                continue
            lay = layout(self.spec, which[-1], which != "target_v")
            if isinstance(params, dict):
                params = {name: params[name] if name in params or not name.startswith("beta") else np.zeros(shape, np.float32)
                          for name, shape in lay}
            elif which == "target_v" and target_v is None:
                params = np.asarray(params, np.float32)[:self.theta[which].numel()]
            _flat.copy_into(self.theta[which], lay, params, which, which[-1] + "/")
        if reset:
            self._reset_adam()
