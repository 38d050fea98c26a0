"""The RL agent's critic training step on the device: `Agent.train()` of RL/src/icnn.py:304-323 (graph :56-112) with
FLAGS.icnn_opt == 'adam'  or 'bundle_entropy' (DESIGN.md §28).

One step, enqueued on the current stream without a host synchronisation (a captured step replayed k times is k steps):
    1. target context of ob2 with the moving BatchNorm statistics (tflearn.is_training(False), :316)
    2. act2 = the inner Adam on the target (rl_adam.AdamSolver, be_adam.hip)
    3. the target value at (ob2, act2): the Adam kernel's f_best without BatchNorm; with BatchNorm a fresh evaluation with
       the batch statistics of ob2, which folds them once into the target's moving statistics
    4. the critic's context of obs (batch statistics, folded once into the critic's moving statistics) and negQ at act
    5. icnn_be_rl_td: TD target, c_j, the loss (be_rl_train.hip)
    6. the critic's gradient of sum_j c_j negQ_j (train.surrogate_grad, one row per sample)
    7. icnn_be_rl_critic_update: soft target update, L2 decay, TF-Adam, proj, both arenas (be_train_update.hip)

opt="bundle_entropy" replaces 2-3: act2 = 2y* - 1 of the bundle-entropy solve on the target's boxed() view and negQ_target(ob2,
act2) out of the same launch (rl_bundle.BundleActionSolver); icnn_be_rl_td then adds the entropy of act2 (:455-458).  With
BatchNorm the value is evaluated afresh with the batch statistics of ob2, as in 3.
"""
import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import _lib, picnn, rl_adam, rl_bundle, train
from .flat import _positive

OPTS = ("adam", "bundle_entropy")        # FLAGS.icnn_opt (RL/src/icnn.py:39-44)


def decay_mask(spec) -> np.ndarray:
    """uint8 [n] over the flat theta (grad_layout order): 1 on the W of every fully connected layer -- the variables that
    tflearn's fully_connected(weight_decay=...) puts under the L2 regulariser -- and 0 on biases and BatchNorm gamma / beta."""
    parts = [np.full(int(np.prod(shape)), 1 if name.endswith("/W") else 0, np.uint8) for name, shape in train.grad_layout(spec)]
    return np.concatenate(parts)


def _same_map(a: train.ParamMap, b: train.ParamMap) -> bool:
    return (a.n == b.n and a.arena_floats == b.arena_floats and list(a.offsets) == list(b.offsets) and a.proj == b.proj
            and np.array_equal(a.dest_off, b.dest_off) and np.array_equal(a.dest, b.dest))


class CriticTrainer:
    """The critic's whole training step at one minibatch size.  Constructing one ATTACHES both models: the critic to a
    train.DeviceAdam (its Adam state and arena), the target to a train.FollowerWeights (an arena of its own), so that the
    descriptors of both stay fixed and a captured step keeps reading the current weights of each.  `critic` and `target`
    are picnn.FCModel of one spec with action_box False (the adam branch optimises the action itself; the bundle-entropy
    branch solves on target.boxed() and leaves the stored actions and the gradient on the plain view).
    opt: the inner optimiser of step 2, "adam" (max_iter) or "bundle_entropy" (n_iter, the reference's nIter = 5).

    wd: the weight decay of tflearn's fully_connected (its default 0.001, taken from tflearn's source); the loss carries
    l2norm * sum_W wd |W|^2 / 2 (RL/src/icnn.py:90-93)."""

    def __init__(self, critic, target, batch, lr=1e-3, tau=0.01, discount=0.99, l2norm=1e-4, wd=1e-3, max_iter=1000,
                 opt="adam", n_iter=5):
        if opt not in OPTS:
            raise RuntimeError("Unrecognized ICNN optimizer: " + str(opt))      # RL/src/icnn.py:44
        if opt == "bundle_entropy" and not 1 <= int(n_iter) <= _lib.MAX_ITERS:
            raise ValueError("n_iter must be in 1..%d, got %r" % (_lib.MAX_ITERS, n_iter))
        if critic.spec != target.spec:
            raise ValueError("the critic and the target must share one spec")
        if critic.spec.action_box:
            raise ValueError("build the models with action_box=False: the adam branch takes the action as is, the "
                             "bundle_entropy branch boxes the target itself")
        if not 0.0 <= tau <= 1.0:
            raise ValueError("tau must lie in [0, 1], got %r" % (tau,))
        self.critic, self.target, self.spec, self.device = critic, target, critic.spec, critic.device
        self.batch = _positive("batch", batch)
        self.lr, self.tau, self.discount, self.l2norm, self.wd = float(lr), float(tau), float(discount), float(l2norm), float(wd)
        self.lib = _lib.load()
        self.opt = train.DeviceAdam(critic, lr)
        self.follower = train.FollowerWeights(target)
        if not _same_map(self.opt.map, self.follower.map):
            raise AssertionError("the critic's and the target's parameter maps differ")
        self.opt_name, self.n_iter = opt, int(n_iter)
        if opt == "adam":
            self.solver = rl_adam.AdamSolver(target, self.batch, max_iter)
        else:
            self.solver = rl_bundle.BundleActionSolver(target, self.batch, self.n_iter)
        dev, B, spec = self.device, self.batch, self.spec
        self.obs = torch.zeros(B, spec.n_features, dtype=torch.float32, device=dev)
        self.ob2 = torch.zeros_like(self.obs)
        self.act = torch.zeros(B, spec.n_labels, dtype=torch.float64, device=dev)
        self.rew = torch.zeros(B, dtype=torch.float32, device=dev)
        self.term = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.td = torch.zeros(B, dtype=torch.float32, device=dev)
        self.c = torch.zeros(B, dtype=torch.float64, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.work = torch.zeros(_lib.RL_TD_WORK_BYTES, dtype=torch.uint8, device=dev)
        self.decay = torch.from_numpy(decay_mask(spec)).to(dev)
        self.grad = None                     # the last step's gradient of sum_j c_j negQ_j (flat, before the decay term)
        self.act2 = None                     # the last step's target actions (float64 [B, n])
        self.q2_src = None                   # the last step's target value source (f_best, or negQ_target at act2)
        self.e_critic = None                 # the last step's negQ(obs, act)
        r = _lib.RlUpdateArgs()
        r.adam = self.opt._args
        r.target_theta, r.target_arena = self.follower.theta.data_ptr(), self.follower.arena.data_ptr()
        r.decay = self.decay.data_ptr()
        r.tau, r.l2norm, r.wd = self.tau, self.l2norm, self.wd
        self._args = r

    def initialise(self):
        """The reference's initialisation (:139-142): makeCvx on the critic, then target <- critic (trainable variables;
        the moving statistics stay as they are).  Synchronises."""
        params = picnn.make_convex(self.opt.host_params())
        self.opt.load(params)
        self.follower.load(params)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def td_loss(self, e_critic, q2_src, act2):
        """Step 5 alone on the trainer's buffers (obs, act, rew, term as the last step or the caller left them):
        icnn_be_rl_td into self.td, self.c, self.loss.  act2 None: q2_src already holds negQ_entr."""
        assert e_critic.dtype == torch.float32 and q2_src.dtype == torch.float32
        assert e_critic.is_contiguous() and q2_src.is_contiguous() and e_critic.shape == q2_src.shape == (self.batch,)
        if act2 is not None:
            assert act2.dtype == torch.float64 and act2.is_contiguous() and act2.shape == self.act.shape
        _lib.check(self.lib.icnn_be_rl_td(
            self.batch, self.spec.n_labels, e_critic.data_ptr(), self.act.data_ptr(), self.rew.data_ptr(), self.term.data_ptr(),
            q2_src.data_ptr(), None if act2 is None else act2.data_ptr(), self.discount, self.opt.theta.data_ptr(), self.opt.n,
            self.decay.data_ptr(), self.l2norm, self.wd, self.td.data_ptr(), self.c.data_ptr(), self.loss.data_ptr(),
            self.work.data_ptr(), self._stream()), "icnn_be_rl_td")

    def update(self, grad):
        """Step 7 alone: icnn_be_rl_critic_update with the flat float32 gradient `grad` (before the decay term)."""
        assert grad.dtype == torch.float32 and grad.shape == (self.opt.n,) and grad.is_contiguous() and grad.data_ptr() % 16 == 0
        self._args.adam.grad = grad.data_ptr()
        _lib.check(self.lib.icnn_be_rl_critic_update(C.byref(self._args), self._stream()), "icnn_be_rl_critic_update")
        self._keep = grad

    def step(self, obs, act, rew, ob2, term) -> torch.Tensor:
        """One training step on the minibatch (obs [B, dimO], act [B, dimA], rew [B], ob2 [B, dimO], term [B] bool).
        Returns the loss at the pre-update weights: the trainer's 0-d float32 device tensor, which the next step
        overwrites.  No host synchronisation."""
        self.obs.copy_(torch.as_tensor(obs).reshape(self.obs.shape))
        self.act.copy_(torch.as_tensor(act).reshape(self.act.shape))
        self.rew.copy_(torch.as_tensor(rew).reshape(self.rew.shape))
        self.ob2.copy_(torch.as_tensor(ob2).reshape(self.ob2.shape))
        self.term.copy_(torch.as_tensor(term).reshape(self.term.shape))
        return self.step_buffers()

    def step_buffers(self) -> torch.Tensor:
        """step() on what the trainer's own obs / act / rew / ob2 / term buffers hold, without the five copies: the minibatch
        was written there on the device (rl_agent.ReplayMemory.sample_into).  Same return value, no host synchronisation."""
        bn = self.spec.batchnorm
        # 1-3: the target
        ctx2 = self.target.context(self.ob2, bn="moving") if bn else self.target.context(self.ob2)
        res = self.solver.solve(ctx2)
        bundle = self.opt_name == "bundle_entropy"
        self.act2 = res.act if bundle else res.act_best
        if bn:
            e2, _ = self.target.fg(self.target.context(self.ob2, bn="batch", bn_updates=1), self.act2)
            self.q2_src, act2 = e2, self.act2
        elif bundle:                         # negQ_target(ob2, act2) from the solve's launch; the entropy is icnn_be_rl_td's
            self.q2_src, act2 = res.q, self.act2
        else:
            self.q2_src, act2 = res.f_best, None
        # 4: the critic's value at (obs, act)
        ctx = self.critic.context(self.obs, bn="batch", bn_updates=1) if bn else self.critic.context(self.obs)
        self.e_critic, _ = self.critic.fg(ctx, self.act)
        # 5-7
        self.td_loss(self.e_critic, self.q2_src, act2)
        self.grad = train.surrogate_grad(self.critic, self.obs, (self.act, self.c), flat=True)
        self.update(self.grad)
        return self.loss

    @property
    def t(self) -> int:
        """updates done (synchronises)"""
        return self.opt.t

    def params(self) -> Dict[str, torch.Tensor]:
        """the critic's weights: live device views"""
        return self.opt.params()

    def target_params(self) -> Dict[str, torch.Tensor]:
        """the target's weights: live device views"""
        return self.follower.params()

    def host_params(self, target=False) -> Dict[str, np.ndarray]:
        """the critic's (target=True: the target's) weights as a NumPy dict (synchronises)"""
        return (self.follower if target else self.opt).host_params()
