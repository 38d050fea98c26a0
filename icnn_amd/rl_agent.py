"""The RL agent on the device: the replay memory of RL/src/replay_memory.py and the reset / act / observe /
train cycle of RL/src/icnn.py:260-323 with either FLAGS.icnn_opt, around rl_train.CriticTrainer and rl_adam.AdamSolver /
rl_bundle.BundleActionSolver.

The memory's arrays, its cursor, its fill and the draw counter of the sampler live in device memory
(icnn_amd/csrc/be_rl_replay.hip): a training iteration is [icnn_be_replay_sample into the trainer's buffers,
CriticTrainer.step_buffers()] with no host data in it, so `iters` of them can be captured once and replayed on every
environment step.  The one host wait per environment step is act()'s copy of the action to the environment.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, ddpg, naf, rl_adam, rl_bundle, rl_train


class ReplayMemory:
    """RL/src/replay_memory.py on the device.  enqueue() stages one transition through a pageable host row and one blocking
    copy, so the caller may reuse its arrays at once; sample() / sample_into() are one launch on the current stream without a
    host wait.  n and i are host mirrors of the device's fill and cursor (deterministic, never read back).  The sampler
    follows the reference's rule with its own random numbers: Philox4x32-10 keyed by `seed`, counter (draw, sample, attempt,
    0), at most _lib.REPLAY_MAX_ATTEMPTS attempts per sample -- raise_on_error() reports a sample that spent them."""

    def __init__(self, size, dimO, dimA, device="cuda", seed=0):
        self.size, self.dimO, self.dimA, self.seed = int(size), int(dimO), int(dimA), int(seed)
        if self.size < 3 or self.dimO < 1 or self.dimA < 1:
            raise ValueError("a replay memory needs size >= 3, dimO >= 1 and dimA >= 1")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        self.device = dev = torch.device(device)
        self.lib = _lib.load()
        self.observations = torch.zeros(self.size, self.dimO, dtype=torch.float32, device=dev)
        self.actions = torch.zeros(self.size, self.dimA, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(self.size, dtype=torch.float32, device=dev)
        self.terminals = torch.zeros(self.size, dtype=torch.uint8, device=dev)
        self.ctrl = torch.zeros(_lib.REPLAY_CTRL_INTS, dtype=torch.int32, device=dev)
        self._stage = torch.zeros(_lib.replay_stage_bytes(self.dimO, self.dimA), dtype=torch.uint8, device=dev)
        self._row = np.zeros(self._stage.numel(), np.uint8)          # pageable: the copy below returns once it is read
        a = 8 * self.dimA
        self._row_act, self._row_obs = self._row[:a].view(np.float64), self._row[a:a + 4 * self.dimO].view(np.float32)
        self._row_rew = self._row[a + 4 * self.dimO:a + 4 * self.dimO + 4].view(np.float32)
        self._row_term = self._row[a + 4 * self.dimO + 4:].view(np.uint32)
        m = _lib.Replay()
        m.size, m.dimO, m.dimA = self.size, self.dimO, self.dimA
        m.observations, m.actions = self.observations.data_ptr(), self.actions.data_ptr()
        m.rewards, m.terminals, m.ctrl = self.rewards.data_ptr(), self.terminals.data_ptr(), self.ctrl.data_ptr()
        self._c = m
        self._idx = {}                       # batch -> the int32 index buffer of sample_into (fixed: a captured graph writes it)
        self.n = self.i = 0

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self):
        """replay_memory.py:23-25, and the sampler back at draw 0 with a clear status word"""
        self.ctrl.zero_()
        self.n = self.i = 0

    def enqueue(self, obs, term, act, rew):
        """replay_memory.py:27-34 (argument order included).  Not capturable: a copy from the host."""
        self._row_obs[:] = np.asarray(obs, np.float32).reshape(self.dimO)
        self._row_act[:] = np.asarray(act, np.float64).reshape(self.dimA)
        self._row_rew[0] = rew
        self._row_term[0] = 1 if term else 0
        self._stage.copy_(torch.from_numpy(self._row))
        _lib.check(self.lib.icnn_be_replay_enqueue(C.byref(self._c), self._stage.data_ptr(), self._stream()),
                   "icnn_be_replay_enqueue")
        self.i = (self.i + 1) % self.size
        self.n = min(self.size - 1, self.n + 1)

    def _sample(self, batch, obs, act, rew, ob2, term, idx):
        _lib.check(self.lib.icnn_be_replay_sample(C.byref(self._c), self.n, batch, self.seed, obs.data_ptr(), act.data_ptr(),
                                                  rew.data_ptr(), ob2.data_ptr(), term.data_ptr(), idx.data_ptr(),
                                                  self._stream()), "icnn_be_replay_sample")

    def sample_into(self, trainer) -> torch.Tensor:
        """replay_memory.py:36-55 straight into a CriticTrainer's obs / act / rew / ob2 / term buffers; returns the sampled
        indices (int32 [B], a buffer of this memory that the next call at this batch size overwrites)."""
        if trainer.obs.shape[1] != self.dimO or trainer.act.shape[1] != self.dimA or trainer.device != self.device:
            raise ValueError("the trainer's shapes or device differ from the memory's")
        B = trainer.batch
        if B not in self._idx:
            self._idx[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._sample(B, trainer.obs, trainer.act, trainer.rew, trainer.ob2, trainer.term, self._idx[B])
        return self._idx[B]

    def sample(self, batch):
        """a minibatch as new tensors: (obs f32 [B, dimO], act f64 [B, dimA], rew f32 [B], ob2 f32 [B, dimO], term u8 [B],
        idx i32 [B])"""
        B, dev = int(batch), self.device
        out = (torch.empty(B, self.dimO, dtype=torch.float32, device=dev), torch.empty(B, self.dimA, dtype=torch.float64, device=dev),
               torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, self.dimO, dtype=torch.float32, device=dev),
               torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        self._sample(B, *out)
        return out

    @property
    def status(self) -> int:
        """the device's status word, an OR of _lib.REPLAY_ST_* (synchronises)"""
        return int(self.ctrl[3].item())

    def raise_on_error(self):
        """Raise if a launch so far met an error on the device (synchronises): a sample that found no valid index within the
        attempt bound, or a control block outside the arrays."""
        st = self.status
        if st & _lib.REPLAY_ST_EXHAUSTED:
            raise RuntimeError("replay memory: a sample found no valid index in %d attempts (nearly every slot below n - 1 "
                               "is terminal or the cursor's); its last candidate was used" % _lib.REPLAY_MAX_ATTEMPTS)
        if st:
            raise RuntimeError("replay memory: the device control block was outside the arrays (status %d)" % st)


class VecReplayMemory:
    """The replay memory of `n_envs` environments that step in lockstep (icnn_be_vec_replay): `steps` time rows of
    n_envs transitions, so each of the n_envs columns is RL/src/replay_memory.py's memory.  enqueue() takes DEVICE tensors --
    one launch, no host data, capturable; n and i are host mirrors of the fill and the cursor, which count time rows.  The
    sampler draws a time row as ReplayMemory does and an environment with its own Philox domain tag; with n_envs = 1 it is
    ReplayMemory's, bit for bit."""

    def __init__(self, steps, n_envs, dimO, dimA, device="cuda", seed=0):
        self.steps, self.n_envs, self.dimO, self.dimA, self.seed = int(steps), int(n_envs), int(dimO), int(dimA), int(seed)
        if self.steps < 3 or self.n_envs < 1 or self.dimO < 1 or self.dimA < 1:
            raise ValueError("a vector replay memory needs steps >= 3, n_envs >= 1, dimO >= 1 and dimA >= 1")
        if self.steps * self.n_envs >= 1 << 31:
            raise ValueError("steps * n_envs must fit 31 bits")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        self.device = dev = torch.device(device)
        self.lib = _lib.load()
        T, E = self.steps, self.n_envs
        self.observations = torch.zeros(T, E, self.dimO, dtype=torch.float32, device=dev)
        self.actions = torch.zeros(T, E, self.dimA, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(T, E, dtype=torch.float32, device=dev)
        self.terminals = torch.zeros(T, E, dtype=torch.uint8, device=dev)
        self.ctrl = torch.zeros(_lib.REPLAY_CTRL_INTS, dtype=torch.int32, device=dev)
        m = _lib.VecReplay()
        m.steps, m.n_envs, m.dimO, m.dimA = T, E, self.dimO, self.dimA
        m.observations, m.actions = self.observations.data_ptr(), self.actions.data_ptr()
        m.rewards, m.terminals, m.ctrl = self.rewards.data_ptr(), self.terminals.data_ptr(), self.ctrl.data_ptr()
        self._c = m
        self._idx = {}
        self.n = self.i = 0

    @property
    def size(self) -> int:
        """time rows: what the cursor and the fill count (ReplayMemory.size for each column)"""
        return self.steps

    _stream = ReplayMemory._stream
    status = ReplayMemory.status
    raise_on_error = ReplayMemory.raise_on_error
    sample_into = ReplayMemory.sample_into
    sample = ReplayMemory.sample

    def reset(self):
        self.ctrl.zero_()
        self.n = self.i = 0

    def enqueue(self, obs, term, act, rew):
        """time row i of every environment from device tensors: obs float32 [E, dimO], term uint8 [E], act float64 [E, dimA],
        rew float32 [E] (ReplayMemory.enqueue's argument order).  They are read when the launch runs, not now."""
        E, dev = self.n_envs, self.ctrl.device
        for t, shape, dtype in ((obs, (E, self.dimO), torch.float32), (term, (E,), torch.uint8),
                                (act, (E, self.dimA), torch.float64), (rew, (E,), torch.float32)):
            if t.device != dev or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
                raise ValueError("enqueue takes contiguous device tensors: obs f32 [E, dimO], term u8 [E], act f64 [E, dimA], "
                                 "rew f32 [E]")
        _lib.check(self.lib.icnn_be_vec_replay_enqueue(C.byref(self._c), obs.data_ptr(), act.data_ptr(), rew.data_ptr(),
                                                       term.data_ptr(), self._stream()), "icnn_be_vec_replay_enqueue")
        self.i = (self.i + 1) % self.steps
        self.n = min(self.steps - 1, self.n + 1)

    def _sample(self, batch, obs, act, rew, ob2, term, idx):
        _lib.check(self.lib.icnn_be_vec_replay_sample(C.byref(self._c), self.n, batch, self.seed, obs.data_ptr(), act.data_ptr(),
                                                      rew.data_ptr(), ob2.data_ptr(), term.data_ptr(), idx.data_ptr(),
                                                      self._stream()), "icnn_be_vec_replay_sample")


class Explorer:
    """The Ornstein-Uhlenbeck exploration noise of `n_envs` environments on the device (icnn_be_explore):
    `noise` float64 [E, dimA], a step counter in device memory (a captured launch draws fresh numbers), and `action`, the
    clipped result, which stays on the device for VecReplayMemory.enqueue.  The normal deviates are the project's own stream
    (Philox4x32-10 keyed by `seed`, Box-Muller in float64), not np.random.randn's."""

    def __init__(self, n_envs, dimA, theta=0.15, sigma=0.1, device="cuda", seed=0):
        self.n_envs, self.dimA, self.theta, self.sigma, self.seed = int(n_envs), int(dimA), float(theta), float(sigma), int(seed)
        if self.n_envs < 1 or self.dimA < 1:
            raise ValueError("n_envs and dimA must be at least 1")
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        self.device = dev = torch.device(device)
        self.lib = _lib.load()
        self.noise = torch.zeros(self.n_envs, self.dimA, dtype=torch.float64, device=dev)
        self.action = torch.zeros(self.n_envs, self.dimA, dtype=torch.float64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)

    def reset(self, mask=None):
        """zero the noise rows where `mask` (bool [E], host or device) is set -- an environment that restarted --, or all rows"""
        if mask is None:
            self.noise.zero_()
        else:
            mask = torch.as_tensor(np.asarray(mask, bool) if not torch.is_tensor(mask) else mask).to(self.noise.device, torch.bool)
            if tuple(mask.shape) != (self.n_envs,):
                raise ValueError("mask is bool [n_envs]")
            self.noise.masked_fill_(mask[:, None], 0.0)

    def step(self, raw, test=False) -> torch.Tensor:
        """raw float64 or float32 [E, dimA] on the device -> self.action (float64 [E, dimA], clipped to [-1, 1]); one launch"""
        if raw.device != self.noise.device or tuple(raw.shape) != (self.n_envs, self.dimA) or not raw.is_contiguous() \
                or raw.dtype not in (torch.float64, torch.float32):
            raise ValueError("raw is a contiguous float64 or float32 device tensor [n_envs, dimA]")
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.icnn_be_explore(self.n_envs, self.dimA, raw.data_ptr(), int(raw.dtype == torch.float32),
                                            self.noise.data_ptr(), self.counter.data_ptr(), self.theta, self.sigma, self.seed,
                                            int(bool(test)), self.action.data_ptr(), stream), "icnn_be_explore")
        return self.action


class _AgentCycle:
    """What the agents share: the replay memory, the Ornstein-Uhlenbeck noise, observe() and the `iters` training iterations
    per observation, eager or captured.  A subclass builds self.trainer (obs / act / rew / ob2 / term buffers, step_buffers(),
    loss) and calls _setup().

    n_envs=E: E environments a step.  The observations [E, dimO], the noise [E, dimA] (Explorer) and the clipped
    action stay on the device; the memory is a VecReplayMemory of rmsize // E time rows.  A subclass's _raw_actions() returns the
    optimiser's or the policy's output for self._obs_dev; row e is what the single-environment agent computes for observation e.
    n_envs=None: the single-environment cycle, unchanged."""

    n_envs = None

    def _setup(self, dimO, dimA, device, warmup, iters, rmsize, outheta, ousigma, seed, capture, n_envs=None):
        self.dimO, self.dimA, self.device = int(dimO), int(dimA), device
        self.n_envs = None if n_envs is None else int(n_envs)
        if self.n_envs is None:
            self.memory = ReplayMemory(rmsize, self.dimO, self.dimA, self.device, seed)
        else:
            E = self.n_envs
            self.memory = VecReplayMemory(int(rmsize) // E, E, self.dimO, self.dimA, self.device, seed)
            self.explorer = Explorer(E, self.dimA, outheta, ousigma, self.device, seed)
            self._obs_dev = torch.zeros(E, self.dimO, dtype=torch.float32, device=self.device)
            # observe()'s packed block: obs2 float32 [E, dimO] | rew float32 [E] | term uint8 [E] -- one copy
            o, r = 4 * E * self.dimO, 4 * E
            self._stage = torch.zeros(o + r + E, dtype=torch.uint8, device=self.device)
            self._stage_obs = self._stage[:o].view(torch.float32).view(E, self.dimO)
            self._stage_rew, self._stage_term = self._stage[o:o + r].view(torch.float32), self._stage[o + r:]
            self._block = np.zeros(o + r + E, np.uint8)               # pageable: the copy returns once it is read
            self._block_obs = self._block[:o].view(np.float32).reshape(E, self.dimO)
            self._block_rew, self._block_term = self._block[o:o + r].view(np.float32), self._block[o + r:]
        self.warmup, self.iters, self.outheta, self.ousigma = int(warmup), int(iters), float(outheta), float(ousigma)
        self.rng = np.random.RandomState(seed)
        self.capture = bool(capture)
        self._graph, self._trained = None, False
        self.noise = np.zeros(self.dimA)
        self.observation = self.action = None
        self.t = 0                           # observations seen in training (icnn.py:146)

    @staticmethod
    def _check_cycle(warmup, iters, n_envs=None, rmsize=None):
        if warmup < 2:
            raise ValueError("warmup must be at least 2: the sampler needs two transitions, got %r" % (warmup,))
        if iters < 0:
            raise ValueError("iters must not be negative")
        if n_envs is not None:
            if int(n_envs) != n_envs or n_envs < 1:
                raise ValueError("n_envs must be a positive integer or None, got %r" % (n_envs,))
            if warmup < 2 * n_envs:
                raise ValueError("warmup must be at least 2 * n_envs: the sampler needs two time rows, got %r" % (warmup,))
            if rmsize // n_envs < 3:
                raise ValueError("rmsize // n_envs must be at least 3 time rows, got %r // %r" % (rmsize, n_envs))

    def reset(self, obs, mask=None):
        """icnn.py:260-262.  n_envs=E: obs [E, dimO] replaces the observation rows; the noise rows where `mask` (bool [E]) is
        set -- the environments that restarted -- are zeroed, or all rows without a mask."""
        if self.n_envs is not None:
            self.observation = np.array(obs, np.float32).reshape(self.n_envs, self.dimO)
            self._obs_dev.copy_(torch.from_numpy(self.observation))
            self.explorer.reset(mask)
            return
        if mask is not None:
            raise ValueError("mask: only with n_envs")
        self.noise = np.zeros(self.dimA)
        self.observation = obs

    def _act_vec(self, test):
        """the vector step of act(): the subclass's raw actions for self._obs_dev, one icnn_be_explore, one copy to the host"""
        self.action = self.explorer.step(self._raw_actions(), test).cpu().numpy()
        return self.action

    def _observe_vec(self, rew, term, obs2, test):
        E = self.n_envs
        self._block_obs[:] = np.asarray(obs2, np.float32).reshape(E, self.dimO)
        self._block_rew[:] = np.asarray(rew, np.float32).reshape(E)
        self._block_term[:] = np.asarray(term).reshape(E) != 0
        self.observation = self._block_obs.copy()
        self._stage.copy_(torch.from_numpy(self._block))
        if not test:
            self.t = self.t + E
            self.memory.enqueue(self._obs_dev, self._stage_term, self.explorer.action, self._stage_rew)
        self._obs_dev.copy_(self._stage_obs)
        if not test and self.t > self.warmup:
            self._train_iters()

    def _explore(self, action, test):
        """the raw action [1, dimA] (float64, host) plus the Ornstein-Uhlenbeck noise unless `test`, clipped to [-1, 1]"""
        if not test:
            self.noise -= self.outheta * self.noise - self.ousigma * self.rng.randn(self.dimA)
            action += self.noise
        action = np.clip(action, -1, 1)
        self.action = np.atleast_1d(np.squeeze(action, axis=0))
        return self.action

    def observe(self, rew, term, obs2, test=False):
        """icnn.py:290-302.  n_envs=E: rew [E], term [E], obs2 [E, dimO] go to the device as one block; one enqueue writes the
        time row from the observations and the action act() left there; t advances by E."""
        if self.n_envs is not None:
            return self._observe_vec(rew, term, obs2, test)
        obs1 = self.observation
        self.observation = obs2
        if not test:
            self.t = self.t + 1
            self.memory.enqueue(obs1, term, self.action, rew)
            if self.t > self.warmup:
                self._train_iters()

    def _train_iters(self):
        if self.iters == 0:
            return
        if not self.capture or not self._trained:
            for _ in range(self.iters):
                self.train()
            self._trained = True
            return
        if self._graph is None:
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                for _ in range(self.iters):
                    self.train()
        self._graph.replay()

    def train(self) -> torch.Tensor:
        """icnn.py:304-323: a minibatch from the memory into the trainer's buffers and one training step.  Returns the
        trainer's device loss scalar, without a host wait."""
        self.memory.sample_into(self.trainer)
        return self.trainer.step_buffers()

    @property
    def loss(self) -> torch.Tensor:
        """the last training iteration's loss (the trainer's 0-d device tensor)"""
        return self.trainer.loss


class Agent(_AgentCycle):
    """`Agent` of RL/src/icnn.py with either inner optimiser (opt = FLAGS.icnn_opt: "adam", or "bundle_entropy" at n_iter
    rounds; anything else raises the reference's RuntimeError): critic and target are picnn.FCModel of one spec
    with action_box False.  The constructor builds the CriticTrainer at minibatch size `bsize` (lr, tau, discount, l2norm, wd and
    max_iter go to it), initialises it as the reference does (:139-142: makeCvx, then target <- critic) and builds the
    ReplayMemory of `rmsize` transitions.  seed: the exploration noise's np.random.RandomState and the memory's sampler.

    capture=True: the first training observe() runs its `iters` iterations eagerly; the next one captures them once into a
    graph (a linear chain of [sample, step] x iters) and every later observe() replays it."""

    def __init__(self, critic, target, bsize=256, warmup=1000, iters=1, rmsize=500000, outheta=0.15, ousigma=0.1, seed=0,
                 capture=False, lr=1e-3, tau=0.01, discount=0.99, l2norm=1e-4, wd=1e-3, max_iter=1000, opt="adam", n_iter=5,
                 n_envs=None):
        if opt not in rl_train.OPTS:
            raise RuntimeError("Unrecognized ICNN optimizer: " + str(opt))      # RL/src/icnn.py:44
        self._check_cycle(warmup, iters, n_envs, rmsize)
        self.trainer = rl_train.CriticTrainer(critic, target, bsize, lr=lr, tau=tau, discount=discount, l2norm=l2norm, wd=wd,
                                              max_iter=max_iter, opt=opt, n_iter=n_iter)
        self.trainer.initialise()
        self.critic, self.spec, self.opt = critic, critic.spec, opt
        self._setup(self.spec.n_features, self.spec.n_labels, critic.device, warmup, iters, rmsize, outheta, ousigma, seed,
                    capture, n_envs)
        if opt == "adam":            # E environments: the stopping rule of every state on its own, so row e is the batch of one
            self._solver = (rl_adam.AdamSolver(critic, 1, max_iter) if n_envs is None else
                            rl_adam.AdamSolver(critic, n_envs, max_iter, stop="each"))
        else:
            self._solver = rl_bundle.BundleActionSolver(critic, n_envs or 1, n_iter)

    def _raw_actions(self):
        ctx = self.critic.context(self._obs_dev, bn="moving") if self.spec.batchnorm else self.critic.context(self._obs_dev)
        res = self._solver.solve(ctx.contiguous())
        return res.act_best if self.opt == "adam" else res.act

    def act(self, test=False):
        """icnn.py:264-288: the inner optimiser (Adam on negQ_entr, or the bundle-entropy solve on negQ: 2y* - 1) on the critic
        at the current observation (inference-mode BatchNorm), plus the Ornstein-Uhlenbeck noise unless `test`, clipped to
        [-1, 1].  Returns float64 [dimA] ([E, dimA] with n_envs=E); the copy to the host is the one synchronisation of an
        environment step."""
        if self.n_envs is not None:
            return self._act_vec(test)
        obs = torch.from_numpy(np.asarray(self.observation, np.float32).reshape(1, self.dimO))
        ctx = self.critic.context(obs, bn="moving") if self.spec.batchnorm else self.critic.context(obs)
        res = self._solver.solve(ctx)
        action = (res.act_best if self.opt == "adam" else res.act).cpu().numpy()
        return self._explore(action, test)


class DDPGAgent(_AgentCycle):
    """`Agent` of RL/src/ddpg.py around ddpg.DDPGTrainer: the same reset / act / observe / train cycle, memory,
    noise and capture as Agent; act() is one launch of the policy at the current observation (icnn_be_ddpg_act).  l1, l2,
    rate, prate, tau, discount, l2norm and pl2norm go to the trainer; seed also draws its initial weights."""

    def __init__(self, dimO, dimA, l1=200, l2=200, bsize=256, warmup=1000, iters=1, rmsize=500000, outheta=0.15, ousigma=0.1,
                 seed=0, capture=False, rate=1e-3, prate=1e-4, tau=0.01, discount=0.99, l2norm=1e-4, pl2norm=0.0,
                 device="cuda", n_envs=None):
        self._check_cycle(warmup, iters, n_envs, rmsize)
        self.trainer = ddpg.DDPGTrainer(dimO, dimA, l1, l2, batch=bsize, rate=rate, prate=prate, tau=tau, discount=discount,
                                        l2norm=l2norm, pl2norm=pl2norm, seed=seed, device=device)
        self.spec = self.trainer.spec
        self._setup(dimO, dimA, self.trainer.device, warmup, iters, rmsize, outheta, ousigma, seed, capture, n_envs)
        self._obs1 = torch.zeros(1, self.dimO, dtype=torch.float32, device=self.device)
        self._act1 = torch.zeros(n_envs or 1, self.dimA, dtype=torch.float32, device=self.device)

    def _raw_actions(self):
        return self.trainer.policy(self._obs_dev, out=self._act1)

    def act(self, test=False):
        """ddpg.py:129-134: pi(observation), plus the Ornstein-Uhlenbeck noise unless `test`, clipped to [-1, 1].  Returns
        float64 [dimA] ([E, dimA] with n_envs=E); the copy to the host is the one synchronisation of an environment step."""
        if self.n_envs is not None:
            return self._act_vec(test)
        self._obs1.copy_(torch.from_numpy(np.asarray(self.observation, np.float32).reshape(1, self.dimO)))
        action = self.trainer.policy(self._obs1, out=self._act1).cpu().numpy().astype(np.float64)
        return self._explore(action, test)


class NAFAgent(_AgentCycle):
    """`Agent` of RL/src/naf.py around naf.NAFTrainer: the same reset / act / observe / train cycle, memory,
    noise and capture as Agent; act() is one launch of the U net at the current observation (icnn_be_naf_act).  l1, l2, rate,
    tau, discount, l2norm and initstd go to the trainer; seed also draws its initial weights.  naf_bn: the networks with
    BatchNorm (agent.py:22); act() then normalises with U's moving pairs (naf.py:118)."""

    def __init__(self, dimO, dimA, l1=200, l2=200, bsize=256, warmup=1000, iters=1, rmsize=500000, outheta=0.15, ousigma=0.1,
                 seed=0, capture=False, rate=1e-3, tau=0.01, discount=0.99, l2norm=1e-4, initstd=0.01, device="cuda",
                 naf_bn=False, n_envs=None):
        self._check_cycle(warmup, iters, n_envs, rmsize)
        self.trainer = naf.NAFTrainer(dimO, dimA, l1, l2, batch=bsize, rate=rate, tau=tau, discount=discount, l2norm=l2norm,
                                      seed=seed, device=device, initstd=initstd, bn=naf_bn)
        self.spec = self.trainer.spec
        self._setup(dimO, dimA, self.trainer.device, warmup, iters, rmsize, outheta, ousigma, seed, capture, n_envs)
        self._obs1 = torch.zeros(1, self.dimO, dtype=torch.float32, device=self.device)
        self._act1 = torch.zeros(n_envs or 1, self.dimA, dtype=torch.float32, device=self.device)

    def _raw_actions(self):
        return self.trainer.policy(self._obs_dev, out=self._act1)

    def act(self, test=False):
        """naf.py:116-121: u(observation), plus the Ornstein-Uhlenbeck noise unless `test`, clipped to [-1, 1].  Returns
        float64 [dimA] ([E, dimA] with n_envs=E); the copy to the host is the one synchronisation of an environment step."""
        if self.n_envs is not None:
            return self._act_vec(test)
        self._obs1.copy_(torch.from_numpy(np.asarray(self.observation, np.float32).reshape(1, self.dimO)))
        action = self.trainer.policy(self._obs1, out=self._act1).cpu().numpy().astype(np.float64)
        return self._explore(action, test)
