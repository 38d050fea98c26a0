"""The agents at n_envs = E (rl_agent.Agent / DDPGAgent / NAFAgent): row e of act() is what the
single-environment agent computes for observation e, the cycle against a host composition of the restatements
(tests/vec_replay_ref.py) and an independent CriticTrainer, eager and captured, and checkpoints."""
import numpy as np
import pytest
import torch

import test_rl_agent as base
import vec_replay_ref as ref
from icnn_amd import checkpoint, rl_agent

DIMO, DIMA = 4, 2


def _spec():
    return base._critic_spec(dimO=DIMO, dimA=DIMA)


def _icnn(seed=9, **kw):
    args = dict(bsize=4, warmup=6, iters=2, rmsize=24, seed=seed, max_iter=50)
    args.update(kw)
    return rl_agent.Agent(*base._models(_spec(), 23), **args)


def _flat(cls, seed=9, **kw):
    args = dict(l1=16, l2=8, bsize=4, warmup=6, iters=2, rmsize=24, seed=seed)
    args.update(kw)
    return cls(DIMO, DIMA, **args)


def _world(steps, E, seed):
    """what E environments answer: obs2 [steps, E, dimO], rew [steps, E], term [steps, E] (some set), and the first observations"""
    rng = np.random.RandomState(seed)
    return (rng.randn(E, DIMO).astype(np.float32), rng.randn(steps, E, DIMO).astype(np.float32),
            rng.randn(steps, E).astype(np.float32), rng.rand(steps, E) < 0.25)


# ------------------------------------------------------------------------------------------------ CPU


def test_constructor_checks_come_before_the_device():
    for cls, args in ((rl_agent.Agent, (None, None)), (rl_agent.DDPGAgent, (DIMO, DIMA)), (rl_agent.NAFAgent, (DIMO, DIMA))):
        with pytest.raises(ValueError, match="warmup"):
            cls(*args, warmup=5, rmsize=24, n_envs=3)                    # two time rows are 6 transitions
        with pytest.raises(ValueError, match="rmsize"):
            cls(*args, warmup=6, rmsize=8, n_envs=3)                     # 8 // 3 = 2 time rows
        with pytest.raises(ValueError, match="n_envs"):
            cls(*args, warmup=6, rmsize=24, n_envs=0)


# ------------------------------------------------------------------------------------------------ GPU


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adam", "bundle_entropy"])
def test_one_environment_is_the_single_environment_agent(opt):
    obs = np.array([0.3, -0.2, 0.1, 0.05], np.float32)
    one, vec = _icnn(opt=opt, warmup=4, rmsize=8), _icnn(opt=opt, n_envs=1)
    one.reset(obs)
    vec.reset(obs[None])
    want, got = one.act(test=True), vec.act(test=True)
    assert got.shape == (1, DIMA) and got.dtype == np.float64 and np.array_equal(got[0], want) and np.any(want != 0)
    assert not vec.explorer.noise.any() and int(vec.explorer.counter.item()) == 0


def _pairs():
    return [("adam", lambda **kw: _icnn(opt="adam", **kw)), ("bundle_entropy", lambda **kw: _icnn(opt="bundle_entropy", **kw)),
            ("ddpg", lambda **kw: _flat(rl_agent.DDPGAgent, **kw)), ("naf", lambda **kw: _flat(rl_agent.NAFAgent, **kw))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", _pairs(), ids=[p[0] for p in _pairs()])
def test_row_e_is_the_single_environment_call(name, make):
    obs = np.random.RandomState(4).randn(3, DIMO).astype(np.float32) * np.array([[1.0], [8.0], [0.1]], np.float32)
    vec, one = make(n_envs=3), make(warmup=4, rmsize=8)
    vec.reset(obs)
    got = vec.act(test=True)
    assert got.shape == (3, DIMA)
    for e in range(3):
        one.reset(obs[e])
        assert np.array_equal(got[e], one.act(test=True)), (name, e)
    assert len({tuple(r) for r in got.tolist()}) == 3
    # with noise: the raw rows plus the device's noise, clipped; the reset mask zeroes the rows it names
    noisy = vec.act()
    noise = vec.explorer.noise.cpu().numpy()
    assert noise.all() and int(vec.explorer.counter.item()) == 1
    raw = vec._raw_actions().cpu().numpy().astype(np.float64)
    assert np.array_equal(noisy, np.clip(raw + noise, -1, 1))
    vec.reset(obs, mask=np.array([False, True, False]))
    after = vec.explorer.noise.cpu().numpy()
    assert not after[1].any() and np.array_equal(after[[0, 2]], noise[[0, 2]])
    vec.reset(obs)
    assert not vec.explorer.noise.any()


def _run(agent, world, steps, start=0, first=True):
    obs0, obs2, rew, term = world
    if first:
        agent.reset(obs0)
    recorded = []
    for s in range(start, start + steps):
        obs1 = agent.observation.copy()
        action = agent.act()
        agent.observe(rew[s], term[s], obs2[s])
        recorded.append((obs1, term[s], action.copy(), rew[s]))
    return recorded


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_vector_cycle_equals_the_hand_composition(capture):
    """five vector steps of E = 3 at warmup 6: the last three train (t = 9, 12, 15), two iterations each; with capture the
    second of them records the graph and the third replays it.  The recorded transitions through the NumPy memory and an
    independent CriticTrainer.step; the noise against the restatement's deviates."""
    E = 3
    agent = _icnn(n_envs=E, capture=capture)
    world = _world(5, E, 3)
    recorded = _run(agent, world, 5)
    assert agent.t == 15 and np.array_equal(agent.observation, world[1][4])
    host = ref.VecReplayMemory(8, E, DIMO, DIMA, 9)
    tr = base._trainer(_spec(), 4, 23)
    worst = 0
    for s, (o, term, a, r) in enumerate(recorded, 1):
        host.enqueue(o, term, a, r)
        if s * E > 6:
            for _ in range(2):
                mb = host.minibatch(4)
                worst = max(worst, int(mb[6].max()))
                tr.step(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in mb[:5]])
    assert worst < ref.MAX_ATTEMPTS
    mem = agent.memory
    assert (mem.n, mem.i) == (host.n, host.i) == (5, 5) and mem.ctrl.cpu().tolist()[:5] == [5, 5, 6, 0, 0]
    for name in ("observations", "actions", "rewards", "terminals"):
        assert np.array_equal(getattr(mem, name).cpu().numpy(), getattr(host, name)), name
    base._same_trainers(agent.trainer, tr)
    assert tr.t == 6 and bool(torch.isfinite(agent.loss)) and torch.equal(agent.loss, tr.loss)
    mem.raise_on_error()
    # the noise after five steps: the restatement's recurrence on its own deviates (tests/test_explore.py's bound)
    noise, scale = np.zeros((E, DIMA)), np.zeros((E, DIMA))
    for s in range(5):
        z = ref.normals(s, E, DIMA, 9)
        _, noise = ref.explore(np.zeros((E, DIMA)), noise, z, 0.15, 0.1)
        scale += 0.1 * np.abs(z)
    assert np.max(np.abs(agent.explorer.noise.cpu().numpy() - noise) / scale) <= 8 * 4.232e-16
    assert int(agent.explorer.counter.item()) == 5


@pytest.mark.gpu
def test_test_steps_store_and_train_nothing():
    agent = _icnn(n_envs=3)
    obs0, obs2, rew, term = _world(1, 3, 5)
    agent.reset(obs0)
    agent.act(test=True)
    agent.observe(rew[0], term[0], obs2[0], test=True)
    assert agent.t == 0 and agent.memory.n == 0 and agent.memory.ctrl.cpu().tolist()[:3] == [0, 0, 0]
    assert np.array_equal(agent._obs_dev.cpu().numpy(), obs2[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", _pairs()[::2], ids=["adam", "ddpg"])
def test_checkpoint_round_trip_and_refusals(name, make, tmp_path):
    """after a round trip the next two steps reproduce bit for bit; files of another n_envs, or of the other kind, are refused"""
    E = 3
    world = _world(6, E, 6)
    a = make(n_envs=E)
    _run(a, world, 4)
    path = str(tmp_path / "vec.npz")
    checkpoint.save(path, a)
    b = make(n_envs=E, seed=10)                                          # another seed: the file's takes over
    checkpoint.load(path, b)
    assert torch.equal(a.explorer.noise, b.explorer.noise) and torch.equal(a.explorer.counter, b.explorer.counter)
    assert torch.equal(a.memory.ctrl, b.memory.ctrl) and torch.equal(a.memory.observations, b.memory.observations)
    ra, rb = _run(a, world, 2, 4, first=False), _run(b, world, 2, 4, first=False)
    for x, y in zip(ra, rb):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])
    assert a.t == b.t == 18 and torch.equal(a.loss, b.loss) and torch.equal(a.memory.actions, b.memory.actions)
    assert torch.equal(a.memory.ctrl, b.memory.ctrl) and torch.equal(a.explorer.noise, b.explorer.noise)
    # ---- refusals
    with pytest.raises(ValueError, match="n_envs"):
        checkpoint.load(path, make(n_envs=2))
    with pytest.raises(ValueError, match="n_envs"):
        checkpoint.load(path, make(rmsize=8))                            # a single-environment agent, the same time rows
    legacy = make(warmup=4, rmsize=8)
    legacy.reset(world[0][0])
    legacy.act()
    legacy.observe(0.5, False, world[1][0][0])
    old = str(tmp_path / "one.npz")
    checkpoint.save(old, legacy)
    with pytest.raises(ValueError, match="n_envs"):
        checkpoint.load(old, make(n_envs=1, rmsize=8))
    again = make(warmup=4, rmsize=8, seed=10)
    checkpoint.load(old, again)                                          # single-environment files load as before
    assert again.t == 1 and np.array_equal(again.noise, legacy.noise)
