"""The RL agent on the device (icnn_amd/rl_agent.py, icnn_be_replay_enqueue, icnn_be_replay_sample, be_rl_replay.hip,
CriticTrainer.step_buffers) against tests/replay_ref.py: Philox4x32-10 against its published vectors, the restatement
against the reference's own class (tests/golden/replay__wrap.npz, tools/gen_golden_replay.py), the ABI and its argument
checks (CPU); enqueue, sampling, the attempt bound, step_buffers, graph capture and the agent's cycle (GPU)."""
import ctypes as C
import dataclasses
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import replay_ref as ref
from icnn_amd import _lib, picnn, rl_adam, rl_agent, rl_train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "replay__wrap.npz")
BATCHES = (1, 5, 256, 257)                   # one wave, a partial workgroup of four waves, whole workgroups, one wave more


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, want):
    assert " ".join("%08x" % w for w in ref.philox4x32_10(counter, key)) == want


def test_candidates_cover_the_range_and_nothing_else():
    for n in (2, 3, 10, 63):
        c = [ref.candidate(7, d, k, 0, n) for d in range(4) for k in range(200)]
        assert min(c) == 0 and max(c) == n - 2


def test_restatement_reproduces_the_reference_class():
    """replay_ref fed the recorded candidate stream makes the decisions RL/src/replay_memory.py made, array for array, at
    every fill state of the fixture: before the wrap, at it and after it."""
    g = np.load(GOLDEN)
    mem = ref.ReplayMemory(int(g["size"]), g["obs_in"].shape[1], g["act_in"].shape[1])
    stream = iter(g["stream"].tolist())
    at, used, seen = list(g["sample_at"]), 0, 0
    assert g["n"].max() == mem.size - 1 and (g["i"][1:] < g["i"][:-1]).any() and 0.15 < g["term_in"].mean() < 0.35
    for e in range(g["obs_in"].shape[0]):
        mem.enqueue(g["obs_in"][e], g["term_in"][e], g["act_in"][e], g["rew_in"][e])
        if e + 1 in at:
            s = at.index(e + 1)
            o, a, r, o2, t2, idx, attempts, exhausted = mem.minibatch(int(g["batch"]), candidates=stream)
            used += int(attempts.sum())
            assert (mem.n, mem.i, used) == (g["n"][s], g["i"][s], g["stream_end"][s])
            assert np.array_equal(idx, g["idx"][s]) and np.array_equal(o, g["o"][s]) and np.array_equal(o2, g["o2"][s])
            assert a.dtype == np.float64 and np.array_equal(a, g["a"][s].astype(np.float64)) and g["a"].dtype == np.float32
            assert np.array_equal(r, g["r"][s]) and np.array_equal(t2, g["t2"][s]) and not exhausted.any()
            seen += 1
    assert seen == len(at) and used == g["stream"].size and (g["stream_end"] > np.arange(1, seen + 1) * g["batch"]).any()


def test_new_exports_declared_and_struct_layout():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in ("icnn_be_replay_enqueue", "icnn_be_replay_sample"):
        assert re.search(r"ICNN_BE_API\s+int\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.icnn_be_struct_size(9) == C.sizeof(_lib.Replay) == 56
    assert lib.icnn_be_abi_version() == 12
    assert "#define ICNN_BE_REPLAY_MAX_ATTEMPTS %d" % _lib.REPLAY_MAX_ATTEMPTS in header
    assert "#define ICNN_BE_REPLAY_CTRL_INTS %d" % _lib.REPLAY_CTRL_INTS in header
    assert ref.MAX_ATTEMPTS == _lib.REPLAY_MAX_ATTEMPTS == 256
    assert _lib.replay_stage_bytes(17, 6) == 8 * 6 + 4 * 17 + 8


def _replay(**kw):
    m = _lib.Replay()
    m.size, m.dimO, m.dimA, m.observations, m.actions, m.rewards, m.terminals, m.ctrl = 8, 3, 2, 64, 128, 192, 256, 320
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _sample_call(lib, m=None, **kw):
    a = dict(fill=5, batch=4, seed=0, obs=512, act=576, rew=640, ob2=704, term=768, idx=832)
    a.update(kw)
    return lib.icnn_be_replay_sample(None if m is None else C.byref(m), a["fill"], a["batch"], a["seed"], a["obs"], a["act"],
                                     a["rew"], a["ob2"], a["term"], a["idx"], None)


def test_bad_arguments_are_rejected_before_launch():
    """Every call below is invalid in exactly one way (the pointers are never dereferenced): EINVAL, nothing launched."""
    lib = _lib.load()
    bad_memory = (dict(size=2), dict(size=0), dict(dimO=0), dict(dimA=0), dict(dimA=-1), dict(observations=None),
                  dict(actions=None), dict(rewards=None), dict(terminals=None), dict(ctrl=None), dict(observations=66),
                  dict(actions=130), dict(rewards=193), dict(ctrl=322))
    assert lib.icnn_be_replay_enqueue(None, 1024, None) == -1
    for kw in bad_memory:
        assert lib.icnn_be_replay_enqueue(C.byref(_replay(**kw)), 1024, None) == -1, kw
    assert lib.icnn_be_replay_enqueue(C.byref(_replay()), None, None) == -1
    assert lib.icnn_be_replay_enqueue(C.byref(_replay()), 1028, None) == -1
    assert _sample_call(lib) == -1
    for kw in bad_memory:
        assert _sample_call(lib, _replay(**kw)) == -1, kw
    for kw in (dict(batch=0), dict(batch=-2), dict(fill=1), dict(fill=0), dict(fill=8), dict(obs=None), dict(act=None),
               dict(rew=None), dict(ob2=None), dict(term=None), dict(idx=None), dict(obs=514), dict(act=580), dict(rew=641),
               dict(ob2=706), dict(idx=834)):
        assert _sample_call(lib, _replay(), **kw) == -1, kw


def test_agent_refuses_a_warmup_the_sampler_cannot_serve():
    """warmup >= 2 is checked before anything touches the device"""
    with pytest.raises(ValueError, match="warmup"):
        rl_agent.Agent(None, None, warmup=1)
    with pytest.raises(ValueError, match="size"):
        rl_agent.ReplayMemory(2, 3, 2, "cpu")


# ------------------------------------------------------------------------------------------------ GPU


def _transitions(count, dimO, dimA, p_term, seed):
    rng = np.random.RandomState(seed)
    obs = rng.randn(count, dimO).astype(np.float32)
    act = np.clip(rng.randn(count, dimA) * 0.7, -1, 1)               # float64 values float32 cannot hold
    rew = rng.randn(count).astype(np.float32)
    term = rng.rand(count) < p_term
    return obs, term, act, rew


def _fill(mem, data):
    for o, t, a, r in zip(*data):
        mem.enqueue(o, t, a, r)
    return mem


# name -> (size, dimO, dimA, enqueues, share of terminals, data seed)
SAMPLE_CASES = {
    "n2": (16, 17, 6, 2, 0.0, 1),                      # only index 0 can be drawn
    "partly_filled": (40, 1, 1, 25, 0.1, 2),
    "wrapped_odd_rows": (32, 67, 3, 45, 0.15, 3),      # rows longer than a wave and of odd length; cursor 13 inside [0, n - 2]
    "aligned_rows_terminals": (64, 64, 4, 50, 0.3, 4),  # 16-byte-aligned rows
}


@functools.lru_cache(maxsize=None)
def _case(name):
    size, dimO, dimA, count, p_term, seed = SAMPLE_CASES[name]
    data = _transitions(count, dimO, dimA, p_term, seed)
    if name == "n2":
        assert not data[1].any()
    return size, dimO, dimA, data


def _pair(name, seed):
    size, dimO, dimA, data = _case(name)
    return (_fill(rl_agent.ReplayMemory(size, dimO, dimA, "cuda", seed), data), _fill(ref.ReplayMemory(size, dimO, dimA, seed), data))


def _equal_minibatch(got, want, mem):
    obs, act, rew, ob2, term, idx = [t.cpu().numpy() for t in got]
    w_obs, w_act, w_rew, w_ob2, w_term, w_idx, attempts, exhausted = want
    assert attempts.max() < ref.MAX_ATTEMPTS and not exhausted.any()       # the condition the comparison rests on
    assert idx.dtype == np.int32 and act.dtype == np.float64 and term.dtype == np.uint8
    assert np.array_equal(idx, w_idx)
    assert np.all((idx >= 0) & (idx <= mem.n - 2) & (idx != mem.i)) and not mem.terminals[idx].any()
    assert np.array_equal(obs, w_obs) and np.array_equal(act, w_act) and np.array_equal(rew, w_rew)
    assert np.array_equal(ob2, w_ob2) and np.array_equal(term, w_term)


@pytest.mark.gpu
def test_enqueue_matches_the_reference_bit_for_bit():
    data = _transitions(20, 3, 2, 0.3, 5)
    assert np.any(data[2].astype(np.float32).astype(np.float64) != data[2]) and data[1].any()
    dev, host = _fill(rl_agent.ReplayMemory(8, 3, 2, "cuda"), data), _fill(ref.ReplayMemory(8, 3, 2), data)
    assert (dev.i, dev.n) == (host.i, host.n) == (4, 7)
    assert dev.ctrl.cpu().tolist()[:5] == [host.i, host.n, 0, 0, 0]
    assert np.array_equal(dev.observations.cpu().numpy(), host.observations)
    assert np.array_equal(dev.actions.cpu().numpy(), host.actions)
    assert np.array_equal(dev.rewards.cpu().numpy(), host.rewards)
    assert np.array_equal(dev.terminals.cpu().numpy(), host.terminals)
    dev.raise_on_error()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", list(SAMPLE_CASES))
def test_sampling_matches_the_reference(name, batch):
    """two consecutive launches are the reference's draws d and d + 1 at the same seed"""
    dev, host = _pair(name, 11)
    if name == "n2":
        assert host.n == 2
    if name == "wrapped_odd_rows":
        assert host.n == host.size - 1 and 0 < host.i <= host.n - 2
    if name == "aligned_rows_terminals":
        assert 0.2 < host.terminals[:host.n].mean() < 0.4
    first, second = dev.sample(batch), dev.sample(batch)
    for got in (first, second):
        _equal_minibatch(got, host.minibatch(batch), host)
    if name == "n2":
        assert not first[5].any()
    elif batch > 5:
        assert not torch.equal(first[5], second[5])
    assert dev.ctrl.cpu().tolist()[:5] == [host.i, host.n, 2, 0, 0]     # the draw counter advanced, the ticket is re-armed
    dev.raise_on_error()


@pytest.mark.gpu
def test_reset_memory_repeats_its_sequence():
    dev, host = _pair("partly_filled", 12)
    first = [t.clone() for t in dev.sample(37)]
    dev.sample(37)
    dev.reset()
    assert (dev.n, dev.i) == (0, 0) and dev.ctrl.cpu().tolist() == [0] * _lib.REPLAY_CTRL_INTS
    with pytest.raises(RuntimeError, match="EINVAL"):
        dev.sample(37)                                                     # the host's n < 2: refused before launch
    _fill(dev, _case("partly_filled")[3])
    again = dev.sample(37)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    _equal_minibatch(again, host.minibatch(37), host)
    other = _pair("partly_filled", 13)[0].sample(37)
    assert not torch.equal(other[5], again[5])                             # another seed, another sequence


@pytest.mark.gpu
def test_attempt_bound_sets_the_status_bit_and_keeps_indices_in_range():
    """every filled slot is terminal, so no candidate is ever valid: the launch must return with each sample at its 256th
    candidate (in range) and the error visible to the host"""
    data = _transitions(10, 3, 2, 2.0, 6)
    assert data[1].all()
    dev, host = _fill(rl_agent.ReplayMemory(16, 3, 2, "cuda", 5), data), _fill(ref.ReplayMemory(16, 3, 2, 5), data)
    got = dev.sample(9)
    want = host.minibatch(9)
    assert want[7].all() and np.all(want[6] == ref.MAX_ATTEMPTS)
    idx = got[5].cpu().numpy()
    assert np.all((idx >= 0) & (idx <= host.n - 2)) and np.array_equal(idx, want[5])
    assert np.array_equal(got[3].cpu().numpy(), host.observations[idx + 1])
    assert dev.status == _lib.REPLAY_ST_EXHAUSTED
    with pytest.raises(RuntimeError, match="256 attempts"):
        dev.raise_on_error()
    assert dev.ctrl.cpu().tolist()[:5] == [host.i, host.n, 1, _lib.REPLAY_ST_EXHAUSTED, 0]


def _critic_spec(batchnorm=False, szs=(5,), dimO=17, dimA=6):
    return dataclasses.replace(picnn.halfcheetah_spec(), n_features=dimO, n_labels=dimA, action_box=False, batchnorm=batchnorm,
                               szs=szs)


def _models(spec, seed):
    params = picnn.init_params(spec, seed, "spread", yu_bias=1.0, gate_bias=1.0)
    return picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda")


def _trainer(spec, B, seed):
    tr = rl_train.CriticTrainer(*_models(spec, seed), B, max_iter=50)
    tr.initialise()
    return tr


def _trainer_state(tr):
    out = [tr.opt.theta, tr.opt.m, tr.opt.v, tr.opt.step_count, tr.opt.arena, tr.follower.theta, tr.follower.arena]
    return out


def _same_trainers(a, b):
    for x, y in zip(_trainer_state(a), _trainer_state(b)):
        assert torch.equal(x, y)
    for ma, mb in ((a.critic, b.critic), (a.target, b.target)):
        sa, sb = ma.get_bn_stats(), mb.get_bn_stats()
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("batchnorm, szs", [(False, (5,)), (True, (5,)), (True, (6, 5))], ids=["plain", "bn", "bn_two_layers"])
def test_step_buffers_equals_step_on_the_sampled_minibatch(batchnorm, szs):
    spec, B = _critic_spec(batchnorm, szs), 4
    data = _transitions(12, spec.n_features, spec.n_labels, 0.2, 7)
    m1 = _fill(rl_agent.ReplayMemory(16, spec.n_features, spec.n_labels, "cuda", 3), data)
    m2 = _fill(rl_agent.ReplayMemory(16, spec.n_features, spec.n_labels, "cuda", 3), data)
    a, b = _trainer(spec, B, 21), _trainer(spec, B, 21)
    _same_trainers(a, b)
    before = a.opt.theta.clone()
    for _ in range(2):
        idx = m1.sample_into(a).clone()
        la = a.step_buffers().clone()
        mb = m2.sample(B)
        assert torch.equal(idx, mb[5])
        lb = b.step(*mb[:5]).clone()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
    _same_trainers(a, b)
    assert a.t == 2 and not torch.equal(before, a.opt.theta)
    m1.raise_on_error()


@pytest.mark.gpu
def test_captured_sample_and_step_replays_equal_eager_iterations():
    spec, B = _critic_spec(), 4
    data = _transitions(12, spec.n_features, spec.n_labels, 0.2, 8)
    host = _fill(ref.ReplayMemory(16, spec.n_features, spec.n_labels, 4), data)
    want_idx = [host.minibatch(B)[5] for _ in range(6)]
    m_eager = _fill(rl_agent.ReplayMemory(16, spec.n_features, spec.n_labels, "cuda", 4), data)
    eager = _trainer(spec, B, 22)
    eager_idx, losses = [], []
    for _ in range(6):
        eager_idx.append(m_eager.sample_into(eager).cpu().numpy().copy())
        losses.append(eager.step_buffers().clone())
    for got, want in zip(eager_idx, want_idx):
        assert np.array_equal(got, want)
    # the captured side: a warm-up step outside the graph on a minibatch of zeros (first-call allocations), then undone
    m_cap = _fill(rl_agent.ReplayMemory(16, spec.n_features, spec.n_labels, "cuda", 4), data)
    cap, fresh = _trainer(spec, B, 22), _trainer(spec, B, 22)
    cap.step_buffers()
    torch.cuda.synchronize()
    for dst, src in zip(_trainer_state(cap), _trainer_state(fresh)):
        dst.copy_(src)
    torch.cuda.synchronize()
    g, idx_out, loss_out = torch.cuda.CUDAGraph(), [], []
    with torch.cuda.graph(g):
        for _ in range(2):
            idx_out.append(m_cap.sample_into(cap).clone())
            loss_out.append(cap.step_buffers().clone())
    cap_idx, cap_losses = [], []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        cap_idx += [t.cpu().numpy().copy() for t in idx_out]
        cap_losses += [t.clone() for t in loss_out]
    for got, want in zip(cap_idx, want_idx):
        assert np.array_equal(got, want)
    for a, b in zip(cap_losses, losses):
        assert torch.equal(a, b)
    _same_trainers(cap, eager)
    assert cap.t == 6 and m_cap.ctrl.cpu().tolist()[:5] == [host.i, host.n, 6, 0, 0]


def _point_mass():
    spec = importlib.util.spec_from_file_location("example_rl_agent", os.path.join(REPO, "examples", "rl_agent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PointMass


def _agent(spec, seed, **kw):
    return rl_agent.Agent(*_models(spec, 23), bsize=4, warmup=4, iters=2, rmsize=8, seed=seed, max_iter=50, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_agent_cycle_equals_the_hand_composition(capture):
    """12 environment steps over two episodes (the first ends by the environment's term after 5, the second is cut by tmax),
    memory of 8 so that it wraps; then the recorded transitions through replay_ref and an independent CriticTrainer.step"""
    spec = _critic_spec(dimO=4, dimA=2)
    agent = _agent(spec, 9, capture=capture)
    env = _point_mass()(4, 2, horizon=5, seed=1)
    recorded, steps = [], 0
    for episode, length in enumerate((5, 7)):
        env.horizon = 5 if episode == 0 else 100
        agent.reset(env.reset())
        for s in range(length):
            obs1 = np.array(agent.observation, np.float32)
            action = agent.act()
            obs2, rew, term = env.step(action)
            assert term == (episode == 0 and s == 4)
            term = term or (episode == 1 and s + 1 >= length)          # main.py:133, tmax
            agent.observe(rew, term, obs2)
            recorded.append((obs1, term, action.copy(), rew))
            steps += 1
    assert steps == agent.t == 12 and sum(t for _, t, _, _ in recorded) == 2
    host = ref.ReplayMemory(8, 4, 2, 9)
    tr = _trainer(spec, 4, 23)
    worst = 0
    for t, (o, term, a, r) in enumerate(recorded, 1):
        host.enqueue(o, term, a, r)
        if t > 4:
            for _ in range(2):
                mb = host.minibatch(4)
                worst = max(worst, int(mb[6].max()))
                tr.step(*[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in mb[:5]])
    assert worst < ref.MAX_ATTEMPTS
    assert (agent.memory.n, agent.memory.i) == (host.n, host.i) == (7, 4)
    assert agent.memory.ctrl.cpu().tolist()[:5] == [host.i, host.n, 16, 0, 0]
    _same_trainers(agent.trainer, tr)
    assert tr.t == 16 and bool(torch.isfinite(agent.loss)) and torch.equal(agent.loss, tr.loss)
    agent.memory.raise_on_error()


@pytest.mark.gpu
def test_agent_act_is_the_inner_adam_plus_ornstein_uhlenbeck_noise():
    spec = _critic_spec(dimO=4, dimA=2)
    agent = _agent(spec, 10, outheta=0.15, ousigma=0.1)
    obs = np.array([0.3, -0.2, 0.1, 0.05], np.float32)
    agent.reset(obs)
    raw = rl_adam.adam(agent.critic, torch.from_numpy(obs[None]), max_iter=50).cpu().numpy()[0]
    quiet = agent.act(test=True)
    assert quiet.shape == (2,) and quiet.dtype == np.float64 and np.array_equal(quiet, np.clip(raw, -1, 1))
    assert not agent.noise.any()
    rng, noise = np.random.RandomState(10), np.zeros(2)
    for _ in range(3):
        noise -= 0.15 * noise - 0.1 * rng.randn(2)
        got = agent.act()
        assert np.array_equal(agent.noise, noise) and np.array_equal(got, np.clip(raw + noise, -1, 1))
    assert np.any(got != quiet)
    agent.observe(0.0, False, obs, test=True)                              # a test step trains nothing and stores nothing
    assert agent.t == 0 and agent.memory.n == 0
    agent.reset(obs)
    assert not agent.noise.any()
