"""The replay memory of E lockstep environments (icnn_be_vec_replay_enqueue / _sample, rl_agent.VecReplayMemory)
against its NumPy statement tests/vec_replay_ref.py, all bit for bit: the arrays after enqueues that wrap the cursor, the
minibatch at every shape the gather takes another path for (rows shorter and longer than a wave, aligned and odd, batches that
fill and do not fill the last workgroup of four samples), the rejection rule per column, the draw counter under graph replay,
and E = 1 against the scalar memory on the same transitions."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import replay_ref
import vec_replay_ref as ref
from icnn_amd import _lib, rl_agent

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_vec_replay_enqueue", "icnn_be_vec_replay_sample", "icnn_be_explore"]

# name -> (steps T, n_envs E, dimO, dimA, batch, enqueues, share of terminals): every T of {3, 4, 8}, E of {1, 2, 3, 5}, dimO of
# {1, 3, 4, 17, 65}, dimA of {1, 6, 65} and batch of {1, 4, 5, 9}
CASES = {
    "T3_E2": (3, 2, 3, 1, 4, 2, 0.0),             # n = 2: only time row 0 can be drawn, the successor is row 1
    "T4_E1": (4, 1, 1, 6, 1, 3, 0.0),             # cursor 3, n = 3: rows 0 and 1
    "T4_E5_wrapped": (4, 5, 4, 65, 9, 6, 0.1),    # wrapped: cursor 2, n = 3, candidates 0 and 1; 16-byte rows
    "T8_E3": (8, 3, 17, 6, 5, 5, 0.2),            # partly filled, odd rows
    "T8_E3_wrapped": (8, 3, 65, 1, 9, 11, 0.2),   # wrapped: cursor 3 inside [0, n - 2]; rows longer than a wave
    "T8_E5": (8, 5, 3, 65, 4, 13, 0.3),
    "T8_E2": (8, 2, 1, 1, 5, 7, 0.3),
}


def _transitions(count, E, dimO, dimA, p_term, seed):
    rng = np.random.RandomState(seed)
    obs = rng.randn(count, E, dimO).astype(np.float32)
    act = np.clip(rng.randn(count, E, dimA) * 0.7, -1, 1)            # float64 values float32 cannot hold
    rew = rng.randn(count, E).astype(np.float32)
    term = (rng.rand(count, E) < p_term).astype(np.uint8)
    return obs, term, act, rew


def _fill_host(mem, data):
    for o, t, a, r in zip(*data):
        mem.enqueue(o, t, a, r)
    return mem


def _fill_dev(mem, data):
    obs, term, act, rew = [torch.from_numpy(x).cuda() for x in data]
    for s in range(obs.shape[0]):
        mem.enqueue(obs[s].contiguous(), term[s].contiguous(), act[s].contiguous(), rew[s].contiguous())
    return mem


@functools.lru_cache(maxsize=None)
def _data(name):
    T, E, dimO, dimA, batch, count, p_term = CASES[name]
    return _transitions(count, E, dimO, dimA, p_term, 1 + list(CASES).index(name))


def _host(name, seed, data=None):
    T, E, dimO, dimA = CASES[name][:4]
    return _fill_host(ref.VecReplayMemory(T, E, dimO, dimA, seed), data or _data(name))


def _equal_minibatch(got, want):
    obs, act, rew, ob2, term, idx = [t.cpu().numpy() for t in got]
    assert idx.dtype == np.int32 and act.dtype == np.float64 and term.dtype == np.uint8
    for g, w in zip((idx, obs, act, rew, ob2, term), (want[5], want[0], want[1], want[2], want[3], want[4])):
        assert g.shape == w.shape and np.array_equal(g, w)


# ------------------------------------------------------------------------------------------------ CPU


def test_cases_cover_the_shapes():
    col = lambda i: {c[i] for c in CASES.values()}
    assert col(0) == {3, 4, 8} and col(1) == {1, 2, 3, 5} and col(2) == {1, 3, 4, 17, 65} and col(3) == {1, 6, 65}
    assert col(4) == {1, 4, 5, 9}
    assert any(c[5] > c[0] for c in CASES.values())                  # some wrap the cursor


def test_new_exports_declared_and_struct_layout():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and ("ICNN_BE_API int %s(" % name) in header
    assert lib.icnn_be_struct_size(22) == C.sizeof(_lib.VecReplay) == 4 * 4 + 5 * 8
    assert lib.icnn_be_struct_size(21) == lib.icnn_be_struct_size(23) == 0


def test_one_environment_is_the_scalar_restatement():
    """E = 1: the vector statement draws what replay_ref.ReplayMemory draws on the same transitions"""
    data = _transitions(45, 1, 5, 2, 0.15, 3)
    vec = _fill_host(ref.VecReplayMemory(32, 1, 5, 2, 7), data)
    one = replay_ref.ReplayMemory(32, 5, 2, 7)
    for o, t, a, r in zip(*data):
        one.enqueue(o[0], t[0], a[0], r[0])
    assert (vec.i, vec.n) == (one.i, one.n) == (13, 31)
    for _ in range(2):
        for v, s in zip(vec.minibatch(9), one.minibatch(9)):
            assert np.array_equal(v, s)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[1] > 1 and c[4] > 1 and c[0] > 3])
def test_the_environment_has_its_own_domain_tag(name):
    """what the time index's words (tag 0) would give for the environment differs on these cases: a sampler that drew both
    from one word fails the comparison below"""
    batch = CASES[name][4]
    assert not np.array_equal(_host(name, 11).minibatch(batch)[5], _host(name, 11).minibatch(batch, env_tag=0)[5])


def test_successor_stride_matters_on_these_cases():
    """rows (c, e) and (c + 1, e) lie E * dimO floats apart: the row dimO floats on is another environment's"""
    for name, c in CASES.items():
        if c[1] > 1:
            m = _host(name, 11)
            want = m.minibatch(c[4])
            flat = m.observations.reshape(-1, c[2])
            assert not np.array_equal(flat[want[5] + 1], want[3]), name


def _vec(**kw):
    m = _lib.VecReplay()
    m.steps, m.n_envs, m.dimO, m.dimA = 8, 3, 3, 2
    m.observations, m.actions, m.rewards, m.terminals, m.ctrl = 64, 128, 192, 256, 320
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_bad_arguments_are_rejected_before_launch():
    """every call is invalid in exactly one way (the pointers are never dereferenced): nothing is launched"""
    lib = _lib.load()
    bad = (dict(steps=2), dict(n_envs=0), dict(dimO=0), dict(dimA=-1), dict(observations=None), dict(actions=None),
           dict(rewards=None), dict(terminals=None), dict(ctrl=None), dict(observations=66), dict(ctrl=322))

    def enq(m, obs=512, act=1024, rew=2048, term=4096):
        return lib.icnn_be_vec_replay_enqueue(None if m is None else C.byref(m), obs, act, rew, term, None)

    def smp(m, fill=4, batch=4, obs=512, act=576, rew=640, ob2=704, term=768, idx=832):
        return lib.icnn_be_vec_replay_sample(None if m is None else C.byref(m), fill, batch, 5, obs, act, rew, ob2, term, idx, None)
    assert enq(None) == -1 and smp(None) == -1
    for kw in bad:
        assert enq(_vec(**kw)) == -1 and smp(_vec(**kw)) == -1, kw
    assert enq(_vec(steps=1 << 20, n_envs=1 << 12)) == -2 and smp(_vec(steps=1 << 20, n_envs=1 << 12)) == -2
    for kw in (dict(obs=None), dict(act=None), dict(rew=None), dict(term=None), dict(obs=514), dict(act=1028), dict(rew=2050)):
        assert enq(_vec(), **kw) == -1, kw
    for kw in (dict(batch=0), dict(fill=1), dict(fill=8), dict(obs=None), dict(act=None), dict(rew=None), dict(ob2=None),
               dict(term=None), dict(idx=None), dict(obs=514), dict(act=580), dict(rew=641), dict(ob2=706), dict(idx=834)):
        assert smp(_vec(), **kw) == -1, kw
    with pytest.raises(ValueError, match="steps"):
        rl_agent.VecReplayMemory(2, 3, 3, 2, "cpu")


# ------------------------------------------------------------------------------------------------ GPU


@pytest.mark.gpu
def test_enqueue_matches_the_reference_bit_for_bit():
    data = _transitions(11, 3, 3, 2, 0.3, 5)
    assert np.any(data[2].astype(np.float32).astype(np.float64) != data[2]) and data[1].any()
    dev = _fill_dev(rl_agent.VecReplayMemory(8, 3, 3, 2, "cuda"), data)
    host = _fill_host(ref.VecReplayMemory(8, 3, 3, 2), data)
    assert (dev.i, dev.n) == (host.i, host.n) == (3, 7)
    assert dev.ctrl.cpu().tolist()[:5] == [3, 7, 0, 0, 0]
    for name in ("observations", "actions", "rewards", "terminals"):
        assert np.array_equal(getattr(dev, name).cpu().numpy(), getattr(host, name)), name
    dev.raise_on_error()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sampling_matches_the_reference(name):
    """two consecutive launches are the statement's draws d and d + 1"""
    T, E, dimO, dimA, batch = CASES[name][:5]
    dev = _fill_dev(rl_agent.VecReplayMemory(T, E, dimO, dimA, "cuda", 11), _data(name))
    host = _host(name, 11)
    assert (dev.i, dev.n) == (host.i, host.n)
    for _ in range(2):
        want = host.minibatch(batch)
        assert not want[7].any()
        got = dev.sample(batch)
        _equal_minibatch(got, want)
        c, e = np.divmod(want[5], E)
        assert np.all((c >= 0) & (c <= host.n - 2) & (c != host.i)) and not host.terminals[c, e].any()
    assert dev.ctrl.cpu().tolist()[:5] == [host.i, host.n, 2, 0, 0]
    dev.raise_on_error()


@pytest.mark.gpu
def test_a_column_of_terminals_and_the_cursor_row_are_never_drawn():
    obs, term, act, rew = _transitions(11, 2, 3, 2, 0.0, 8)
    term[:, 0] = 1                                                      # environment 0: every transition terminal
    dev = _fill_dev(rl_agent.VecReplayMemory(8, 2, 3, 2, "cuda", 3), (obs, term, act, rew))
    host = _fill_host(ref.VecReplayMemory(8, 2, 3, 2, 3), (obs, term, act, rew))
    assert 0 < host.i <= host.n - 2
    want = host.minibatch(64)
    assert want[6].max() > 2 and not want[7].any()                      # some samples needed several attempts
    got = dev.sample(64)
    _equal_minibatch(got, want)
    idx = got[5].cpu().numpy()
    assert np.all(idx % 2 == 1) and np.all(idx // 2 != host.i) and len(set((idx // 2).tolist())) > 2
    assert dev.status == 0


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 2])
def test_attempt_bound_where_every_candidate_is_terminal(E):
    """one environment (or both) whose every transition is terminal: each sample keeps its 256th candidate, in range, and the
    status word says so"""
    obs, term, act, rew = _transitions(6, E, 3, 2, 0.0, 9)
    term[:] = 1
    dev = _fill_dev(rl_agent.VecReplayMemory(8, E, 3, 2, "cuda", 5), (obs, term, act, rew))
    host = _fill_host(ref.VecReplayMemory(8, E, 3, 2, 5), (obs, term, act, rew))
    want = host.minibatch(5)
    assert want[7].all() and np.all(want[6] == ref.MAX_ATTEMPTS)
    got = dev.sample(5)
    _equal_minibatch(got, want)
    assert dev.status == _lib.REPLAY_ST_EXHAUSTED
    with pytest.raises(RuntimeError, match="256 attempts"):
        dev.raise_on_error()
    assert dev.ctrl.cpu().tolist()[:5] == [host.i, host.n, 1, _lib.REPLAY_ST_EXHAUSTED, 0]


@pytest.mark.gpu
def test_draw_counter_advances_under_graph_replay():
    """a captured [enqueue, sample] replayed three times: three time rows written from the same device buffers, and draws d,
    d + 1, d + 2 of the statement"""
    name = "T8_E3"
    T, E, dimO, dimA, batch = CASES[name][:5]
    dev = _fill_dev(rl_agent.VecReplayMemory(T, E, dimO, dimA, "cuda", 11), _data(name))
    host = _host(name, 11)
    out = dev.sample(batch)                                             # eager: first-call allocations, draw 0
    _equal_minibatch(out, host.minibatch(batch))
    step = [torch.from_numpy(x[0]).cuda() for x in _transitions(1, E, dimO, dimA, 0.0, 77)]
    bufs = [torch.empty_like(t) for t in out]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.enqueue(*step)
        dev._sample(batch, *bufs)
    dev.i, dev.n = (dev.i - 1) % T, host.n                              # the capture launched nothing: undo the host mirrors
    for r in range(3):
        g.replay()
        dev.i, dev.n = (dev.i + 1) % T, min(T - 1, dev.n + 1)
        host.enqueue(*[t.cpu().numpy() for t in step])
        torch.cuda.synchronize()
        _equal_minibatch(bufs, host.minibatch(batch))
        assert dev.ctrl.cpu().tolist()[:5] == [host.i, host.n, 2 + r, 0, 0]
    assert np.array_equal(dev.observations.cpu().numpy(), host.observations)


@pytest.mark.gpu
def test_one_environment_equals_the_scalar_memory():
    """E = 1: outputs, idx and the control block equal ReplayMemory's on the same transitions"""
    data = _transitions(45, 1, 67, 3, 0.15, 3)
    vec = _fill_dev(rl_agent.VecReplayMemory(32, 1, 67, 3, "cuda", 7), data)
    one = rl_agent.ReplayMemory(32, 67, 3, "cuda", 7)
    for o, t, a, r in zip(*data):
        one.enqueue(o[0], t[0], a[0], r[0])
    assert (vec.i, vec.n) == (one.i, one.n) == (13, 31)
    assert torch.equal(vec.observations[:, 0], one.observations) and torch.equal(vec.actions[:, 0], one.actions)
    assert torch.equal(vec.terminals[:, 0], one.terminals) and torch.equal(vec.rewards[:, 0], one.rewards)
    for batch in (9, 4):
        for v, s in zip(vec.sample(batch), one.sample(batch)):
            assert torch.equal(v, s)
    assert torch.equal(vec.ctrl, one.ctrl) and vec.ctrl.cpu().tolist()[:5] == [13, 31, 2, 0, 0]
