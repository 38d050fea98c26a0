"""The RL agent's critic training step on the device (rl_train.CriticTrainer; icnn_be_rl_td, be_rl_train.hip;
icnn_be_rl_critic_update, the critic instantiation of be_train_update.hip's kernel) against the host restatement of
Agent.train() in tests/rl_train_ref.py: the ABI and its argument checks, the closed-form gradient of the loss (CPU), each
kernel against NumPy, whole steps against the oracle, BatchNorm folds and graph capture (GPU)."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import bn_ref
import rl_train_ref as ref
from icnn_amd import _lib, picnn, rl_train, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, TAU, DISCOUNT, L2NORM, WD = 1e-3, 0.01, 0.99, 1e-4, 1e-3


def _critic_spec(batchnorm=False, szs=(200, 200)):
    return dataclasses.replace(picnn.halfcheetah_spec(), action_box=False, batchnorm=batchnorm, szs=szs)


def _params(spec, seed):
    return picnn.init_params(spec, seed, "spread", yu_bias=1.0, gate_bias=1.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _flat(spec, params):
    return np.concatenate([np.asarray(params[k], np.float32).reshape(-1) for k, _ in train.grad_layout(spec)])


TD_THREADS = 256                             # be_rl_train.hip


def rl_td_blocks(n_theta):
    """be_rl_train.hip rl_td_blocks: four grid strides per thread, 1 .. ICNN_BE_RL_TD_MAX_BLOCKS workgroups"""
    return max(1, min(-(-n_theta // (TD_THREADS * 4)), _lib.RL_TD_MAX_BLOCKS))


def _n_theta(spec):
    return sum(int(np.prod(s)) for _, s in train.grad_layout(spec))


# the critics of the TD cases: one workgroup, the default grid, and a grid capped at ICNN_BE_RL_TD_MAX_BLOCKS
TD_CRITICS = {"one_block": (5,), "default": (200, 200), "capped": (200, 200, 200)}
# critics whose n_theta % 4 is 0 and 2 (the halfcheetah ones give 1 and 3): a partial last group of four in the update
UPDATE_SPECS = {"mod4_0": dict(n_labels=7), "mod4_2": dict(n_labels=5)}


# ------------------------------------------------------------------------------------------------ CPU


def test_new_exports_declared_and_struct_layout():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in ("icnn_be_rl_td", "icnn_be_rl_critic_update"):
        assert re.search(r"ICNN_BE_API\s+int\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.icnn_be_struct_size(7) == C.sizeof(_lib.RlUpdateArgs)
    assert lib.icnn_be_struct_size(6) == C.sizeof(_lib.ParamUpdateArgs)
    assert lib.icnn_be_abi_version() == 12
    assert "#define ICNN_BE_RL_TD_MAX_BLOCKS %d" % _lib.RL_TD_MAX_BLOCKS in header


def _td_call(lib, **kw):
    a = dict(batch=4, n=6, e=64, act=128, rew=192, term=256, q2=320, act2=None, discount=0.99, theta=384, n_theta=100,
             decay=448, l2norm=1e-4, wd=1e-3, td=512, c=576, loss=640, work=1024)
    a.update(kw)
    return lib.icnn_be_rl_td(a["batch"], a["n"], a["e"], a["act"], a["rew"], a["term"], a["q2"], a["act2"], a["discount"],
                             a["theta"], a["n_theta"], a["decay"], a["l2norm"], a["wd"], a["td"], a["c"], a["loss"],
                             a["work"], None)


def _update_args(**kw):
    r = _lib.RlUpdateArgs()
    a = r.adam
    a.n, a.theta, a.m, a.v, a.grad, a.dest_off, a.dest, a.arena, a.step = 4, 16, 32, 48, 64, 80, 96, 112, 128
    a.arena_floats, a.lr, a.beta1, a.beta2, a.eps = 8, 1e-3, 0.9, 0.999, 1e-8
    r.target_theta, r.target_arena, r.decay = 256, 512, 768
    r.tau, r.l2norm, r.wd = 0.01, 1e-4, 1e-3
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_bad_arguments_are_rejected_before_launch():
    """Every call below is invalid in exactly one way (the pointers are never dereferenced): EINVAL, nothing launched."""
    lib = _lib.load()
    for kw in (dict(batch=0), dict(batch=-3), dict(n=0), dict(n_theta=0), dict(e=None), dict(act=None), dict(theta=None),
               dict(decay=None), dict(work=None), dict(act=132), dict(act2=12), dict(c=580), dict(work=1032), dict(e=66),
               dict(discount=float("nan")), dict(discount=float("inf")), dict(l2norm=-1.0), dict(wd=-1e-3)):
        assert _td_call(lib, **kw) == -1, kw
    assert lib.icnn_be_rl_critic_update(None, None) == -1
    for kw in (dict(tau=-0.01), dict(tau=1.5), dict(tau=float("nan")), dict(target_theta=None), dict(target_arena=None),
               dict(decay=None), dict(target_theta=260), dict(decay=770), dict(l2norm=-1.0), dict(wd=float("nan"))):
        assert lib.icnn_be_rl_critic_update(C.byref(_update_args(**kw)), None) == -1, kw
    r = _update_args()
    r.adam.n = 0
    assert lib.icnn_be_rl_critic_update(C.byref(r), None) == -1                 # what icnn_be_param_update refuses
    r = _update_args()
    r.adam.grad = 68
    assert lib.icnn_be_rl_critic_update(C.byref(r), None) == -1
    r = _update_args()
    r.adam.n_proj, r.adam.proj_begin[0], r.adam.proj_end[0] = 1, 0, 5
    assert lib.icnn_be_rl_critic_update(C.byref(r), None) == -1


@pytest.mark.parametrize("batchnorm", [False, True])
def test_decay_mask_covers_exactly_the_weights(batchnorm):
    spec = _critic_spec(batchnorm, szs=(200, 200, 200) if batchnorm else (200, 200))
    mask = rl_train.decay_mask(spec)
    at, names = 0, []
    for name, shape in train.grad_layout(spec):
        size = int(np.prod(shape))
        seg = mask[at:at + size]
        want = 1 if name.endswith("/W") else 0
        assert np.all(seg == want), name
        at += size
        names.append(name)
    assert at == mask.size
    decayed = [k for k in names if k.endswith("/W")]
    assert all(k.split("/")[0] in [n.split("/")[0] for n in names] for k in decayed)
    assert not any(k.endswith(("/b", "/gamma", "/beta")) for k in decayed)
    L = len(spec.szs)
    assert len(decayed) == 6 * L + 3             # u_i (L), z_i yu_u / yu / u (3 (L + 1)), z_i zu_u / zu_proj (2 L)
    if batchnorm:
        assert any(k.endswith("/gamma") for k in names)


@pytest.mark.parametrize("batchnorm", [False, True])
def test_closed_form_gradient_equals_autograd_of_the_loss(batchnorm):
    """c_j = -(2 td_j / B) and g += l2norm wd W on every W: float64 autograd of mean(td^2) + l2norm sum_W wd |W|^2/2
    with y held fixed, on a minibatch whose targets lie inside and beyond q +- 1 and with term mixed."""
    spec = _critic_spec(batchnorm, szs=(24, 16))
    params = _params(spec, 5)
    rng = np.random.RandomState(3)
    B = 32
    obs = rng.randn(B, spec.n_features).astype(np.float32)
    act = np.clip(rng.randn(B, spec.n_labels), -0.999, 0.999).astype(np.float32).astype(np.float64)
    theta64 = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    E, _ = ref.train_ref.energy(spec, theta64, torch.as_tensor(obs.astype(np.float64)), torch.as_tensor(act))
    E = E.numpy().astype(np.float32)
    rew = (3.0 * rng.randn(B)).astype(np.float32)
    term = rng.rand(B) < 0.4
    q2_src = (E + 2.0 * rng.randn(B)).astype(np.float32)
    q, y, td, c = ref.td(E, act, rew, term, q2_src, None, DISCOUNT, B)
    clipped_hi, clipped_lo = y == q + np.float32(1), y == q - np.float32(1)
    assert clipped_hi.any() and clipped_lo.any() and (~clipped_hi & ~clipped_lo).any() and term.any() and (~term).any()
    l2, wd = 1e-2, 0.5                                           # large, so the decay term is visible beside the TD part
    want, td64 = ref.autograd_loss_grad(spec, params, obs, act, y, ref.entropy_sum(act), l2, wd)
    assert np.allclose(td64, td, rtol=0, atol=1e-5)
    # the closed form with c from the float64 td (the autograd side differentiates that one)
    c64 = -(2.0 * td64 / B)
    got = ref.closed_form_grad(spec, params, obs, act, c64, l2, wd)
    for k in want:
        assert np.allclose(got[k], want[k], rtol=1e-5, atol=1e-7 * max(1.0, np.abs(want[k]).max())), k   # c as float32
    # and the float32 c the kernel forms is that one to float32 rounding
    assert np.allclose(c, c64, rtol=1e-6, atol=1e-9)


def test_td_cases_reach_the_grids_they_claim():
    grids = {k: rl_td_blocks(_n_theta(_critic_spec(szs=szs))) for k, szs in TD_CRITICS.items()}
    assert _lib.RL_TD_MAX_BLOCKS == 256 and grids == {"one_block": 1, "default": 209, "capped": 256}
    n = _n_theta(_critic_spec(szs=TD_CRITICS["one_block"]))
    assert TD_THREADS < n <= TD_THREADS * 4                       # one workgroup, some of its threads take a second stride
    n = _n_theta(_critic_spec(szs=TD_CRITICS["capped"]))
    assert n > 4 * TD_THREADS * _lib.RL_TD_MAX_BLOCKS              # the capped grid: threads past four strides
    assert _n_theta(_critic_spec()) % 4 in (1, 3)
    assert sorted(_n_theta(dataclasses.replace(_critic_spec(), **kw)) % 4 for kw in UPDATE_SPECS.values()) == [0, 2]


# ------------------------------------------------------------------------------------------------ GPU


def _trainer(spec, B, seed, tau=TAU, wd=WD, l2norm=L2NORM, max_iter=1000):
    params = _params(spec, seed)
    critic, target = picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda")
    tr = rl_train.CriticTrainer(critic, target, B, lr=LR, tau=tau, discount=DISCOUNT, l2norm=l2norm, wd=wd, max_iter=max_iter)
    tr.initialise()
    return tr


def _minibatch(spec, B, seed):
    rng = np.random.RandomState(seed)
    obs = rng.randn(B, spec.n_features).astype(np.float32)
    act = np.clip(rng.randn(B, spec.n_labels) * 0.6, -0.999, 0.999).astype(np.float32).astype(np.float64)
    rew = (2.0 * rng.randn(B)).astype(np.float32)
    ob2 = (obs + 0.1 * rng.randn(B, spec.n_features)).astype(np.float32)
    term = rng.rand(B) < 0.2
    return obs, act, rew, ob2, term


def _check_td(spec, B, with_act2):
    tr = _trainer(spec, B, 1)
    assert tr.opt.n == _n_theta(spec)
    obs, act, rew, ob2, term = _minibatch(spec, B, 2)
    rng = np.random.RandomState(4)
    e = (rng.randn(B) * 3).astype(np.float32)
    q2 = (e + 2.5 * rng.randn(B)).astype(np.float32)
    act2 = np.clip(rng.randn(B, spec.n_labels), -1, 1) if with_act2 else None
    tr.act.copy_(torch.from_numpy(act))
    tr.rew.copy_(torch.from_numpy(rew))
    tr.term.copy_(torch.from_numpy(term.astype(np.uint8)))
    a2 = torch.from_numpy(act2).cuda() if with_act2 else None
    tr.td_loss(torch.from_numpy(e).cuda(), torch.from_numpy(q2).cuda(), a2)
    torch.cuda.synchronize()
    q, y, td, c = ref.td(e, act, rew, term, q2, act2, DISCOUNT, B)
    if B >= 255:
        assert (y == q + np.float32(1)).any() and (y == q - np.float32(1)).any() and term.any()
    got_td = tr.td.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(q), np.abs(td)).astype(np.float32))
    assert np.all(np.abs(got_td - td) <= 2 * ulp)          # entropy's log may differ by an ulp
    assert np.all(np.abs(tr.c.cpu().numpy() - c) <= 2 * np.spacing(np.abs(c).astype(np.float32)) + 1e-30)
    theta = tr.opt.theta.cpu().numpy()
    want = ref.loss(td, theta, rl_train.decay_mask(spec), L2NORM, WD)
    assert abs(float(tr.loss.item()) - float(want)) <= 1e-6 * abs(float(want))
    first = tr.loss.clone()
    tr.td_loss(torch.from_numpy(e).cuda(), torch.from_numpy(q2).cuda(), a2)   # the ticket was re-armed; repeatable
    assert torch.equal(first, tr.loss)


@pytest.mark.gpu
@pytest.mark.parametrize("with_act2", [False, True])
def test_rl_td_matches_numpy(with_act2):
    spec = _critic_spec()
    assert rl_td_blocks(_n_theta(spec)) == 209
    _check_td(spec, 256, with_act2)


@pytest.mark.gpu
@pytest.mark.parametrize("with_act2", [False, True], ids=["q2", "act2"])
@pytest.mark.parametrize("B", [1, 255, 257, 1000])
@pytest.mark.parametrize("critic", list(TD_CRITICS))
def test_rl_td_at_every_grid_and_batch(critic, B, with_act2):
    """a one-workgroup grid, the default one and the capped one (threads past four strides), each at batches of one, on
    either side of a TD_THREADS multiple and past several of them"""
    spec = _critic_spec(szs=TD_CRITICS[critic])
    assert rl_td_blocks(_n_theta(spec)) == {"one_block": 1, "default": 209, "capped": 256}[critic]
    _check_td(spec, B, with_act2)


def _set_state(tr, rng, step):
    n = tr.opt.n
    theta = tr.opt.theta.cpu().numpy()
    theta_t = (theta + 1e-2 * rng.randn(n)).astype(np.float32)
    m = (1e-3 * rng.randn(n)).astype(np.float32)
    v = (1e-6 * rng.rand(n)).astype(np.float32)
    tr.follower.load(train.unpack_grad(tr.spec, torch.from_numpy(theta_t)))
    tr.opt.m.copy_(torch.from_numpy(m))
    tr.opt.v.copy_(torch.from_numpy(v))
    tr.opt.step_count.copy_(torch.tensor([step - 1, 0], dtype=torch.int32))
    g = (1e-2 * rng.randn(n)).astype(np.float32)
    g[rng.rand(n) < 0.05] = 0
    return theta, theta_t, m, v, g


def _check_critic_update(spec):
    tr = _trainer(spec, 8, 3)
    rng = np.random.RandomState(5)
    theta, theta_t, m, v, g = _set_state(tr, rng, 4)
    tr.update(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    th_r, tt_r, m_r, v_r = ref.critic_update(theta, theta_t, m, v, g, 4, rl_train.decay_mask(spec), tr.opt.map.proj, LR, TAU,
                                             L2NORM, WD)
    assert np.array_equal(_bits(tr.opt.theta.cpu().numpy()), _bits(th_r))
    assert np.array_equal(_bits(tr.follower.theta.cpu().numpy()), _bits(tt_r))
    assert np.array_equal(_bits(tr.opt.m.cpu().numpy()), _bits(m_r))
    assert np.array_equal(_bits(tr.opt.v.cpu().numpy()), _bits(v_r))
    assert tr.opt.step_count.cpu().tolist() == [4, 0]
    assert np.array_equal(_bits(tr.opt.arena.cpu().numpy()), _bits(tr.opt.map.scatter(th_r)))
    assert np.array_equal(_bits(tr.follower.arena.cpu().numpy()), _bits(tr.opt.map.scatter(tt_r)))


@pytest.mark.gpu
@pytest.mark.parametrize("batchnorm", [False, True])
def test_rl_critic_update_matches_numpy_bit_for_bit(batchnorm):
    _check_critic_update(_critic_spec(batchnorm, szs=(200, 200, 200) if batchnorm else (200, 200)))


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(UPDATE_SPECS))
def test_rl_critic_update_bit_for_bit_at_other_remainders(which):
    spec = dataclasses.replace(_critic_spec(), **UPDATE_SPECS[which])
    assert _n_theta(spec) % 4 == {"mod4_0": 0, "mod4_2": 2}[which]
    _check_critic_update(spec)


@pytest.mark.gpu
def test_tau_one_copies_the_pre_update_critic():
    """tau = 1: theta_t - (theta_t - theta) is theta exactly when theta_t lies within a factor two of theta (the difference
    is exact, Sterbenz), so the target must come out as the critic's theta BEFORE this step's Adam update."""
    spec = _critic_spec()
    tr = _trainer(spec, 8, 6, tau=1.0)
    rng = np.random.RandomState(7)
    theta, _, _, _, g = _set_state(tr, rng, 1)
    theta_t = (theta * (1 + 0.4 * rng.uniform(-1, 1, theta.size))).astype(np.float32)
    tr.follower.load(train.unpack_grad(spec, torch.from_numpy(theta_t)))
    tr.update(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tr.follower.theta.cpu().numpy()), _bits(theta))
    assert not np.array_equal(_bits(tr.opt.theta.cpu().numpy()), _bits(theta))


@pytest.mark.gpu
def test_decay_alone_moves_weights_and_not_biases():
    spec = _critic_spec()
    tr = _trainer(spec, 8, 8, wd=10.0, l2norm=1.0)
    theta = tr.opt.theta.cpu().numpy()
    tr.update(torch.zeros(tr.opt.n, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    after = tr.opt.theta.cpu().numpy()
    at = 0
    for name, shape in train.grad_layout(spec):
        size = int(np.prod(shape))
        before, now = theta[at:at + size], after[at:at + size]
        if name.endswith("/W"):
            nz = before != 0
            assert np.all(now[nz] != before[nz]), name
        else:
            assert np.array_equal(_bits(now), _bits(before)), name
        at += size


def _check_step(tr, batch, state, bn):
    """one device step against the oracle, teacher-forced from `state` (the device's weights before it)"""
    spec, B = tr.spec, tr.batch
    obs, act, rew, ob2, term = batch
    theta, theta_t, m, v, t, stats_c, stats_t = state
    pc = {k: a.numpy() for k, a in train.unpack_grad(spec, torch.from_numpy(theta)).items()}
    pt = {k: a.numpy() for k, a in train.unpack_grad(spec, torch.from_numpy(theta_t)).items()}
    # the target's context rows with its moving statistics, from a fresh model of its weights (the oracle's Adam input)
    fresh = picnn.FCModel(spec, pt, "cuda")
    if bn:
        fresh.set_bn_stats(stats_t)
    ctx2 = (fresh.context(torch.from_numpy(ob2), bn="moving") if bn else fresh.context(torch.from_numpy(ob2))).cpu().numpy()
    act2_o, iters_o, fbest_o = ref.target_actions(spec, pt, ctx2)
    assert int(tr.solver.iters.item()) == iters_o
    act2 = tr.act2.cpu().numpy()
    assert np.max(np.abs(act2 - act2_o)) <= 1e-9
    x64 = torch.as_tensor(obs.astype(np.float64))
    th64 = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in pc.items()}
    E = ref.train_ref.energy(spec, th64, x64, torch.as_tensor(act))[0].numpy().astype(np.float32)
    if bn:
        tt64 = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in pt.items()}
        a2 = torch.as_tensor(act2.astype(np.float32).astype(np.float64))
        q2 = ref.train_ref.energy(spec, tt64, torch.as_tensor(ob2.astype(np.float64)), a2)[0].numpy().astype(np.float32)
        _, _, td, c = ref.td(E, act, rew, term, q2, act2, DISCOUNT, B)
    else:
        assert np.max(np.abs(tr.q2_src.cpu().numpy() - fbest_o)) <= 1e-6
        _, _, td, c = ref.td(E, act, rew, term, fbest_o, None, DISCOUNT, B)
    mask = rl_train.decay_mask(spec)
    want = float(ref.loss(td, theta, mask, L2NORM, WD))
    assert abs(float(tr.loss.item()) - want) <= 1e-5 * abs(want)
    g64, _, _ = ref.train_ref.surrogate_grad64(spec, pc, obs, act, None, c)
    got = train.unpack_grad(spec, tr.grad.cpu())
    # the final layer's x-only term z{L}_u has the gradient sum_j c_j [u_{L-1}(x_j), 1], which can cancel to rounding
    # residue: compared against the size of the terms that cancel, as tests/test_train_grad.py does
    L = len(spec.szs)
    c32 = np.abs(c.astype(np.float32).astype(np.float64))
    u_last = ref.train_ref.last_u(spec, pc, obs)
    cancel = {"z%d_u/b" % L: np.sum(c32), "z%d_u/W" % L: np.sum(c32 * np.linalg.norm(u_last, axis=1))}
    for k, r in g64.items():
        err = np.linalg.norm(got[k].double().numpy() - r)
        assert err <= 1e-3 * np.linalg.norm(r) + 1e-7 or err <= 1e-5 * cancel.get(k, 0.0), k
    th_r, tt_r, m_r, v_r = ref.critic_update(theta, theta_t, m, v, tr.grad.cpu().numpy(), t + 1, mask, tr.opt.map.proj, LR,
                                             TAU, L2NORM, WD)
    assert np.array_equal(_bits(tr.opt.theta.cpu().numpy()), _bits(th_r))
    assert np.array_equal(_bits(tr.follower.theta.cpu().numpy()), _bits(tt_r))
    assert np.array_equal(_bits(tr.opt.m.cpu().numpy()), _bits(m_r))
    assert np.array_equal(_bits(tr.opt.v.cpu().numpy()), _bits(v_r))
    assert tr.t == t + 1
    if bn:
        _, bs_c = bn_ref.fc_context64(spec, pc, obs)
        _, bs_t = bn_ref.fc_context64(spec, pt, ob2)
        for model, start, bs in ((tr.critic, stats_c, bs_c), (tr.target, stats_t, bs_t)):
            want_s = bn_ref.fold32(start, bs, 1)
            for k, w in want_s.items():
                assert np.allclose(model.get_bn_stats()[k], w, rtol=1e-5, atol=1e-6), k


def _state(tr):
    return (tr.opt.theta.cpu().numpy(), tr.follower.theta.cpu().numpy(), tr.opt.m.cpu().numpy(), tr.opt.v.cpu().numpy(),
            tr.t, tr.critic.get_bn_stats(), tr.target.get_bn_stats())


@pytest.mark.gpu
def test_five_steps_against_the_oracle_teacher_forced():
    """B = 256 on the halfcheetah critic: act2 as tests/test_adam.py asserts it, the fed gradient within the RL-form
    tolerance of tests/test_train_grad.py, the loss within 1e-5, the update bit for bit -- every step restarted from the
    device's state so that Adam's sign sensitivity cannot compound."""
    spec, B = _critic_spec(), 256
    tr = _trainer(spec, B, 11)
    for s in range(5):
        batch = _minibatch(spec, B, 100 + s)
        state = _state(tr)
        tr.step(*[torch.from_numpy(np.asarray(a)).cuda() for a in batch])
        torch.cuda.synchronize()
        _check_step(tr, batch, state, False)


@pytest.mark.gpu
def test_batchnorm_steps_fold_each_network_once():
    spec, B = _critic_spec(True, szs=(200, 200, 200)), 64
    tr = _trainer(spec, B, 12)
    tr.critic.set_bn_stats(bn_ref.random_bn_stats(tr.critic.bn_stats, 1))
    tr.target.set_bn_stats(bn_ref.random_bn_stats(tr.target.bn_stats, 2))
    for s in range(2):
        batch = _minibatch(spec, B, 200 + s)
        state = _state(tr)
        tr.step(*[torch.from_numpy(np.asarray(a)).cuda() for a in batch])
        torch.cuda.synchronize()
        _check_step(tr, batch, state, True)


@pytest.mark.gpu
def test_captured_step_replays_equal_eager_steps():
    spec, B = _critic_spec(), 256
    eager, cap = _trainer(spec, B, 13), _trainer(spec, B, 13)
    batch = [torch.from_numpy(np.asarray(a)).cuda() for a in _minibatch(spec, B, 300)]
    losses = []
    for _ in range(3):
        losses.append(eager.step(*batch).clone())
    cap.step(*batch)                            # warm-up outside the graph (first-call allocations), then undo it
    torch.cuda.synchronize()
    fresh = _trainer(spec, B, 13)
    for dst, src in ((cap.opt.theta, fresh.opt.theta), (cap.opt.m, fresh.opt.m), (cap.opt.v, fresh.opt.v),
                     (cap.opt.step_count, fresh.opt.step_count), (cap.opt.arena, fresh.opt.arena),
                     (cap.follower.theta, fresh.follower.theta), (cap.follower.arena, fresh.follower.arena)):
        dst.copy_(src)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = cap.step(*batch)
    cap_losses = []
    for _ in range(3):
        g.replay()
        cap_losses.append(loss.clone())
    torch.cuda.synchronize()
    for a, b in ((cap.opt.theta, eager.opt.theta), (cap.opt.m, eager.opt.m), (cap.opt.v, eager.opt.v),
                 (cap.opt.step_count, eager.opt.step_count), (cap.follower.theta, eager.follower.theta),
                 (cap.opt.arena, eager.opt.arena), (cap.follower.arena, eager.follower.arena)):
        assert torch.equal(a, b)
    assert cap.t == 3
    for a, b in zip(cap_losses, losses):
        assert torch.equal(a, b)


def _raw_update_case(n, t):
    """theta, target, m, v, grad, a destination map in which parameter i has (i + 1) % 3 destinations scattered over an
    arena with spare cells, and proj ranges that straddle the quad boundary at 4 and the workgroup boundary at 1024"""
    rng = np.random.RandomState(1000 * n + t)
    theta = (1e-2 * rng.randn(n)).astype(np.float32)
    target = (theta + 1e-2 * rng.randn(n)).astype(np.float32)
    m = (1e-3 * rng.randn(n)).astype(np.float32)
    v = (1e-6 * rng.rand(n)).astype(np.float32)
    g = (1e-2 * rng.randn(n)).astype(np.float32)
    dest_off = np.concatenate([[0], np.cumsum((np.arange(n) + 1) % 3)]).astype(np.int32)
    arena_floats = int(dest_off[-1]) + 5
    dest = rng.permutation(arena_floats).astype(np.int32)           # the first dest_off[-1] are read
    proj = [(2, min(n, 7))] if n > 2 else [(0, n)]
    if n > 1024:
        proj.append((1022, n))
    return theta, target, m, v, g, dest_off, dest, arena_floats, proj


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_critic_update_without_decay_is_the_plain_update(n, t):
    """icnn_be_rl_critic_update with a decay mask of zeros (and a large l2norm wd that the mask must keep out) leaves
    theta, m, v, the arena and the step word as icnn_be_param_update does from the same state, bit for bit, and the
    target as tt - tau (tt - theta_old) in float32: one quad, a tail alone, a quad and a tail, and two workgroups."""
    lib = _lib.load()
    theta, target, m, v, g, dest_off, dest, arena_floats, proj = _raw_update_case(n, t)
    assert -(-n // 1024) == (2 if n == 1027 else 1)                 # workgroups of 256 threads x 4 parameters
    counts = np.diff(dest_off)
    assert set(counts.tolist()) == ({0, 1, 2} if n >= 3 else {1})
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()       # noqa: E731
    fill = np.full(arena_floats, -7.0, np.float32)
    grad, d_off, d_dest = dev(g), dev(dest_off), dev(dest)
    decay = torch.zeros(n + 3, dtype=torch.uint8, device="cuda")
    runs = []
    for critic in (False, True):
        s = dict(theta=dev(theta), m=dev(m), v=dev(v), arena=dev(fill), tt=dev(target), ta=dev(fill),
                 step=torch.tensor([t - 1, 0], dtype=torch.int32, device="cuda"))
        r = _lib.RlUpdateArgs()
        a = r.adam
        a.n, a.theta, a.m, a.v, a.grad = n, s["theta"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), grad.data_ptr()
        a.dest_off, a.dest, a.arena, a.arena_floats = d_off.data_ptr(), d_dest.data_ptr(), s["arena"].data_ptr(), arena_floats
        a.step, a.lr, a.beta1, a.beta2, a.eps, a.n_proj = s["step"].data_ptr(), 1e-2, 0.9, 0.999, 1e-8, len(proj)
        for i, (b, e) in enumerate(proj):
            a.proj_begin[i], a.proj_end[i] = b, e
        r.target_theta, r.target_arena, r.decay = s["tt"].data_ptr(), s["ta"].data_ptr(), decay.data_ptr()
        r.tau, r.l2norm, r.wd = TAU, 1.0, 10.0
        rc = lib.icnn_be_rl_critic_update(C.byref(r), None) if critic else lib.icnn_be_param_update(C.byref(a), None)
        assert rc == 0
        torch.cuda.synchronize()
        runs.append({k: x.cpu().numpy() for k, x in s.items()})
    plain, crit = runs
    for k in ("theta", "m", "v", "arena"):
        assert np.array_equal(_bits(crit[k]), _bits(plain[k])), k
    assert crit["step"].tolist() == plain["step"].tolist() == [t, 0]
    assert np.array_equal(_bits(plain["tt"]), _bits(target)) and np.array_equal(_bits(plain["ta"]), _bits(fill))
    tt_new = target - np.float32(TAU) * (target - theta)
    assert tt_new.dtype == np.float32 and np.array_equal(_bits(crit["tt"]), _bits(tt_new))
    owner = np.repeat(np.arange(n), counts)
    want_arena, want_ta = fill.copy(), fill.copy()
    want_arena[dest[:owner.size]] = plain["theta"][owner]
    want_ta[dest[:owner.size]] = tt_new[owner]
    assert np.array_equal(_bits(plain["arena"]), _bits(want_arena)) and np.array_equal(_bits(crit["ta"]), _bits(want_ta))
    # the update did something, and at the largest size the clamp acted inside a proj range and nowhere else
    assert not np.array_equal(_bits(plain["theta"]), _bits(theta))
    if n == 1027:
        inside = np.zeros(n, bool)
        for b, e in proj:
            inside[b:e] = True
        assert np.any(plain["theta"][inside] == 0) and np.all(plain["theta"][inside] >= 0) and np.any(plain["theta"][~inside] < 0)
