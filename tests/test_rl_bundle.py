"""The ICNN agent on the bundle-entropy inner optimiser: icnn_be_rl_bundle_solve -- the persistent rows solve
with the action and its value out of the same launch --, picnn.FCModel.boxed(), rl_bundle.BundleActionSolver,
rl_train.CriticTrainer(opt="bundle_entropy"), rl_agent.Agent(opt="bundle_entropy") and the checkpoint's opt field.

CPU: the export and what it refuses, the argument checks of the host classes, and the screens of the seeds on the oracle alone.
GPU: the new entry against the three-step composition bit for bit (array_equal, nothing exempt), the solver and five
teacher-forced training steps against tests/rl_bundle_ref.py, capture, the agent and its checkpoint."""
import ctypes as C
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

import bn_ref
import rl_bundle_ref as R
import rl_train_ref as ref
from icnn_amd import _lib, checkpoint, picnn, rl_agent, rl_bundle, rl_train, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, TAU, DISCOUNT, L2NORM, WD = 1e-3, 0.01, 0.99, 1e-4, 1e-3
ENTRY = "icnn_be_rl_bundle_solve"
EINVAL, ELIMIT = -1, -2

# (n, B, nIter) -> seeds.  B = 257: two samples per workgroup and a last workgroup of one; B = 1021: four and a partial last
# workgroup (256 CUs); nIter 5, 7 / 8 and 15: the three register forms of the narrow-row dual step; n = 17: the wave-per-sample
# step; nIter = 16: the 32-slot form.  Weights with the y-path shrunk to a tenth (rl_bundle_ref.params_for): the stall rule
# then stops part of a batch early.  The seeds of a case hold, between them, a sample that stalls before the last round and
# one that runs every round (test_case_seeds_hold_an_early_stall_and_a_full_run); at B = 1 that takes two seeds, and the
# first one's only workgroup leaves the round loop through its break.
CASES = {(1, 1, 5): (0, 1), (6, 1, 5): (0, 1), (6, 257, 5): (0,), (6, 1021, 5): (0,), (16, 5, 7): (0,), (16, 5, 8): (0,),
         (6, 3, 15): (4,), (17, 3, 5): (0,), (6, 3, 16): (4,)}
Y_SCALE = 0.1
# (n, B, nIter, seed) of the comparisons with the oracle: full-size y-path weights, on which the oracle meets no singular
# Newton system (test_oracle_seeds_are_clean), so no sample is exempt
ORACLE_CASES = [(6, 16, 5, 0), (6, 16, 5, 1), (16, 5, 7, 0), (17, 3, 5, 0)]
STEP_SEED = {False: 31, True: 32}            # the weights of the teacher-forced steps, without and with BatchNorm


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ CPU


def test_export_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    assert re.search(r"ICNN_BE_API\s+int\s+%s\s*\(" % ENTRY, header)
    assert ENTRY in _lib.EXPORTS and hasattr(lib, ENTRY)
    assert lib.icnn_be_rl_bundle_solve.argtypes[:5] == lib.icnn_be_solve_fc.argtypes[:5]
    assert lib.icnn_be_rl_bundle_solve.argtypes[5:] == [C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.icnn_be_abi_version() == 12


def _dummy_call(lib, model_kw=None, state_kw=None, **kw):
    """a call that is valid but for what the keywords change; the pointers are never dereferenced"""
    spec = dataclasses.replace(R.spec_for(6), action_box=True)
    m = _lib.FcModel()
    m.n, m.n_layers, m.alpha, m.action_box, m.ctx_width, m.wpack = 6, spec.n_layers, 0.01, 1, spec.ctx_width, 4096
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    s = _lib.State()
    s.batch, s.n, s.slots, s.iters, s.cut_dtype, s.variant, s.flags = 4, 6, 5, 0, _lib.CUT_F32, _lib.VARIANT["rl"], 0
    for i, name in enumerate(("y", "G", "h", "ys", "lam", "active", "count", "n_iters", "finished", "status", "newton_iters",
                              "t_next", "phase", "skip_fg", "pending", "park", "fvals")):
        setattr(s, name, 8192 + 256 * i)
    for k, v in (model_kw or {}).items():
        setattr(m, k, v)
    for k, v in (state_kw or {}).items():
        setattr(s, k, v)
    a = dict(model=C.byref(m), ctx=64, st=C.byref(s), f_work=128, g_work=192, y0=0.5, act=256, q=320)
    a.update(kw)
    return lib.icnn_be_rl_bundle_solve(a["model"], a["ctx"], a["st"], a["f_work"], a["g_work"], a["y0"], a["act"], a["q"], None)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    for kw in (dict(model=None), dict(ctx=None), dict(st=None), dict(f_work=None), dict(g_work=None), dict(act=None),
               dict(y0=float("nan")), dict(y0=float("inf")), dict(y0=-float("inf")),
               dict(model_kw=dict(action_box=0)), dict(model_kw=dict(wpack=None)), dict(model_kw=dict(n=5)),
               dict(state_kw=dict(variant=_lib.VARIANT["dual"])), dict(state_kw=dict(variant=_lib.VARIANT["pdipm"])),
               dict(state_kw=dict(cut_dtype=_lib.CUT_F64)), dict(state_kw=dict(y=None)), dict(state_kw=dict(slots=0))):
        assert _dummy_call(lib, **kw) == EINVAL, kw
    assert _dummy_call(lib, state_kw=dict(batch=0)) == 0                       # nothing to solve, nothing launched


def test_host_classes_check_their_arguments():
    for cls in (rl_agent.Agent, lambda c, t, **kw: rl_train.CriticTrainer(c, t, 4, **kw)):
        for bad in ("x", "Adam", "", None):
            with pytest.raises(RuntimeError, match="^Unrecognized ICNN optimizer: %s$" % bad):
                cls(None, None, opt=bad)
    assert rl_train.OPTS == ("adam", "bundle_entropy")
    plain = types.SimpleNamespace(spec=R.spec_for(6))
    boxed = types.SimpleNamespace(spec=dataclasses.replace(R.spec_for(6), action_box=True))
    other = types.SimpleNamespace(spec=R.spec_for(5))
    for n_iter in (0, -1, _lib.MAX_ITERS + 1):
        with pytest.raises(ValueError, match="n_iter"):
            rl_train.CriticTrainer(plain, plain, 4, opt="bundle_entropy", n_iter=n_iter)
    with pytest.raises(ValueError, match="one spec"):
        rl_train.CriticTrainer(plain, other, 4, opt="bundle_entropy")
    with pytest.raises(ValueError, match="action_box=False"):
        rl_train.CriticTrainer(boxed, boxed, 4, opt="bundle_entropy")
    with pytest.raises(ValueError, match="tau"):
        rl_train.CriticTrainer(plain, plain, 4, opt="bundle_entropy", tau=1.5)


_SOLVES = {}


def _oracle(n, B, T, seed, y_scale):
    """the oracle's solve of a case, computed once and shared (read-only) by the tests"""
    key = (n, B, T, seed, y_scale)
    if key not in _SOLVES:
        spec, params, obs, ctx = R.problem(n, B, seed, y_scale=y_scale)
        _SOLVES[key] = (spec, params, obs, ctx, R.solve(spec, params, ctx, T))
    return _SOLVES[key]


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "n%d_B%d_T%d" % c)
def test_case_seeds_hold_an_early_stall_and_a_full_run(case):
    n, B, T = case
    early = full = 0
    for seed in CASES[case]:
        s = _oracle(n, B, T, seed, Y_SCALE)[4]
        early += int((s.stalled & (s.stopped_at < T - 1)).sum())
        full += int((s.stopped_at == T - 1).sum())
        if B == 1 and seed == CASES[case][0]:
            assert s.stalled[0] and s.stopped_at[0] < T - 1               # its workgroup leaves the loop through the break
    assert early > 0 and full > 0, (early, full)


def test_cases_reach_the_plans_and_forms_they_claim():
    for (n, B, T) in CASES:
        spec = dataclasses.replace(R.spec_for(n), action_box=True)
        m, s = _plan_descriptors(spec, B, T)
        path, per_wg, _, rounds = _lib.solve_plan(m, s, 256)
        assert path == "ROWS" and rounds == T and per_wg == -(-B // 256), (n, B, T)
    m, s = _plan_descriptors(dataclasses.replace(R.spec_for(6), action_box=True), 1025, 5)
    assert _lib.solve_plan(m, s, 256)[0] != "ROWS" and _lib.solve_plan(m, s, 4)[0] != "ROWS"


def _plan_descriptors(spec, B, T):
    m = _lib.FcModel()
    m.n, m.n_layers, m.alpha, m.action_box, m.ctx_width = spec.n_labels, spec.n_layers, spec.alpha, 1, spec.ctx_width
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    s = _lib.State()
    s.batch, s.n, s.slots, s.iters = B, spec.n_labels, min(T, _lib.MAX_SLOTS), 0
    s.cut_dtype, s.variant = _lib.CUT_F32, _lib.VARIANT["rl"]
    return m, s


def test_oracle_seeds_are_clean():
    for n, B, T, seed in ORACLE_CASES:
        assert B <= 16 and not _oracle(n, B, T, seed, 1.0)[4].singular, (n, B, T, seed)


# ------------------------------------------------------------------------------------------------ GPU: bit identity


def _state_host(st):
    """what a solve leaves in a BundleState: the per-sample words whole, lam and the cuts on the active slots"""
    B = st.B
    cnt = st.count[:B].cpu().numpy()
    act = st.active.cpu().numpy()
    lam, G, h, ys = st.lam.cpu().numpy(), st.G.cpu().numpy(), st.h.cpu().numpy(), st.ys.cpu().numpy()
    out = dict(y=st.y.cpu().numpy(), count=cnt, n_iters=st.n_iters[:B].cpu().numpy(), status=st.status[:B].cpu().numpy(),
               finished=st.finished[:B].cpu().numpy())
    rows = [(u, s) for u in range(B) for s in act[u, :cnt[u]]]
    out["active"] = np.array(rows, np.int64).reshape(-1, 2)
    out["lam"] = np.array([lam[u, i] for u in range(B) for i in range(cnt[u])])
    for name, a in (("G", G), ("h", h), ("ys", ys)):
        out[name] = np.array([a[u, s] for u, s in rows])
    return out


def _solve_both(model, ctx, B, T):
    """the entry and the composition on one model and context: (entry's result, composition's result) on the host"""
    outs = []
    for entry in (True, False):
        solver = rl_bundle.BundleActionSolver(model, B, T, entry=entry)
        solver.act.fill_(float("nan"))
        solver.q.fill_(float("nan"))
        res = solver.solve(ctx)
        torch.cuda.synchronize()
        host = _state_host(res.state)
        host["act"], host["q"] = res.act.cpu().numpy(), res.q.cpu().numpy()
        outs.append((host, solver.used_entry))
    return outs


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k       # (array_equal: a NaN on either side fails)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "n%d_B%d_T%d" % c)
def test_entry_equals_the_three_step_composition_bit_for_bit(case):
    n, B, T = case
    for seed in CASES[case]:
        spec, params, obs, ctx = R.problem(n, B, seed, y_scale=Y_SCALE)
        model = picnn.FCModel(spec, params, "cuda")
        (one, used_one), (three, used_three) = _solve_both(model, torch.from_numpy(ctx).cuda(), B, T)
        assert used_one and not used_three
        _assert_same(one, three)
        assert np.array_equal(one["act"], 2.0 * one["y"] - 1.0) and np.all(np.abs(one["act"]) <= 1.0)
        assert one["q"].dtype == np.float32 and np.all(np.isfinite(one["q"]))


@pytest.mark.gpu
def test_outside_the_rows_plan_the_entry_refuses_and_the_solver_composes():
    n, B, T = 6, 1025, 5
    spec, params, obs, ctx = R.problem(n, B, 0, y_scale=Y_SCALE)
    model = picnn.FCModel(spec, params, "cuda")
    ctx_d = torch.from_numpy(ctx).cuda()
    solver = rl_bundle.BundleActionSolver(model, B, T)
    assert _lib.solve_plan(solver.model.c_model, solver.state.c_state, 4)[0] != "ROWS"
    assert _lib.solve_plan(solver.model.c_model, solver.state.c_state, 0)[0] != "ROWS"          # this device's CUs
    rc = solver.lib.icnn_be_rl_bundle_solve(C.byref(solver.model.c_model), ctx_d.data_ptr(), C.byref(solver.state.c_state),
                                            solver.f_work.data_ptr(), solver.g_work.data_ptr(), 0.5, solver.act.data_ptr(),
                                            solver.q.data_ptr(), solver.state.stream())
    assert rc == ELIMIT
    (one, used_one), (three, used_three) = _solve_both(model, ctx_d, B, T)
    assert not used_one and not used_three
    _assert_same(one, three)
    boxed = picnn.FCModel(dataclasses.replace(spec, action_box=True), params, "cuda")
    f, _ = boxed.fg(ctx_d, torch.from_numpy(one["y"]).cuda())
    assert np.array_equal(one["q"], f.cpu().numpy()) and np.array_equal(one["act"], 2.0 * one["y"] - 1.0)


def _trainer(spec, B, seed, opt="bundle_entropy", tau=TAU, n_iter=5, models=None):
    params = R.params_for(spec, seed)
    critic, target = models or (picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda"))
    tr = rl_train.CriticTrainer(critic, target, B, lr=LR, tau=tau, discount=DISCOUNT, l2norm=L2NORM, wd=WD, opt=opt, n_iter=n_iter)
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


def _dev(batch):
    return [torch.from_numpy(np.asarray(a)).cuda() for a in batch]


def _trainer_state(tr):
    return [tr.opt.theta, tr.opt.m, tr.opt.v, tr.opt.step_count, tr.opt.arena, tr.follower.theta, tr.follower.arena]


@pytest.mark.gpu
@pytest.mark.parametrize("batchnorm", [False, True], ids=["plain", "bn"])
def test_boxed_view_follows_the_attached_model(batchnorm):
    spec, B = R.spec_for(6, batchnorm), 8
    params = R.params_for(spec, 41)
    critic, target = picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda")
    views = critic.boxed(), target.boxed()                 # taken BEFORE the trainer moves the weights into its arenas
    assert views[0].spec.action_box and not critic.spec.action_box and views[0].boxed() is views[0]
    tr = _trainer(spec, B, 41, models=(critic, target))
    for s in range(2):
        tr.step(*_dev(_minibatch(spec, B, 400 + s)))
    torch.cuda.synchronize()
    obs, _, _, _, _ = _minibatch(spec, B, 402)
    y = torch.from_numpy(np.random.RandomState(5).rand(B, spec.n_labels)).cuda()
    for view, model, is_target in ((views[0], critic, False), (views[1], target, True)):
        assert view._optimizer is model._optimizer is not None and view.c_model.wpack == model.c_model.wpack
        assert view.c_model.action_box == 1 and model.c_model.action_box == 0
        fresh = picnn.FCModel(view.spec, tr.host_params(target=is_target), "cuda")
        if batchnorm:
            fresh.set_bn_stats(model.get_bn_stats())
        kw = dict(bn="moving") if batchnorm else {}
        ctx = fresh.context(torch.from_numpy(obs), **kw)
        assert torch.equal(view.context(torch.from_numpy(obs), **kw), ctx)
        f, g = view.fg(ctx, y)
        f_want, g_want = fresh.fg(ctx, y)
        f_plain, _ = model.fg(ctx, y)
        assert torch.equal(f, f_want) and torch.equal(g, g_want) and not torch.equal(f, f_plain)
    with pytest.raises(RuntimeError, match="boxed"):
        views[0].repack(params)


@pytest.mark.gpu
@pytest.mark.parametrize("batchnorm", [False, True], ids=["plain", "bn"])
def test_step_run_twice_equals_itself(batchnorm):
    spec, B = R.spec_for(6, batchnorm), 16
    a, b = _trainer(spec, B, 42), _trainer(spec, B, 42)
    before = a.opt.theta.clone()
    for s in range(2):
        batch = _dev(_minibatch(spec, B, 500 + s))
        la, lb = a.step(*batch).clone(), b.step(*batch).clone()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
        assert torch.equal(a.act2, b.act2) and torch.equal(a.q2_src, b.q2_src) and a.act2.dtype == torch.float64
    for x, y in zip(_trainer_state(a), _trainer_state(b)):
        assert torch.equal(x, y)
    assert a.t == 2 and not torch.equal(before, a.opt.theta) and a.solver.used_entry


@pytest.mark.gpu
def test_captured_step_replays_equal_eager_steps():
    spec, B = R.spec_for(6), 16
    eager, cap = _trainer(spec, B, 43), _trainer(spec, B, 43)
    batch = _dev(_minibatch(spec, B, 600))
    losses = [eager.step(*batch).clone() for _ in range(3)]
    cap.step(*batch)                            # warm-up outside the graph (first-call allocations), then undo it
    torch.cuda.synchronize()
    fresh = _trainer(spec, B, 43)
    for dst, src in zip(_trainer_state(cap), _trainer_state(fresh)):
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
    for a, b in zip(_trainer_state(cap), _trainer_state(eager)):
        assert torch.equal(a, b)
    assert cap.t == 3 and torch.equal(cap.act2, eager.act2)
    for a, b in zip(cap_losses, losses):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_step_without_decay_and_tau_one_has_the_update_tests_bits():
    """a decay mask of zeros and tau = 1: theta, m, v come out as tests/rl_train_ref.critic_update forms them from the fed
    gradient (the expectation of tests/test_rl_train.py's update tests), and the target as the critic's theta before the step"""
    spec, B = R.spec_for(6), 16
    tr = _trainer(spec, B, 44, tau=1.0)
    tr.decay.zero_()
    theta, theta_t, m, v = (t.cpu().numpy() for t in (tr.opt.theta, tr.follower.theta, tr.opt.m, tr.opt.v))
    assert np.array_equal(_bits(theta), _bits(theta_t))
    tr.step(*_dev(_minibatch(spec, B, 700)))
    torch.cuda.synchronize()
    mask = np.zeros(tr.opt.n, np.uint8)
    th_r, tt_r, m_r, v_r = ref.critic_update(theta, theta_t, m, v, tr.grad.cpu().numpy(), 1, mask, tr.opt.map.proj, LR, 1.0,
                                             L2NORM, WD)
    for got, want in ((tr.opt.theta, th_r), (tr.follower.theta, tt_r), (tr.opt.m, m_r), (tr.opt.v, v_r)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(tr.follower.theta.cpu().numpy()), _bits(theta))
    assert not np.array_equal(_bits(tr.opt.theta.cpu().numpy()), _bits(theta))
    assert np.array_equal(_bits(tr.opt.arena.cpu().numpy()), _bits(tr.opt.map.scatter(th_r)))
    assert np.array_equal(_bits(tr.follower.arena.cpu().numpy()), _bits(tr.opt.map.scatter(tt_r)))


# ------------------------------------------------------------------------------------------------ GPU: against the restatement


@pytest.mark.gpu
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "n%d_B%d_T%d_s%d" % c)
def test_solver_matches_the_chain_order_oracle(case):
    """y within 1e-6 of the oracle (the bound of test_fused_rl_matches_chain_order_oracle for clean samples; every sample is
    clean here) with identical counts and n_iters; act and q follow from y exactly"""
    n, B, T, seed = case
    spec, params, obs, ctx, s = _oracle(n, B, T, seed, 1.0)
    assert not s.singular
    model = picnn.FCModel(spec, params, "cuda")
    res = rl_bundle.BundleActionSolver(model, B, T).solve(torch.from_numpy(ctx).cuda())
    torch.cuda.synchronize()
    y = res.y.cpu().numpy()
    dy = np.max(np.abs(y - s.y))
    print("n=%d B=%d nIter=%d seed=%d: max|dy| = %.3e, status %s" % (n, B, T, seed, dy, res.state.status[:B].cpu().tolist()))
    assert dy <= 1e-6
    assert np.array_equal(res.state.count[:B].cpu().numpy(), s.counts)
    assert np.array_equal(res.state.n_iters[:B].cpu().numpy(), s.n_iters)
    assert np.array_equal(res.act.cpu().numpy(), 2.0 * y - 1.0)
    chain = R.picnn_oracle.make_fg_chain(params, ctx, list(spec.szs), spec.alpha, True)
    assert np.array_equal(res.q.cpu().numpy(), chain(y)[0])


def _state(tr):
    return (tr.opt.theta.cpu().numpy(), tr.follower.theta.cpu().numpy(), tr.opt.m.cpu().numpy(), tr.opt.v.cpu().numpy(),
            tr.t, tr.critic.get_bn_stats(), tr.target.get_bn_stats())


def _check_step(tr, batch, state, bn):
    """one device step against tests/rl_bundle_ref.py, teacher-forced from `state` (the device's weights before it): the
    checks and tolerances of tests/test_rl_train.py's _check_step, with the inner optimiser's own bound (y within 1e-6,
    identical counts and n_iters) where that one has the inner Adam's"""
    spec, B = tr.spec, tr.batch
    obs, act, rew, ob2, term = batch
    theta, theta_t, m, v, t, stats_c, stats_t = state
    pc = {k: a.numpy() for k, a in train.unpack_grad(spec, torch.from_numpy(theta)).items()}
    pt = {k: a.numpy() for k, a in train.unpack_grad(spec, torch.from_numpy(theta_t)).items()}
    fresh = picnn.FCModel(spec, pt, "cuda")
    if bn:
        fresh.set_bn_stats(stats_t)
    ctx2 = (fresh.context(torch.from_numpy(ob2), bn="moving") if bn else fresh.context(torch.from_numpy(ob2))).cpu().numpy()
    s = R.solve(spec, pt, ctx2, tr.n_iter)
    assert not s.singular
    st = tr.solver.state
    dy = np.max(np.abs(tr.solver.y.cpu().numpy() - s.y))
    print("step %d: max|dy| = %.3e" % (t, dy))
    assert dy <= 1e-6
    assert np.array_equal(st.count[:B].cpu().numpy(), s.counts) and np.array_equal(st.n_iters[:B].cpu().numpy(), s.n_iters)
    act2 = tr.act2.cpu().numpy()
    assert np.array_equal(act2, 2.0 * tr.solver.y.cpu().numpy() - 1.0)
    x64 = torch.as_tensor(obs.astype(np.float64))
    th64 = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in pc.items()}
    E = ref.train_ref.energy(spec, th64, x64, torch.as_tensor(act))[0].numpy().astype(np.float32)
    q2 = None
    if bn:
        tt64 = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in pt.items()}
        a2 = torch.as_tensor(act2.astype(np.float32).astype(np.float64))
        q2 = ref.train_ref.energy(spec, tt64, torch.as_tensor(ob2.astype(np.float64)), a2)[0].numpy().astype(np.float32)
    else:
        assert np.max(np.abs(tr.q2_src.cpu().numpy() - s.q)) <= 1e-6
    mask = rl_train.decay_mask(spec)
    td, c, want = R.td_and_loss(s, E, batch, theta, mask, DISCOUNT, L2NORM, WD, q2)
    want = float(want)
    assert abs(float(tr.loss.item()) - want) <= 1e-5 * abs(want)
    g64, _, _ = ref.train_ref.surrogate_grad64(spec, pc, obs, act, None, c)
    got = train.unpack_grad(spec, tr.grad.cpu())
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
    if bn:                                       # each network's moving statistics fold once per step
        _, bs_c = bn_ref.fc_context64(spec, pc, obs)
        _, bs_t = bn_ref.fc_context64(spec, pt, ob2)
        for model, start, bs in ((tr.critic, stats_c, bs_c), (tr.target, stats_t, bs_t)):
            want_s = bn_ref.fold32(start, bs, 1)
            for k, w in want_s.items():
                assert np.allclose(model.get_bn_stats()[k], w, rtol=1e-5, atol=1e-6), k


@pytest.mark.gpu
@pytest.mark.parametrize("batchnorm", [False, True], ids=["plain", "bn"])
def test_five_steps_against_the_restatement_teacher_forced(batchnorm):
    spec, B = R.spec_for(6, batchnorm), 16
    tr = _trainer(spec, B, STEP_SEED[batchnorm])
    if batchnorm:
        tr.critic.set_bn_stats(bn_ref.random_bn_stats(tr.critic.bn_stats, 1))
        tr.target.set_bn_stats(bn_ref.random_bn_stats(tr.target.bn_stats, 2))
    for s in range(5):
        batch = _minibatch(spec, B, 800 + s)
        state = _state(tr)
        tr.step(*_dev(batch))
        torch.cuda.synchronize()
        _check_step(tr, batch, state, batchnorm)


# ------------------------------------------------------------------------------------------------ GPU: the agent

AGENT_SPEC = R.spec_for(2, dimO=4, szs=(6, 5))


def _agent(model_seed, seed, **kw):
    params = R.params_for(AGENT_SPEC, model_seed)
    kw.setdefault("opt", "bundle_entropy")
    return rl_agent.Agent(picnn.FCModel(AGENT_SPEC, params, "cuda"), picnn.FCModel(AGENT_SPEC, params, "cuda"), bsize=4,
                          warmup=4, iters=2, rmsize=8, seed=seed, max_iter=50, **kw)


def _environment(obs, action, step):
    """a deterministic toy transition: (obs2, rew, term)"""
    obs2 = np.tanh(0.9 * obs + 0.3 * np.resize(action, 4) + 0.05 * np.sin(step + np.arange(4))).astype(np.float32)
    return obs2, float(-np.sum(obs2 ** 2)), step % 5 == 4


def _run(agent, first, last, start=None):
    """environment steps first .. last: (action, loss) of each"""
    out = []
    if start is not None:
        agent.reset(start)
    for step in range(first, last + 1):
        action = agent.act()
        obs2, rew, term = _environment(np.asarray(agent.observation, np.float32), action, step)
        agent.observe(rew, term, obs2)
        torch.cuda.synchronize()
        out.append((action.copy(), agent.loss.clone()))
    return out


OBS0 = np.array([0.3, -0.2, 0.1, 0.05], np.float32)


@pytest.mark.gpu
def test_agent_act_is_the_solvers_action():
    agent = _agent(51, 10)
    agent.reset(OBS0)
    ctx = agent.critic.context(torch.from_numpy(OBS0[None]))
    res = rl_bundle.BundleActionSolver(agent.critic, 1, 5).solve(ctx)
    want = (2.0 * res.y - 1.0).cpu().numpy()[0]
    quiet = agent.act(test=True)
    assert quiet.shape == (2,) and quiet.dtype == np.float64 and np.array_equal(quiet, want) and np.all(np.abs(quiet) <= 1)
    assert not agent.noise.any()
    rng, noise = np.random.RandomState(10), np.zeros(2)
    noise -= 0.15 * noise - 0.1 * rng.randn(2)
    assert np.array_equal(agent.act(), np.clip(want + noise, -1, 1))


@pytest.mark.gpu
def test_captured_agent_leaves_the_eager_agents_weights():
    eager, cap = _agent(52, 11, capture=False), _agent(52, 11, capture=True)
    a, b = _run(eager, 1, 8, OBS0), _run(cap, 1, 8, OBS0)               # four warm-up observes, four that train
    assert cap._graph is not None and eager._graph is None and eager.trainer.t == cap.trainer.t == 8
    for (act_a, loss_a), (act_b, loss_b) in zip(a, b):
        assert np.array_equal(act_a, act_b) and torch.equal(loss_a, loss_b)
    for x, y in zip(_trainer_state(eager.trainer), _trainer_state(cap.trainer)):
        assert torch.equal(x, y)
    eager.memory.raise_on_error()


@pytest.mark.gpu
def test_checkpoint_round_trips_an_agent_and_refuses_the_other_optimiser(tmp_path):
    path, adam_path = str(tmp_path / "bundle.npz"), str(tmp_path / "adam.npz")
    a = _agent(53, 12)
    _run(a, 1, 7, OBS0)
    checkpoint.save(path, a)
    arrays = checkpoint.read_arrays(path)
    assert str(arrays["opt"]) == "bundle_entropy" and int(arrays["n_iter"]) == 5
    want = _run(a, 8, 10)
    b = _agent(54, 13)
    _run(b, 1, 6, OBS0)
    checkpoint.load(path, b)
    got = _run(b, 8, 10)
    for (act_a, loss_a), (act_b, loss_b) in zip(want, got):
        assert np.array_equal(act_a, act_b) and torch.equal(loss_a, loss_b)
    for x, y in zip(_trainer_state(a.trainer), _trainer_state(b.trainer)):
        assert torch.equal(x, y)
    # a file of an adam agent, and one from before the file carried `opt`, are adam files
    c = _agent(53, 12, opt="adam")
    _run(c, 1, 5, OBS0)
    checkpoint.save(adam_path, c)
    assert str(checkpoint.read_arrays(adam_path)["opt"]) == "adam"
    before = [t.clone() for t in _trainer_state(b.trainer)]
    with pytest.raises(ValueError, match="^opt: "):
        checkpoint.load(adam_path, b)
    with pytest.raises(ValueError, match="^opt: "):
        checkpoint.load(path, c)
    old = {k: v for k, v in checkpoint.read_arrays(adam_path).items() if k not in ("opt", "n_iter")}
    checkpoint.write_arrays(str(tmp_path / "old.npz"), old)
    with pytest.raises(ValueError, match="^opt: "):
        checkpoint.load(str(tmp_path / "old.npz"), b)
    for x, y in zip(_trainer_state(b.trainer), before):
        assert torch.equal(x, y)
    checkpoint.load(str(tmp_path / "old.npz"), c)                       # ... and loads into an adam agent
    other = _agent(53, 12, n_iter=7)
    with pytest.raises(ValueError, match="^n_iter: "):
        checkpoint.load(path, other)
