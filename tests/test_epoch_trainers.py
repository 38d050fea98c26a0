"""The epoch level of the training scripts on the device: train.GDTrainer's test phase against its hand
composition, train.BestKeeper inside a captured graph against a twin that keeps the best model on the host, and
checkpoint.save / load: a resumed run of every trainer and of the RL agent equals the uninterrupted one bit for bit, eagerly
and through a graph captured before the load, and a file that does not fit is refused with the object untouched."""
import ctypes as C
import dataclasses
import importlib.util
import os

import numpy as np
import pytest
import torch

from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = picnn.FCSpec(40, 16, (64, 32), batchnorm=True)
B, E, K = 8, 12, 5
GD_LR, GD_MU = 0.1, 0.3
# the seeds of the six batches of the keeper tests: at these the host twin keeps iterations 0, 1 and 3 and declines 2, 4 and 5
# in both modes (each test asserts at least two of either, so it cannot pass with a branch untaken)
KEEPER_SEED = {"max": 4, "min": 3}


def _fc_params(spec, seed):
    rng = np.random.RandomState(seed)
    params = picnn.init_params(spec, seed, "spread")
    for k in params:
        if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    return params


def _gd_trainer(seed, spec=SPEC, **kw):
    from icnn_amd import train
    args = dict(n_iter=K, lr=GD_LR, momentum=GD_MU, adam_lr=1e-2, bn_updates=1, f1=True, eval_batch=E)
    args.update(kw)
    return train.GDTrainer(picnn.FCModel(spec, _fc_params(spec, seed), "cuda"), B, **args)


def _fc_batch(spec, rows, seed):
    rng = np.random.RandomState(seed)
    x = rng.rand(rows, spec.n_features).astype(np.float32)
    t = (rng.rand(rows, spec.n_labels) < 0.35).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def _opt_state(opt):
    return [opt.theta, opt.m, opt.v, opt.step_count, opt.arena]


def _clones(tensors):
    torch.cuda.synchronize()
    return [t.clone() for t in tensors]


def _equal(a, b):
    torch.cuda.synchronize()
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and torch.equal(x, y), i


# ------------------------------------------------------------------------------------------------ the test phase


@pytest.mark.gpu
def test_evaluate_equals_the_hand_composition_and_touches_nothing():
    from icnn_amd import _lib, gd
    tr = _gd_trainer(3)
    lib, model, n = tr.model._lib, tr.model, SPEC.n_labels
    for i in range(2):                                  # two steps: the moving statistics have left their initial values
        tr.step(*_fc_batch(SPEC, B, 10 + i))
    step_results = [tr.loss, tr.grad, tr.y, tr.f1_tallies]
    state = _opt_state(tr.opt) + [model.bn_stats[k] for k in sorted(model.bn_stats)] + step_results
    before = _clones(state)
    xe, te = _fc_batch(SPEC, E, 20)
    loss = tr.evaluate(xe, te)
    assert loss is tr.eval_loss and loss.dtype == torch.float32 and loss.shape == ()
    _equal(_clones(state), before)
    assert all(a is b for a, b in zip(step_results, [tr.loss, tr.grad, tr.y, tr.f1_tallies]))
    # ---- the hand composition: context with the moving statistics, gd.solve, the feed with throw-away rows ----
    ctx = model.context(xe, bn="moving")
    assert torch.equal(ctx, tr.ctx_eval)
    assert not torch.equal(ctx, model.context(xe, bn="batch"))               # the mode matters on this batch
    y = gd.solve(model, ctx, 0.5, K, GD_LR, GD_MU)[0]
    coef = torch.zeros(K, dtype=torch.float64, device="cuda")
    v = torch.empty(E * K, n, dtype=torch.float64, device="cuda")
    c = torch.empty(E * K, dtype=torch.float64, device="cuda")
    off = torch.empty(E + 1, dtype=torch.int32, device="cuda")
    want_loss = torch.zeros((), dtype=torch.float32, device="cuda")
    want_tallies = torch.zeros(E, 3, dtype=torch.int32, device="cuda")
    work = torch.zeros((lib.icnn_be_gd_feed_work_bytes(E) + 7) // 8, dtype=torch.float64, device="cuda")
    _lib.check(lib.icnn_be_gd_feed(y.data_ptr(), te.data_ptr(), coef.data_ptr(), E, n, K, 1.0, v.data_ptr(), c.data_ptr(),
                                   off.data_ptr(), want_loss.data_ptr(), want_tallies.data_ptr(), work.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "icnn_be_gd_feed")
    torch.cuda.synchronize()
    assert torch.equal(tr.y_eval, y) and tr.y_eval.shape == (E, n)
    assert torch.equal(tr.eval_loss, want_loss) and float(want_loss) > 0
    assert torch.equal(tr.eval_f1_tallies, want_tallies) and int(want_tallies.sum()) > 0
    from icnn_amd import train
    assert tr.eval_macro_f1() == train.macro_f1(want_tallies)
    # ---- a captured evaluate replayed on a new batch equals the eager one ----
    xe2, te2 = _fc_batch(SPEC, E, 21)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.evaluate()
        y_out, loss_out = tr.y_eval.clone(), tr.eval_loss.clone()
    tr.x_eval.copy_(xe2)
    tr.t_eval.copy_(te2)
    g.replay()
    torch.cuda.synchronize()
    got = (y_out.clone(), loss_out.clone(), tr.eval_f1_tallies.clone())
    tr.evaluate(xe2, te2)
    torch.cuda.synchronize()
    assert torch.equal(got[0], tr.y_eval) and torch.equal(got[1], tr.eval_loss) and torch.equal(got[2], tr.eval_f1_tallies)
    assert not torch.equal(got[1], want_loss)
    _equal(_clones(state), before)


@pytest.mark.gpu
def test_evaluate_needs_eval_batch_and_a_model_without_batchnorm_ignores_eval_bn():
    tr = _gd_trainer(3, eval_batch=None)
    with pytest.raises(ValueError, match="eval_batch"):
        tr.evaluate(*_fc_batch(SPEC, E, 20))
    with pytest.raises(ValueError, match="eval_batch"):
        tr.eval_macro_f1()
    with pytest.raises(ValueError):
        _gd_trainer(3, eval_batch=0)
    with pytest.raises(ValueError):
        _gd_trainer(3, eval_bn="population")
    plain = dataclasses.replace(SPEC, batchnorm=False)
    xe, te = _fc_batch(plain, E, 20)
    a, b = _gd_trainer(4, plain, eval_bn="moving", f1=False), _gd_trainer(4, plain, eval_bn="batch", f1=False)
    assert torch.equal(a.evaluate(xe, te), b.evaluate(xe, te)) and torch.equal(a.y_eval, b.y_eval)
    assert a.eval_f1_tallies is None
    with pytest.raises(ValueError):
        a.eval_macro_f1()


# ------------------------------------------------------------------------------------------------ the keeper


def _keeper_batches(seed, spec=SPEC, rows=B, eval_rows=E):
    return [(_fc_batch(spec, rows, 1000 * seed + i), _fc_batch(spec, eval_rows, 1000 * seed + 100 + i)) for i in range(6)]


def host_max_cycle(seed):
    """the twin of the "max" case: six iterations of step, evaluate, train.macro_f1 on the host and a copy of host_params()
    when strictly better.  Returns (the F1 of every iteration, the iterations kept, the kept params, statistics, eval loss)"""
    from icnn_amd import train
    tw = _gd_trainer(5)
    best, f1s, kept, params, stats, loss = -np.inf, [], [], None, None, None
    for i, ((x, t), (xe, te)) in enumerate(_keeper_batches(seed)):
        tw.step(x, t)
        tw.evaluate(xe, te)
        f1 = train.macro_f1(tw.eval_f1_tallies)
        f1s.append(f1)
        if f1 > best:
            best, params, stats, loss = f1, tw.host_params(), tw.model.get_bn_stats(), tw.eval_loss.clone()
            kept.append(i)
    return f1s, kept, params, stats, loss


@pytest.mark.gpu
def test_best_keeper_in_a_graph_equals_the_host_twin():
    from icnn_amd import train
    seed = KEEPER_SEED["max"]
    f1s, kept, params, stats, kept_loss = host_max_cycle(seed)
    print("F1 per iteration", f1s, "kept", kept)
    assert len(kept) >= 2 and 6 - len(kept) >= 2, (f1s, kept)                # both branches taken, each at least twice
    tr = _gd_trainer(5)
    keeper = train.BestKeeper(tr, mode="max")
    assert keeper.best_value() == -np.inf and keeper.offers == 0 and keeper.kept == 0
    live = _opt_state(tr.opt) + [tr.model.flatten_bn_stats()]
    fresh = _clones(live)
    batches = _keeper_batches(seed)

    def cycle():
        tr.step()
        tr.evaluate()
        keeper.offer_macro_f1(tr.eval_f1_tallies)
    tr._put(tr.x, batches[0][0][0]), tr._put(tr.t, batches[0][0][1])
    tr._put(tr.x_eval, batches[0][1][0]), tr._put(tr.t_eval, batches[0][1][1])
    cycle()                                             # a warm-up outside the graph, then undone
    torch.cuda.synchronize()
    for dst, src in zip(live, fresh):
        dst.copy_(src)
    keeper.best.fill_(-np.inf)
    keeper.gate.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cycle()
    for (x, t), (xe, te) in batches:
        tr.x.copy_(x), tr.t.copy_(t), tr.x_eval.copy_(xe), tr.t_eval.copy_(te)
        g.replay()
    torch.cuda.synchronize()
    assert keeper.offers == 6 and keeper.kept == len(kept)
    assert abs(keeper.best_value() - max(f1s)) <= E * 2.0 ** -52
    got = keeper.host_params()
    assert list(got) == list(params)
    for k in params:
        assert np.array_equal(got[k], params[k]), k
    got_stats = keeper.bn_stats()
    assert sorted(got_stats) == sorted(stats) and len(stats) > 0
    for k in stats:
        assert np.array_equal(got_stats[k], stats[k]), k
    assert tr.t_steps == 6
    last = tr.host_params()
    assert any(not np.array_equal(last[k], params[k]) for k in params)       # the last iteration was not the kept one
    # ---- restore: the kept iteration's evaluation again, and m, v, the step count left alone ----
    mv = _clones([tr.opt.m, tr.opt.v, tr.opt.step_count])
    keeper.restore()
    xe, te = batches[kept[-1]][1]
    assert torch.equal(tr.evaluate(xe, te), kept_loss)
    _equal(_clones([tr.opt.m, tr.opt.v, tr.opt.step_count]), mv)
    assert torch.equal(tr.opt.arena, torch.from_numpy(tr.opt.map.scatter(tr.opt.theta.cpu().numpy())).cuda())


def _ficnn_trainer(seed, batch=16):
    from icnn_amd import ficnn
    spec = ficnn.synthetic_spec()
    params = ficnn.make_convex(ficnn.init_params(spec, seed))
    return ficnn.GDTrainer(ficnn.FICNNModel(spec, params), batch, n_iter=K, adam_lr=1e-2)


def _ficnn_batch(rows, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, (rows, 2)).astype(np.float32)
    t = (rng.rand(rows, 1) < 0.5).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def host_min_cycle(seed):
    """the twin of the "min" case: synthetic-cls's rule on the train loss, without its `bestMSE is None` clause"""
    tw = _ficnn_trainer(6)
    best, losses, kept, params = np.inf, [], [], None
    for i in range(6):
        loss = float(tw.step(*_ficnn_batch(16, 1000 * seed + i)).item())
        losses.append(loss)
        if loss < best:
            best, params = loss, tw.host_params()
            kept.append(i)
    return losses, kept, params


@pytest.mark.gpu
def test_best_keeper_min_mode_on_a_float32_loss_without_batchnorm():
    from icnn_amd import train
    seed = KEEPER_SEED["min"]
    losses, kept, params = host_min_cycle(seed)
    print("loss per iteration", losses, "kept", kept)
    assert len(kept) >= 2 and 6 - len(kept) >= 2, (losses, kept)
    tr = _ficnn_trainer(6)
    keeper = train.BestKeeper(tr, mode="min")
    assert keeper.bn is None and keeper.bn_stats() == {} and keeper.best_value() == np.inf
    live = _opt_state(tr.opt)
    fresh = _clones(live)

    def cycle():
        keeper.offer(tr.step())
    tr._put(tr.x, _ficnn_batch(16, 1000 * seed)[0]), tr._put(tr.t, _ficnn_batch(16, 1000 * seed)[1])
    cycle()
    torch.cuda.synchronize()
    for dst, src in zip(live, fresh):
        dst.copy_(src)
    keeper.best.fill_(np.inf)
    keeper.gate.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cycle()
    for i in range(6):
        x, t = _ficnn_batch(16, 1000 * seed + i)
        tr.x.copy_(x), tr.t.copy_(t)
        g.replay()
    torch.cuda.synchronize()
    assert keeper.offers == 6 and keeper.kept == len(kept)
    assert keeper.best_value() == min(losses)            # a float32 score widened to float64: exact
    got = keeper.host_params()
    for k in params:
        assert np.array_equal(got[k], params[k]), k
    keeper.restore()
    assert all(np.array_equal(v, params[k]) for k, v in tr.host_params().items())
    with pytest.raises(ValueError):
        keeper.offer(torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError):
        keeper.offer(torch.zeros(1, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        train.BestKeeper(tr, mode="best")
    with pytest.raises(TypeError):
        train.BestKeeper(object())


# ------------------------------------------------------------------------------------------------ resume


class _Case:
    """One trainer kind for the resume test: make(seed) builds the trainer and its keeper from weights seeded by `seed`,
    put(i) copies batch i into the trainer's buffers, run() is one iteration on what the buffers hold."""

    def __init__(self, kind, seed):
        from icnn_amd import ficnn, rl_train, train
        self.kind = kind
        if kind == "bundle":
            spec = picnn.FCSpec(20, 12, (24, 12), alpha=0.0, batchnorm=True, action_box=False)
            self.tr = tr = train.BundleTrainer(picnn.FCModel(spec, _fc_params(spec, seed), "cuda"), 9, n_iter=6, loss="xent",
                                               variant="pdipm", lr=1e-3, skip_on_error=True, eval_batch=7)
            self.keeper = train.BestKeeper(tr, mode="max", start=0.0)
            self.bufs = lambda i: [(tr.x, _fc_batch(spec, 9, 50 + i)[0]), (tr.true_y, _fc_batch(spec, 9, 50 + i)[1]),
                                   (tr.x_eval, _fc_batch(spec, 7, 80 + i)[0]), (tr.true_y_eval, _fc_batch(spec, 7, 80 + i)[1])]
            self.losses = lambda: [tr.loss, tr.eval_loss]

            def run():
                tr.step()
                tr.evaluate()
                self.keeper.offer_macro_f1(tr.eval_f1_tallies)
        elif kind == "gd":
            self.tr = tr = _gd_trainer(seed)
            self.keeper = train.BestKeeper(tr, mode="max")
            self.bufs = lambda i: [(tr.x, _fc_batch(SPEC, B, 50 + i)[0]), (tr.t, _fc_batch(SPEC, B, 50 + i)[1]),
                                   (tr.x_eval, _fc_batch(SPEC, E, 80 + i)[0]), (tr.t_eval, _fc_batch(SPEC, E, 80 + i)[1])]
            self.losses = lambda: [tr.loss, tr.eval_loss]

            def run():
                tr.step()
                tr.evaluate()
                self.keeper.offer_macro_f1(tr.eval_f1_tallies)
        elif kind == "conv":
            spec = picnn.ConvSpec(32, 32)
            self.tr = tr = train.ConvGDTrainer(picnn.ConvModel(spec, picnn.init_conv_params(spec, seed, "spread"), "cuda"), 3,
                                               n_iter=3, lr=0.01, momentum=0.9, y0=0.5, bn_updates=1)
            self.keeper = train.BestKeeper(tr, mode="min")

            def batch(i):
                rng = np.random.RandomState(50 + i)
                return (torch.from_numpy(rng.rand(3, 32, 32, 1).astype(np.float32)).cuda(),
                        torch.from_numpy(rng.rand(3, spec.n_labels).astype(np.float32)).cuda())
            self.bufs = lambda i: [(tr.x, batch(i)[0]), (tr.t, batch(i)[1])]
            self.losses = lambda: [tr.loss]

            def run():
                self.keeper.offer(tr.step())
        elif kind == "ficnn":
            self.tr = tr = _ficnn_trainer(seed)
            self.keeper = train.BestKeeper(tr, mode="min")
            self.bufs = lambda i: [(tr.x, _ficnn_batch(16, 50 + i)[0]), (tr.t, _ficnn_batch(16, 50 + i)[1])]
            self.losses = lambda: [tr.loss]

            def run():
                self.keeper.offer(tr.step())
        else:
            assert kind == "critic"
            spec = dataclasses.replace(picnn.halfcheetah_spec(), n_features=17, n_labels=6, action_box=False, batchnorm=True,
                                       szs=(6, 5))
            params = picnn.init_params(spec, seed, "spread", yu_bias=1.0, gate_bias=1.0)
            self.tr = tr = rl_train.CriticTrainer(picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda"), 4,
                                                  max_iter=50)
            tr.initialise()
            self.keeper = train.BestKeeper(tr, mode="min")

            def batch(i):
                rng = np.random.RandomState(50 + i)
                return [(tr.obs, rng.randn(4, 17).astype(np.float32)), (tr.act, rng.uniform(-1, 1, (4, 6))),
                        (tr.rew, rng.randn(4).astype(np.float32)), (tr.ob2, rng.randn(4, 17).astype(np.float32)),
                        (tr.term, (rng.rand(4) < 0.3).astype(np.uint8))]
            self.bufs = lambda i: [(dst, torch.from_numpy(np.ascontiguousarray(a)).cuda()) for dst, a in batch(i)]
            self.losses = lambda: [tr.loss]

            def run():
                self.keeper.offer(tr.step_buffers())
        self.run = run

    def put(self, i):
        for dst, src in self.bufs(i):
            dst.copy_(src.to(dst.dtype).reshape(dst.shape))

    def state(self):
        tr, kp = self.tr, self.keeper
        out = _opt_state(tr.opt) + [kp.best, kp.gate, kp.theta, kp.arena]
        models = [tr.critic, tr.target] if self.kind == "critic" else [tr.model]
        for m in models:
            if getattr(m, "has_bn", False):
                out += [m.bn_stats[k] for k in sorted(m.bn_stats)]
        if kp.bn is not None:
            out.append(kp.bn)
        if self.kind == "critic":
            out += [tr.follower.theta, tr.follower.arena]
        if self.kind == "bundle":
            out += [tr.skipped, tr._gate]
        return out


KINDS = ["bundle", "gd", "conv", "ficnn", "critic"]
_uninterrupted = {}


def _state_a(kind, tmp_path_factory):
    """3 steps, save, 3 more steps: the file, the final state and the three losses -- computed once per kind"""
    from icnn_amd import checkpoint
    if kind not in _uninterrupted:
        a = _Case(kind, 1)
        path = str(tmp_path_factory.mktemp("ck") / (kind + ".npz"))
        for i in range(3):
            a.put(i)
            a.run()
        checkpoint.save(path, a.tr, keeper=a.keeper)
        losses = []
        for i in range(3, 6):
            a.put(i)
            a.run()
            losses += _clones(a.losses())
        _uninterrupted[kind] = (path, _clones(a.state()), losses)
    return _uninterrupted[kind]


@pytest.mark.gpu
@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured_before_load"])
@pytest.mark.parametrize("kind", KINDS)
def test_resumed_run_equals_the_uninterrupted_one(kind, captured, tmp_path_factory):
    from icnn_amd import checkpoint
    path, want_state, want_losses = _state_a(kind, tmp_path_factory)
    b = _Case(kind, 2)                                  # other initial weights
    b.put(0)
    b.run()                                             # one step of its own: m, v, the step count, the statistics are not fresh
    torch.cuda.synchronize()
    assert not torch.equal(b.tr.opt.theta, want_state[0])
    g = None
    if captured:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            b.run()
    ptrs = [t.data_ptr() for t in b.state()]
    checkpoint.load(path, b.tr, keeper=b.keeper)
    assert ptrs == [t.data_ptr() for t in b.state()]    # no address moved
    losses = []
    for i in range(3, 6):
        b.put(i)
        if g is None:
            b.run()
        else:
            g.replay()
        losses += _clones(b.losses())
    _equal(_clones(b.state()), want_state)
    _equal(losses, want_losses)
    assert b.keeper.offers == 6
    assert all(bool(torch.isfinite(x)) for x in losses)


# ------------------------------------------------------------------------------------------------ the agent


def _point_mass():
    spec = importlib.util.spec_from_file_location("example_rl_agent", os.path.join(REPO, "examples", "rl_agent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PointMass


AGENT_SPEC = dataclasses.replace(picnn.halfcheetah_spec(), n_features=4, n_labels=2, action_box=False, batchnorm=False, szs=(5,))


def _agent(model_seed, seed, rmsize=8, **kw):
    from icnn_amd import rl_agent
    params = picnn.init_params(AGENT_SPEC, model_seed, "spread", yu_bias=1.0, gate_bias=1.0)
    return rl_agent.Agent(picnn.FCModel(AGENT_SPEC, params, "cuda"), picnn.FCModel(AGENT_SPEC, params, "cuda"), bsize=4,
                          warmup=4, iters=2, rmsize=rmsize, seed=seed, max_iter=50, **kw)


def _agent_state(agent):
    tr, mem = agent.trainer, agent.memory
    return _opt_state(tr.opt) + [tr.follower.theta, tr.follower.arena, mem.observations, mem.actions, mem.rewards,
                                 mem.terminals, mem.ctrl]


def _agent_run(agent, record, first, last, env=None, path=None, save_after=None, **save_kw):
    """environment steps first .. last of the 12-step cycle of tests/test_rl_agent.py (episodes of 5 and 7 steps): with
    `env` they are made and recorded, without they are replayed from `record` (the actions must come out the same)"""
    from icnn_amd import checkpoint
    out = []
    for step in range(first, last + 1):
        if env is not None:
            if step in (1, 6):
                env.horizon = 5 if step == 1 else 100
                agent.reset(env.reset())
            action = agent.act()
            obs2, rew, term = env.step(action)
            term = term or step == 12
            record[step] = (action.copy(), obs2, rew, term)
        else:
            action = agent.act()
            _, obs2, rew, term = record[step]
        agent.observe(rew, term, obs2)
        torch.cuda.synchronize()
        idx = agent.memory._idx[4].clone() if 4 in agent.memory._idx else None
        out.append((action.copy(), agent.loss.clone(), idx))
        if step == save_after:
            checkpoint.save(path, agent, **save_kw)
    return out


def _own_steps(agent, count):
    env = _point_mass()(4, 2, horizon=100, seed=5)
    agent.reset(env.reset())
    for _ in range(count):
        obs2, rew, _ = env.step(agent.act())
        agent.observe(rew, False, obs2)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
def test_agent_resumes_as_if_it_had_not_stopped(capture, tmp_path):
    from icnn_amd import checkpoint
    path, lean = str(tmp_path / "agent.npz"), str(tmp_path / "lean.npz")
    record = {}
    a = _agent(23, 9, capture=capture)
    env = _point_mass()(4, 2, horizon=5, seed=1)
    _agent_run(a, record, 1, 8, env=env, path=path, save_after=8)
    checkpoint.save(lean, a, memory=False)
    saved = _clones(_agent_state(a))
    want = _agent_run(a, record, 9, 12, env=env)
    assert a.t == 12 and (a.memory.n, a.memory.i) == (7, 4)
    b = _agent(24, 11, capture=capture)                 # other weights, other noise, another sampler
    _own_steps(b, 6)                                    # and a past of its own: trained eagerly once, then captured
    assert not torch.equal(b.trainer.opt.theta, saved[0]) and b.t == 6
    ptrs = [t.data_ptr() for t in _agent_state(b)]
    checkpoint.load(path, b)
    assert ptrs == [t.data_ptr() for t in _agent_state(b)]
    _equal(_clones(_agent_state(b)), saved)
    assert (b.t, b.memory.n, b.memory.i, b._trained) == (8, 7, 0, True)
    got = _agent_run(b, record, 9, 12)
    for (act_a, loss_a, idx_a), (act_b, loss_b, idx_b) in zip(want, got):
        assert np.array_equal(act_a, act_b) and torch.equal(loss_a, loss_b) and torch.equal(idx_a, idx_b)
    _equal(_clones(_agent_state(b)), _clones(_agent_state(a)))
    assert b.t == 12 and np.array_equal(a.noise, b.noise) and a.rng.randn() == b.rng.randn()
    b.memory.raise_on_error()
    # ---- memory=False: the reference's checkpoint; weights and optimiser state arrive, the memory is empty ----
    c = _agent(25, 12, capture=capture)
    c.reset(np.zeros(4, np.float32))
    c.act()
    c.observe(0.0, False, np.ones(4, np.float32))       # one transition of its own, which the load drops
    checkpoint.load(lean, c)
    _equal(_clones(_agent_state(c))[:7], saved[:7])
    assert (c.memory.n, c.memory.i, c.t) == (0, 0, 8) and not bool(c.memory.ctrl.any())
    assert c.memory.seed == 9 and c._graph is None


# ------------------------------------------------------------------------------------------------ refusals


def _refused(path, obj, keeper, field, state):
    from icnn_amd import checkpoint
    before = _clones(state)
    with pytest.raises(ValueError, match="^%s: " % field):         # the message names the field first
        checkpoint.load(path, obj, keeper=keeper)
    _equal(_clones(state), before)


@pytest.mark.gpu
def test_load_refuses_what_does_not_fit_and_leaves_the_object_alone(tmp_path):
    from icnn_amd import checkpoint, train
    p = lambda name: str(tmp_path / name)               # noqa: E731
    gd = _Case("gd", 1)
    gd.put(0)
    gd.run()
    checkpoint.save(p("gd_keeper.npz"), gd.tr, keeper=gd.keeper)
    checkpoint.save(p("gd.npz"), gd.tr)
    other = _gd_trainer(1, picnn.FCSpec(40, 16, (64, 48), batchnorm=True))
    other.step(*_fc_batch(SPEC, B, 50))
    checkpoint.save(p("other_spec.npz"), other)

    def trainer_state(tr):
        return [tr.opt.theta, tr.opt.m, tr.opt.v, tr.opt.step_count] + [tr.model.bn_stats[k] for k in sorted(tr.model.bn_stats)]
    # a GDTrainer's file into a BundleTrainer
    bundle = _Case("bundle", 2)
    bundle.put(0)
    bundle.run()
    _refused(p("gd.npz"), bundle.tr, None, "kind", trainer_state(bundle.tr))
    # a file of another spec
    fresh = _Case("gd", 2)
    fresh.put(1)
    fresh.run()
    state = trainer_state(fresh.tr) + [fresh.keeper.best, fresh.keeper.gate, fresh.keeper.theta, fresh.keeper.bn]
    _refused(p("other_spec.npz"), fresh.tr, None, "spec", state)
    # a keeper's file without a keeper, and a file without one given a keeper
    _refused(p("gd_keeper.npz"), fresh.tr, None, "keeper", state)
    _refused(p("gd.npz"), fresh.tr, fresh.keeper, "keeper", state)
    # a keeper of the other mode
    _refused(p("gd_keeper.npz"), fresh.tr, train.BestKeeper(fresh.tr, mode="min"), "keeper/mode", state)
    # an array of another shape inside an otherwise fitting file
    arrays = checkpoint.read_arrays(p("gd.npz"))
    arrays["m"] = arrays["m"][:-1]
    checkpoint.write_arrays(p("short.npz"), arrays)
    _refused(p("short.npz"), fresh.tr, None, "m", state)
    arrays = checkpoint.read_arrays(p("gd.npz"))
    arrays["theta"] = arrays["theta"].astype(np.float64)
    checkpoint.write_arrays(p("wide.npz"), arrays)
    _refused(p("wide.npz"), fresh.tr, None, "theta", state)
    # and the fitting files do load
    checkpoint.load(p("gd.npz"), fresh.tr)
    assert torch.equal(fresh.tr.opt.theta, gd.tr.opt.theta)
    # a file of another rmsize
    small = _agent(23, 9, rmsize=8)
    checkpoint.save(p("agent8.npz"), small)
    big = _agent(24, 10, rmsize=16)
    _refused(p("agent8.npz"), big, None, "rmsize", _agent_state(big))
    with pytest.raises(TypeError):
        checkpoint.save(p("x.npz"), object())
