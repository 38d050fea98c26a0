"""The bundle-entropy training step as one device step (icnn_amd.train.BundleTrainer, be_train_bundle.hip):
the feed plan against the host composition, the loss and F1 tallies against NumPy float64, the gradient over a padded feed
against the float64 references of tests/test_train_grad.py and tests/test_train_grad_conv.py (same bounds), what must be
bit-identical to the compact path, a row count of 0, the step against its own composition, graph capture, the error surface."""
import os
import re

import numpy as np
import pytest
import torch

import test_train_grad as tg
import test_train_grad_conv as tgc
import train_conv_ref
import train_ref
from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_feed_plan_work_bytes", "icnn_be_feed_plan", "icnn_be_feed_pad", "icnn_be_fc_surrogate_grad_dev",
               "icnn_be_conv_surrogate_grad_dev", "icnn_be_fc_context_bn_dev", "icnn_be_conv_context_bn_dev",
               "icnn_be_fc_surrogate_grad_dev_work_floats", "icnn_be_conv_surrogate_grad_dev_work_floats"]
CONV = picnn.ConvSpec()


# ------------------------------------------------------------------------------------------------ CPU


def test_new_exports_in_header_and_library():
    from icnn_amd import _lib
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()
    assert lib.icnn_be_feed_plan_work_bytes(128) >= 128 * 8 + 4


def test_macro_f1_on_hand_made_tallies():
    from icnn_amd import train
    # example 0: tp 2, fp 1, fn 1 -> 4/6; example 1: nothing positive anywhere -> 0; example 2: only misses -> 0;
    # example 3: perfect -> 1
    t = np.array([[2, 1, 1], [0, 0, 0], [0, 0, 3], [5, 0, 0]], np.int32)
    assert train.macro_f1(t) == pytest.approx((4.0 / 6.0 + 0.0 + 0.0 + 1.0) / 4.0, abs=1e-15)
    assert train.macro_f1(torch.from_numpy(t)) == train.macro_f1(t)
    assert train.macro_f1(np.zeros((3, 3), np.int32)) == 0.0
    # the per-example statement of util.macroF1 (sklearn's classes are the examples after its transpose)
    rng = np.random.RandomState(0)
    truth, pred = rng.rand(7, 11) < 0.3, rng.rand(7, 11) < 0.3
    truth[2] = False
    pred[2] = False
    tallies = np.stack([(truth & pred).sum(1), (~truth & pred).sum(1), (truth & ~pred).sum(1)], 1)
    f1 = []
    for j in range(7):
        tp, fp, fn = tallies[j]
        p = tp / (tp + fp) if tp + fp else 0.0
        r = tp / (tp + fn) if tp + fn else 0.0
        f1.append(2 * p * r / (p + r) if p + r else 0.0)
    assert train.macro_f1(tallies) == pytest.approx(np.mean(f1), abs=1e-15)


def test_trainer_rejects_bad_arguments_before_any_launch():
    from icnn_amd import ficnn, train
    fc = object.__new__(picnn.FCModel)              # never initialised: any use beyond isinstance would raise AttributeError
    conv = object.__new__(picnn.ConvModel)
    with pytest.raises(ValueError):
        train.BundleTrainer(fc, 8, loss="mse")
    with pytest.raises(ValueError):
        train.BundleTrainer(conv, 8, loss="xent")
    with pytest.raises(ValueError):
        train.BundleTrainer(fc, 8, loss="hinge")
    with pytest.raises(ValueError):
        train.BundleTrainer(fc, 0, loss="xent")
    with pytest.raises(ValueError):
        train.BundleTrainer(fc, 8, loss="xent", variant="rl")
    with pytest.raises(TypeError):
        train.BundleTrainer(object.__new__(ficnn.FICNNModel), 8, loss="mse")


# ------------------------------------------------------------------------------------------------ GPU helpers


def _bn_spec():
    return picnn.FCSpec(20, 12, (24, 12), alpha=0.0, batchnorm=True, action_box=False)


def _problem(kind):
    """(spec, params, Model, x, labels, B, n_iter, loss) of the four shapes"""
    if kind == "bibtex":             # the inputs of tests/test_train_grad.py::_bibtex_feed
        spec, B, n_iter = picnn.bibtex_spec(), 128, 10
        rng = np.random.RandomState(0)
        x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32)
        labels = (rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)
        return spec, picnn.init_params(spec, 0, "spread"), picnn.FCModel, x, labels, B, n_iter, "xent"
    if kind == "small":
        spec, B, n_iter = _bn_spec(), 9, 6
        rng = np.random.RandomState(5)
        params = picnn.init_params(spec, 5, "spread")
        for k in params:
            if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
                params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
        x = rng.rand(B, spec.n_features).astype(np.float32)
        labels = (rng.rand(B, spec.n_labels) < 0.3).astype(np.float64)
        return spec, params, picnn.FCModel, x, labels, B, n_iter, "xent"
    B, n_iter, seed = (70, 5, 70) if kind == "completion" else (6, 3, 8)
    rng = np.random.RandomState(seed)
    x = rng.rand(B, CONV.H, CONV.W, 1).astype(np.float32)
    labels = rng.rand(B, CONV.n_labels)
    return CONV, picnn.init_conv_params(CONV, seed, "spread"), picnn.ConvModel, x, labels, B, n_iter, "mse"


def _solve(kind, variant="dual", n_iter=None):
    """a model, its solve of the problem and the device inputs"""
    from icnn_amd import bundle_entropy
    spec, params, Model, x, labels, B, k, loss = _problem(kind)
    n_iter = k if n_iter is None else n_iter
    model = Model(spec, params, "cuda")
    xd = torch.from_numpy(x).cuda()
    solver = bundle_entropy.FusedSolver(model, B, n_iter, variant)
    res = solver.solve(model.context(xd), 0.5)
    t = torch.from_numpy(labels).cuda()
    return dict(spec=spec, params=params, model=model, x=x, xd=xd, labels=labels, t=t, B=B, n_iter=n_iter, loss=loss,
                solver=solver, res=res)


def _plan_and_feed(p, scale=1):
    from icnn_amd import train
    plan = train.FeedPlan(p["solver"].state, p["loss"]).run(p["t"])
    feed = train.PaddedFeed(p["solver"].state, scale).fill(plan, p["t"])
    return plan, feed


def _padded_grad(p, plan, feed, bn_updates=0, F_rows=None, flat=False):
    from icnn_amd import train
    return train.surrogate_grad(p["model"], p["xd"], (feed.y, feed.v, feed.c), row_offset=plan.row_offset, F_rows=F_rows,
                                bn_updates=bn_updates, rows_dev=plan.rows, flat=flat)


def _stats(model):
    return {k: v.clone() for k, v in model.bn_stats.items()}


# ------------------------------------------------------------------------------------------------ 1. the plan


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", [("bibtex", "dual"), ("bibtex", "pdipm"), ("small", "dual"), ("conv", "pdipm"),
                                          ("completion", "dual")])
def test_feed_plan_equals_host_composition(kind, variant):
    from icnn_amd import bundle_entropy
    p = _solve(kind, variant)
    res, st, B = p["res"], p["solver"].state, p["B"]
    plan, feed = _plan_and_feed(p)
    host = bundle_entropy.implicit_feed(res, p["labels"], p["loss"])
    torch.cuda.synchronize()
    cnt = st.count[:B].cpu().numpy().astype(np.int64)
    R = int(cnt.sum())
    assert np.array_equal(plan.row_offset.cpu().numpy(), np.concatenate([[0], np.cumsum(cnt)]))
    assert int(plan.rows.item()) == R == host.y.shape[0]
    assert feed.row_cap == B * st.T and R <= feed.row_cap
    for name in ("y", "v", "c", "sample"):
        assert np.array_equal(getattr(feed, name)[:R].cpu().numpy(), getattr(host, name).cpu().numpy()), name
    assert np.all(feed.v[R:].cpu().numpy() == 0) and np.all(feed.c[R:].cpu().numpy() == 0)
    assert np.all(np.isfinite(feed.y[R:].cpu().numpy()))
    pad_s = feed.sample[R:].cpu().numpy()
    assert np.all((pad_s >= 0) & (pad_s < B))
    assert int(plan.fg_evals.item()) == res.fg_evaluations()
    assert int(plan.status_or.item()) == int(np.bitwise_or.reduce(st.status[:B].cpu().numpy()))
    print("%s/%s: R = %d, R_cap = %d (ratio %.2f), fg evaluations %d" % (kind, variant, R, feed.row_cap, feed.row_cap / max(R, 1),
                                                                       int(plan.fg_evals.item())))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_fg_evaluations_when_all_finish_early_and_when_none_does(variant):
    from icnn_amd import bundle_entropy
    seen = set()
    # two iterations of the Bibtex batch finish nobody; thirty of the small model finish everybody
    for kind, n_iter in (("bibtex", 2), ("small", 30)):
        p = _solve(kind, variant, n_iter)
        st, B = p["solver"].state, p["B"]
        plan, _ = _plan_and_feed(p)
        torch.cuda.synchronize()
        fin = st.finished[:B].cpu().numpy().astype(bool)
        want = bundle_entropy.fg_evaluations(st.n_iters[:B].cpu().numpy(), n_iter, fin)
        assert int(plan.fg_evals.item()) == want == p["res"].fg_evaluations()
        if n_iter == 2:
            assert not fin.any() and want == 2             # nobody finishes in two iterations
            seen.add("none")
        else:
            assert fin.all() and want < n_iter             # everybody finished early: max(nIters) + 2
            seen.add("all")
    assert seen == {"none", "all"}


# ------------------------------------------------------------------------------------------------ 2. loss and tallies


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bibtex", "small", "conv", "completion"])
def test_loss_and_tallies_against_numpy_float64(kind):
    from icnn_amd import train
    p = _solve(kind)
    plan, _ = _plan_and_feed(p)
    torch.cuda.synchronize()
    y, t = p["res"].y.cpu().numpy(), p["labels"]
    if p["loss"] == "xent":          # crossEntr, multi-label-cls/icnn_ebundle.py:419-421
        with np.errstate(all="ignore"):
            want = -np.sum((t * np.log(y))[y > 0]) - np.sum(((1. - t) * np.log(1. - y))[y < 1])
    else:                            # mse, completion/icnn_ebundle.py:476-477
        want = np.mean(np.square(255. * (y - t)))
    got = float(plan.loss.item())
    print("%s: loss %.15e, NumPy %.15e, relative difference %.2e" % (kind, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-11 * abs(want)
    if p["loss"] != "xent":
        assert plan.f1_tallies is None
        return
    pred, truth = (y >= 0.5).astype(int), t.astype(int)           # util.macroF1
    tallies = np.stack([(pred & truth).sum(1), (pred & (1 - truth)).sum(1), ((1 - pred) & truth).sum(1)], 1)
    assert np.array_equal(plan.f1_tallies.cpu().numpy(), tallies)
    f1 = [2. * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0 for tp, fp, fn in tallies]
    assert train.macro_f1(plan.f1_tallies) == pytest.approx(np.mean(f1), abs=1e-15)


# ------------------------------------------------------------------------------------------------ 3. the gradient


def _pad_rows(prob, n, extra):
    """rows of a hand-made problem behind `extra` rows of padding, with the device row count"""
    R = len(prob["samp"])
    y = np.concatenate([prob["y"], np.full((extra, n), 0.5)])
    v = np.concatenate([prob["v"], np.zeros((extra, n))])
    c = np.concatenate([prob["c"], np.zeros(extra)])
    rows = torch.tensor([R], dtype=torch.int32, device="cuda")
    return tuple(torch.from_numpy(a).cuda() for a in (y, v, c)), rows


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1000])
def test_small_fc_padded_gradient_matches_float64(seed):
    from icnn_amd import train
    spec = tg._small_spec(True, 0.0, False)
    prob = tg._small_problem(spec, seed, True)
    model = picnn.FCModel(spec, prob["params"], "cuda")
    R = len(prob["samp"])
    off = torch.from_numpy(tg._offsets(prob["counts"])).cuda()
    for cap in (R + 5, 2 * (R + 5)):
        rows3, rows_dev = _pad_rows(prob, spec.n_labels, cap - R)
        F = torch.full((cap,), float("nan"), dtype=torch.float32, device="cuda")
        g = train.surrogate_grad(model, torch.from_numpy(prob["x"]), rows3, row_offset=off, F_rows=F, rows_dev=rows_dev)
        torch.cuda.synchronize()
        for k, ref in prob["g64"].items():
            got = g[k].double().cpu().numpy()
            err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
            assert err <= 1e-4 * scale + 1e-7, (cap, k, err, scale)
        Fd = F.double().cpu().numpy()
        assert np.max(np.abs(Fd[:R] - prob["F64"])) <= 1e-5 * np.max(np.abs(prob["F64"]))
        assert np.all(Fd[R:] == 0)


@pytest.mark.gpu
def test_bibtex_padded_gradient_matches_float64():
    p = _solve("bibtex")
    spec, params, x = p["spec"], p["params"], p["x"]
    g64 = None
    for scale in (1, 2):
        plan, feed = _plan_and_feed(p, scale)
        g = _padded_grad(p, plan, feed)
        torch.cuda.synchronize()
        R = int(plan.rows.item())
        assert 128 < R < feed.row_cap
        samp = feed.sample[:R].cpu().numpy()
        yr, vr, cr = (getattr(feed, k)[:R].cpu().numpy() for k in ("y", "v", "c"))
        if g64 is None:
            g64, _, _ = train_ref.surrogate_grad64(spec, params, x[samp], yr, vr, cr)
        ratios = {k: float(np.linalg.norm(g[k].double().cpu().numpy() - ref) / max(np.linalg.norm(ref), 1e-300))
                  for k, ref in g64.items()}
        L = len(spec.szs)               # z{L}_u/*: against the size of their cancelling terms (tests/test_train_grad.py)
        c32 = cr.astype(np.float32).astype(np.float64)
        u_last = train_ref.last_u(spec, params, x[samp])
        terms = {"z%d_u/b" % L: np.sum(np.abs(c32)), "z%d_u/W" % L: np.sum(np.abs(c32) * np.linalg.norm(u_last, axis=1))}
        for k, size in terms.items():
            err = float(np.linalg.norm(g[k].double().cpu().numpy() - g64[k]))
            print("R_cap x%d  %-12s |g - g64|_F = %.2e against cancelling terms of size %.2e" % (scale, k, err, size))
            assert err <= 1e-5 * size, (scale, k, err, size)
            del ratios[k]
        print("R = %d, R_cap = %d, worst Frobenius ratio %.2e" % (R, feed.row_cap, max(ratios.values())))
        bad = {k: r for k, r in ratios.items() if not r <= 1e-3}
        assert not bad, (scale, bad)


@pytest.mark.gpu
def test_small_conv_padded_gradient_matches_float64():
    from icnn_amd import train
    prob = tgc._small_problem("spread", 21, True)
    model = picnn.ConvModel(CONV, prob["params"])
    R = len(prob["samp"])
    x = torch.from_numpy(prob["x"]).cuda()
    off = torch.from_numpy(tgc._offsets(prob["counts"])).cuda()
    for cap in (R + 3, 2 * (R + 3)):
        rows3, rows_dev = _pad_rows(prob, CONV.n_labels, cap - R)
        F = torch.full((cap,), float("nan"), dtype=torch.float32, device="cuda")
        g = train.surrogate_grad(model, x, rows3, row_offset=off, F_rows=F, rows_dev=rows_dev)
        torch.cuda.synchronize()
        bad = []
        for name, ref in prob["g64"].items():
            got = g[name].double().cpu().numpy().reshape(ref.shape)
            if name in tgc.ZERO_VARS:
                if not (np.all(got == 0) and np.all(ref == 0)):
                    bad.append(name)
                continue
            scale, err = np.max(np.abs(ref)), np.max(np.abs(got - ref))
            if not (scale > 0 and err <= (tgc.BN_TOL if name.startswith("u") else 1e-4) * scale):
                bad.append((name, err / scale if scale > 0 else err))
        assert not bad, (cap, bad)
        Fd = F.double().cpu().numpy()
        assert np.max(np.abs(Fd[:R] - prob["F64"])) <= 1e-4 * np.max(np.abs(prob["F64"]))
        assert np.all(Fd[R:] == 0)


@pytest.mark.gpu
def test_completion_padded_gradient_matches_float64():
    """B = 70 / nIter 5 / mse with the bounds of tests/test_train_grad_conv.py::test_end_to_end_reference_training_batch"""
    p = _solve("completion")
    g64 = gabs = None
    for scale in (1, 2):
        plan, feed = _plan_and_feed(p, scale)
        g = _padded_grad(p, plan, feed)
        torch.cuda.synchronize()
        R = int(plan.rows.item())
        assert p["B"] < R <= p["B"] * p["n_iter"]
        samp = feed.sample[:R].cpu().numpy()
        yr, vr, cr = (getattr(feed, k)[:R].cpu().numpy() for k in ("y", "v", "c"))
        if g64 is None:
            g64, _, _ = train_conv_ref.surrogate_grad64(CONV, p["params"], p["x"][samp], yr, vr, cr)
            gabs, _, _ = train_conv_ref.surrogate_grad64(CONV, p["params"], p["x"][samp], yr, None, np.abs(cr))
        for name, ref in g64.items():
            got = g[name].double().cpu().numpy().reshape(ref.shape)
            if name in tgc.ZERO_VARS:
                assert np.all(got == 0), name
                continue
            err, size = np.linalg.norm(got - ref), np.linalg.norm(gabs[name])
            if name in tgc.CANCEL_CANDIDATES and np.linalg.norm(ref) <= 1e-6 * size:
                assert err <= 1e-4 * size, (scale, name, err, size)
                continue
            assert err <= 1e-4 * np.linalg.norm(ref), (scale, name, err, np.linalg.norm(ref))
        print("completion: R = %d, R_cap = %d" % (R, feed.row_cap))


# ------------------------------------------------------------------------------------------------ 4. bit-identical


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "conv"])
def test_bn_stats_and_F_rows_equal_the_compact_call(kind):
    from icnn_amd import bundle_entropy, train
    p = _solve(kind)
    q = _solve(kind)                                          # the twin: same weights, its own moving statistics
    plan, feed = _plan_and_feed(p, 2)
    host = bundle_entropy.implicit_feed(q["res"], q["labels"], q["loss"])
    R = host.y.shape[0]
    Fp = torch.full((feed.row_cap,), float("nan"), dtype=torch.float32, device="cuda")
    Fc = torch.empty(R, dtype=torch.float32, device="cuda")
    before = _stats(p["model"])
    _padded_grad(p, plan, feed, bn_updates=1, F_rows=Fp)
    train.surrogate_grad(q["model"], q["xd"], host, F_rows=Fc, bn_updates=1)
    torch.cuda.synchronize()
    assert int(plan.rows.item()) == R and R < feed.row_cap
    assert torch.equal(Fp[:R], Fc) and bool((Fp[R:] == 0).all())
    assert any(not torch.equal(before[k], p["model"].bn_stats[k]) for k in before)       # the fold happened
    for k, v in q["model"].bn_stats.items():
        assert torch.equal(p["model"].bn_stats[k], v), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "conv"])
@pytest.mark.parametrize("k", [0, 1, 7])
def test_context_folds_with_a_device_count_equal_the_host_count(kind, k):
    spec, params, Model, x, _, _, _, _ = _problem(kind)
    a, b = Model(spec, params, "cuda"), Model(spec, params, "cuda")
    xd = torch.from_numpy(x).cuda()
    k_dev = torch.tensor([k], dtype=torch.int32, device="cuda")
    ca = a.context(xd, bn_updates=k_dev)
    cb = b.context(xd, bn_updates=k)
    torch.cuda.synchronize()
    assert torch.equal(ca, cb)
    fresh = Model(spec, params, "cuda").bn_stats
    for name, v in b.bn_stats.items():
        assert torch.equal(a.bn_stats[name], v), name
        assert torch.equal(v, fresh[name]) == (k == 0), name


# ------------------------------------------------------------------------------------------------ 5. a count of 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["small", "conv"])
def test_a_true_row_count_of_zero(kind):
    p = _solve(kind)
    p["solver"].state.count.zero_()
    plan, feed = _plan_and_feed(p)
    before = _stats(p["model"])
    g = _padded_grad(p, plan, feed, bn_updates=1, flat=True)
    torch.cuda.synchronize()
    assert int(plan.rows.item()) == 0 and int(plan.row_offset.abs().max().item()) == 0
    assert bool((g == 0).all()) and not bool(torch.isnan(g).any())
    for k, v in before.items():
        assert torch.equal(p["model"].bn_stats[k], v), k


# ------------------------------------------------------------------------------------------------ 6, 7, 9. the step


class _ByHand:
    """BundleTrainer.step chained from the new pieces on a model of its own"""

    def __init__(self, kind, variant, lr):
        from icnn_amd import bundle_entropy, train
        spec, params, Model, x, labels, B, n_iter, loss = _problem(kind)
        self.model = Model(spec, params, "cuda")
        self.opt = train.DeviceAdam(self.model, lr=lr)
        self.solver = bundle_entropy.FusedSolver(self.model, B, n_iter, variant)
        self.plan = train.FeedPlan(self.solver.state, loss)
        self.feed = train.PaddedFeed(self.solver.state)
        self.x, self.t = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
        self.bn = Model is picnn.ConvModel or bool(spec.batchnorm)

    def step(self):
        from icnn_amd import train
        ctx = self.model.context(self.x)
        self.solver.solve(ctx, 0.5)
        self.plan.run(self.t)
        if self.bn:
            self.model.context(self.x, bn_updates=self.plan.fg_evals)
        self.feed.fill(self.plan, self.t)
        g = train.surrogate_grad(self.model, self.x, (self.feed.y, self.feed.v, self.feed.c), row_offset=self.plan.row_offset,
                                 bn_updates=1, flat=True, rows_dev=self.plan.rows)
        self.opt.step(g)
        return self.plan.loss


def _trainer(kind, variant, lr=1e-3):
    from icnn_amd import train
    spec, params, Model, x, labels, B, n_iter, loss = _problem(kind)
    model = Model(spec, params, "cuda")
    tr = train.BundleTrainer(model, B, n_iter=n_iter, loss=loss, variant=variant, lr=lr)
    return tr, torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()


def _same_state(tr, opt, model, loss, rows):
    assert torch.equal(tr.opt.theta, opt.theta)
    assert torch.equal(tr.opt.m, opt.m) and torch.equal(tr.opt.v, opt.v)
    assert torch.equal(tr.opt.arena, opt.arena)
    assert torch.equal(tr.opt.step_count, opt.step_count)
    for k, v in model.bn_stats.items():
        assert torch.equal(tr.model.bn_stats[k], v), k
    assert torch.equal(tr.loss, loss) and torch.equal(tr.rows, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", [("small", "dual"), ("small", "pdipm"), ("bibtex", "pdipm"), ("conv", "dual"),
                                          ("completion", "pdipm")])
def test_step_is_its_own_composition(kind, variant):
    tr, x, t = _trainer(kind, variant)
    hand = _ByHand(kind, variant, 1e-3)
    theta0 = tr.opt.theta.clone()
    for i in range(2):
        loss = tr.step(x, t) if i == 0 else tr.step(None, None)
        hand.step()
    torch.cuda.synchronize()
    assert loss is tr.loss and loss.dtype == torch.float64 and np.isfinite(float(loss.item()))
    assert not torch.equal(tr.opt.theta, theta0) and tr.t_steps == 2
    assert int(tr.rows.item()) > 0 and bool(torch.isfinite(tr.grad).all())
    _same_state(tr, hand.opt, hand.model, hand.plan.loss, hand.plan.rows)
    tr.raise_on_error()
    if kind in ("small", "bibtex"):
        assert 0.0 <= tr.macro_f1() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", [("bibtex", "pdipm"), ("bibtex", "dual"), ("small", "pdipm"), ("completion", "pdipm")])
def test_step_is_graph_capturable(kind, variant):
    """capture fails on any host wait inside step; three replays equal three eager steps of a twin, bit for bit"""
    tr, x, t = _trainer(kind, variant)
    twin, _, _ = _trainer(kind, variant)
    # the warm-up step on a side stream counts for both: the twin takes it eagerly too
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.step(x, t)
    torch.cuda.current_stream().wait_stream(s)
    twin.step(x, t)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.step(None, None)
    torch.cuda.synchronize()
    assert tr.t_steps == 1                       # capturing ran nothing
    for _ in range(3):
        graph.replay()
        twin.step(None, None)
    torch.cuda.synchronize()
    assert tr.t_steps == 4
    _same_state(tr, twin.opt, twin.model, twin.loss, twin.rows)


# ------------------------------------------------------------------------------------------------ 8. errors


@pytest.mark.gpu
def test_raise_on_error_maps_the_status_or():
    from icnn_amd import _lib
    tr, x, t = _trainer("small", "pdipm")
    tr.step(x, t)
    torch.cuda.synchronize()
    tr.raise_on_error()                                   # a clean solve raises nothing
    st = tr.solver.state
    for bit, exc in ((_lib.ST_SINGULAR, np.linalg.LinAlgError), (_lib.ST_NONFINITE, FloatingPointError),
                     (_lib.ST_UNFINISHED, RuntimeError), (_lib.ST_OVERFLOW, MemoryError)):
        st.status.zero_()
        st.status[3] = bit                                # the status word of one sample, written by hand
        tr.plan.run(tr.true_y)
        torch.cuda.synchronize()
        assert int(tr.status_or.item()) == bit
        with pytest.raises(exc):
            tr.raise_on_error()
