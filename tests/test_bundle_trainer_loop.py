"""What the bundle-entropy scripts do around one training iteration, on train.BundleTrainer: the start point
y0, the skip of a step on a solver error (skip_on_error) and the test phase (evaluate).  The shapes are those of
tests/test_bundle_trainer.py ("small": FCSpec(20, 12, (24, 12), batchnorm) at B = 9 / nIter 6; "conv": the default ConvSpec
at B = 6 / nIter 3).  Every comparison is between two orders of the same launches, or between a launch and its ungated form:
torch.equal, no tolerance.  A solver error is produced by writing a status word by hand between the two halves of a step;
one test (test_a_nan_in_the_input_skips_the_step_end_to_end) feeds the step a NaN instead and lets the solve set the bit."""
import inspect

import numpy as np
import pytest
import torch

from icnn_amd import _lib, picnn

CONV = picnn.ConvSpec()
CASES = [("small", "dual"), ("small", "pdipm"), ("conv", "pdipm")]
E_OF = {"small": 7, "conv": 4}            # eval batches: both differ from the training batch


# ------------------------------------------------------------------------------------------------ CPU


def test_trainer_has_the_new_arguments_with_their_defaults():
    from icnn_amd import train
    sig = inspect.signature(train.BundleTrainer.__init__).parameters
    assert [sig[k].default for k in ("y0", "eval_batch", "eval_bn", "skip_on_error")] == [0.5, None, None, False]
    for name in ("set_y0", "evaluate", "eval_macro_f1", "_infer", "_learn"):
        assert callable(getattr(train.BundleTrainer, name)), name
    assert "go" in inspect.signature(train.DeviceAdam.step).parameters


def test_trainer_rejects_a_bad_test_phase_before_any_launch():
    from icnn_amd import train
    fc = object.__new__(picnn.FCModel)              # never initialised: any use beyond isinstance would raise AttributeError
    conv = object.__new__(picnn.ConvModel)
    for bad in (0, -2):
        with pytest.raises(ValueError):
            train.BundleTrainer(fc, 8, loss="xent", eval_batch=bad)
        with pytest.raises(ValueError):
            train.BundleTrainer(conv, 8, loss="mse", eval_batch=bad)
    with pytest.raises(ValueError):
        train.BundleTrainer(fc, 8, loss="xent", eval_batch=4, eval_bn="population")


# ------------------------------------------------------------------------------------------------ GPU helpers


def _problem(kind):
    """(spec, params, Model, x, labels, B, n_iter, loss): the "small" and "conv" shapes of tests/test_bundle_trainer.py"""
    if kind == "small":
        spec, B, n_iter = picnn.FCSpec(20, 12, (24, 12), alpha=0.0, batchnorm=True, action_box=False), 9, 6
        rng = np.random.RandomState(5)
        params = picnn.init_params(spec, 5, "spread")
        for k in params:
            if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
                params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
        x = rng.rand(B, spec.n_features).astype(np.float32)
        labels = (rng.rand(B, spec.n_labels) < 0.3).astype(np.float64)
        return spec, params, picnn.FCModel, x, labels, B, n_iter, "xent"
    B, n_iter, seed = 6, 3, 8
    rng = np.random.RandomState(seed)
    x = rng.rand(B, CONV.H, CONV.W, 1).astype(np.float32)
    labels = rng.rand(B, CONV.n_labels)
    return CONV, picnn.init_conv_params(CONV, seed, "spread"), picnn.ConvModel, x, labels, B, n_iter, "mse"


def _eval_batch(kind):
    """E samples of a test split that the training batch never saw"""
    spec, _, _, _, _, _, _, loss = _problem(kind)
    E, rng = E_OF[kind], np.random.RandomState(77)
    if kind == "small":
        x = rng.rand(E, spec.n_features).astype(np.float32)
        t = (rng.rand(E, spec.n_labels) < 0.3).astype(np.float64)
    else:
        x = rng.rand(E, CONV.H, CONV.W, 1).astype(np.float32)
        t = rng.rand(E, CONV.n_labels)
    return torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def _trainer(kind, variant, **kw):
    from icnn_amd import train
    spec, params, Model, x, labels, B, n_iter, loss = _problem(kind)
    tr = train.BundleTrainer(Model(spec, params, "cuda"), B, n_iter=n_iter, loss=loss, variant=variant, lr=1e-3, **kw)
    return tr, torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()


def _row(kind, seed=3):
    """a start row drawn in (0.2, 0.8): the stand-in of the completion script's meanY"""
    n = _problem(kind)[0].n_labels
    return 0.2 + 0.6 * np.random.RandomState(seed).rand(n)


class _ByHand:
    """BundleTrainer.step chained from its pieces on a model of its own, the solve started from a tensor"""

    def __init__(self, kind, variant, y0):
        from icnn_amd import bundle_entropy, train
        spec, params, Model, x, labels, B, n_iter, loss = _problem(kind)
        self.model = Model(spec, params, "cuda")
        self.opt = train.DeviceAdam(self.model, lr=1e-3)
        self.solver = bundle_entropy.FusedSolver(self.model, B, n_iter, variant)
        self.plan = train.FeedPlan(self.solver.state, loss)
        self.feed = train.PaddedFeed(self.solver.state)
        self.x, self.t = torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda()
        self.y0 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(y0, (B, spec.n_labels)))).cuda()

    def step(self):
        from icnn_amd import train
        ctx = self.model.context(self.x)
        self.solver.solve(ctx, self.y0)
        self.plan.run(self.t)
        self.model.context(self.x, bn_updates=self.plan.fg_evals)
        self.feed.fill(self.plan, self.t)
        self.grad = train.surrogate_grad(self.model, self.x, (self.feed.y, self.feed.v, self.feed.c),
                                         row_offset=self.plan.row_offset, bn_updates=1, flat=True, rows_dev=self.plan.rows)
        self.opt.step(self.grad)


def _state(tr):
    """clones of everything a skipped step and evaluate() must leave alone"""
    out = {"theta": tr.opt.theta, "m": tr.opt.m, "v": tr.opt.v, "arena": tr.opt.arena, "step_count": tr.opt.step_count}
    out.update({"bn:" + k: v for k, v in tr.model.bn_stats.items()})
    return {k: v.clone() for k, v in out.items()}


def _same_state(tr, want, results=None):
    got = _state(tr)
    assert set(got) == set(want) and len(got) >= 7            # five tensors of the optimiser, two or more statistics
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    if results is not None:
        assert torch.equal(tr.loss, results.loss) and torch.equal(tr.rows, results.rows)


def _bad_word(tr, bit, sample=3):
    """one status bit in one sample's status word, written by hand, and the plan run again on it"""
    tr.solver.state.status[sample] = bit
    tr.plan.run(tr.true_y)


ERRORS = {_lib.ST_SINGULAR: np.linalg.LinAlgError, _lib.ST_NONFINITE: FloatingPointError, _lib.ST_UNFINISHED: RuntimeError,
          _lib.ST_OVERFLOW: MemoryError}


# ------------------------------------------------------------------------------------------------ 1. the start point


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", CASES)
def test_step_from_a_start_row_is_its_own_composition(kind, variant):
    row = _row(kind)
    B = _problem(kind)[5]
    hand = _ByHand(kind, variant, row)
    by_row, x, t = _trainer(kind, variant, y0=row)
    by_array, _, _ = _trainer(kind, variant)                 # built with the default, replaced before the first step
    by_array.set_y0(np.tile(row, (B, 1)))
    for i in range(2):
        hand.step()
        for tr in (by_row, by_array):
            tr.step(x, t) if i == 0 else tr.step(None, None)
    torch.cuda.synchronize()
    for tr in (by_row, by_array):
        assert torch.equal(tr.y0, hand.y0) and tr.y0.dtype == torch.float64
        assert torch.equal(tr.solver.y, hand.solver.y)       # y*
        assert torch.equal(tr.grad, hand.grad) and bool(torch.isfinite(tr.grad).all())
        _same_state(tr, _state(hand), hand.plan)
        assert tr.t_steps == 2 and int(tr.rows.item()) > 0
    half, _, _ = _trainer(kind, variant)
    half.step(x, t)
    half.step(None, None)
    assert not torch.equal(half.solver.y, by_row.solver.y)   # the start point is in effect


@pytest.mark.gpu
def test_set_y0_shapes():
    tr, x, t = _trainer("conv", "pdipm", eval_batch=E_OF["conv"])
    B, n, E = tr.batch, CONV.n_labels, E_OF["conv"]
    row = _row("conv")
    tr.set_y0(row.reshape(CONV.H, CONV.W, 1))                # an image
    assert torch.equal(tr.y0.cpu(), torch.from_numpy(np.tile(row, (B, 1))))
    assert torch.equal(tr.y0_eval.cpu(), torch.from_numpy(np.tile(row, (E, 1))))
    tr.set_y0(row[None])                                     # [1, n]
    assert torch.equal(tr.y0[B - 1].cpu(), torch.from_numpy(row))
    for bad in (np.zeros(n + 1), np.zeros((B + 1, n)), np.zeros((2, 3, 5)), np.zeros((B, n + 1))):
        with pytest.raises(ValueError):
            tr.set_y0(bad)
    with pytest.raises(ValueError):                          # a per-sample start cannot serve E != B
        tr.set_y0(np.zeros((B, n)))
    with pytest.raises(ValueError):
        _trainer("conv", "pdipm", eval_batch=E, y0=np.zeros((B, CONV.H, CONV.W, 1)))
    same, _, _ = _trainer("small", "dual", eval_batch=9, y0=np.full((9, 12), 0.25))        # E == B: served
    assert torch.equal(same.y0_eval, same.y0)
    fc, _, _ = _trainer("small", "dual")
    with pytest.raises(ValueError):
        fc.set_y0(np.zeros(11))
    fc.set_y0(0.25)                                          # a scalar keeps the solver's fill
    assert fc.y0 is None


# ------------------------------------------------------------------------------------------------ 2. clean steps


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", CASES)
def test_clean_steps_with_the_gate_equal_steps_without_it(kind, variant):
    tr, x, t = _trainer(kind, variant, skip_on_error=True)
    twin, _, _ = _trainer(kind, variant)
    assert twin.went is None and twin.skipped is None
    for i in range(3):
        for one in (tr, twin):
            one.step(x, t) if i == 0 else one.step(None, None)
    torch.cuda.synchronize()
    _same_state(tr, _state(twin), twin)
    assert tr.t_steps == 3 == twin.t_steps
    assert int(tr.went.item()) == 1 and int(tr.skipped.item()) == 0
    assert tr.went.dtype == torch.int32 and tr.skipped.dtype == torch.int32 and tr.went.is_cuda
    tr.raise_on_error()


# ------------------------------------------------------------------------------------------------ 3. skipped steps


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant,bit", [("small", "dual", _lib.ST_SINGULAR), ("small", "pdipm", _lib.ST_NONFINITE),
                                              ("small", "pdipm", _lib.ST_UNFINISHED), ("conv", "pdipm", _lib.ST_OVERFLOW)])
def test_a_skipped_step_changes_nothing_and_the_next_is_the_twins(kind, variant, bit):
    tr, x, t = _trainer(kind, variant, skip_on_error=True)
    twin, _, _ = _trainer(kind, variant)
    tr.step(x, t)
    twin.step(x, t)
    before = _state(tr)
    _same_state(twin, before)
    tr._infer()
    _bad_word(tr, bit)
    tr._learn()
    torch.cuda.synchronize()
    _same_state(tr, before)                                  # theta, m, v, arena, both step words, every statistic
    assert tr.t_steps == 1
    assert int(tr.skipped.item()) == 1 and int(tr.went.item()) == 0
    assert int(tr.status_or.item()) == bit
    with pytest.raises(ERRORS[bit]):
        tr.raise_on_error()
    tr.step(None, None)                                      # the next clean step: as if the bad one had never been
    twin.step(None, None)
    torch.cuda.synchronize()
    _same_state(tr, _state(twin), twin)
    assert tr.t_steps == 2 and int(tr.skipped.item()) == 1 and int(tr.went.item()) == 1
    tr.raise_on_error()


@pytest.mark.gpu
def test_a_nan_in_the_input_skips_the_step_end_to_end():
    """No hand-written status word: one NaN in one sample's features.  The solve itself sets ICNN_BE_ST_NONFINITE (BatchNorm may
    spread the NaN over the whole minibatch: only what the gate promises is asserted), the step does not go, and the next
    clean step is the twin's."""
    tr, x, t = _trainer("small", "dual", skip_on_error=True)
    twin, _, _ = _trainer("small", "dual")
    tr.step(x, t)
    twin.step(x, t)
    before = _state(tr)
    _same_state(twin, before)
    bad = x.clone()
    bad[3, 7] = float("nan")
    tr.step(bad, t)
    torch.cuda.synchronize()
    _same_state(tr, before)                                  # theta, m, v, arena, both step words, every statistic
    assert tr.t_steps == 1
    assert int(tr.skipped.item()) == 1 and int(tr.went.item()) == 0
    assert int(tr.status_or.item()) & _lib.ST_NONFINITE
    assert int(tr.solver.state.status[3].item()) & _lib.ST_NONFINITE
    with pytest.raises(FloatingPointError):
        tr.raise_on_error()
    tr.step(x, t)                                            # the clean batch again
    twin.step(None, None)
    torch.cuda.synchronize()
    _same_state(tr, _state(twin), twin)
    assert tr.t_steps == 2 and int(tr.skipped.item()) == 1 and int(tr.went.item()) == 1
    tr.raise_on_error()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", CASES)
def test_a_skipped_step_between_captured_halves(kind, variant):
    """the two halves of step() captured as two graphs; the bad word goes in between them with a copy and an eager plan"""
    tr, x, t = _trainer(kind, variant, skip_on_error=True)
    twin, _, _ = _trainer(kind, variant)
    bad = torch.tensor([_lib.ST_SINGULAR], dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.step(x, t)                                        # the warm-up step counts: the twin takes it too
    torch.cuda.current_stream().wait_stream(s)
    twin.step(x, t)
    infer, learn = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(infer):
        tr._infer()
    with torch.cuda.graph(learn):
        tr._learn()
    torch.cuda.synchronize()
    assert tr.t_steps == 1                                   # capturing ran nothing
    before = _state(tr)
    infer.replay()
    tr.solver.state.status[2:3].copy_(bad)
    tr.plan.run(tr.true_y)
    learn.replay()
    torch.cuda.synchronize()
    _same_state(tr, before)
    assert int(tr.skipped.item()) == 1 and int(tr.went.item()) == 0
    for _ in range(2):
        infer.replay()
        learn.replay()
        twin.step(None, None)
    torch.cuda.synchronize()
    _same_state(tr, _state(twin), twin)
    assert tr.t_steps == 3 and int(tr.skipped.item()) == 1 and int(tr.went.item()) == 1


# ------------------------------------------------------------------------------------------------ 4. the test phase


def _fresh_evaluation(tr, kind, variant, bn, xe, te):
    """what evaluate() must equal: a model of its own from the trainer's weights and statistics, its context in mode `bn`,
    a solver and a plan at E"""
    from icnn_amd import bundle_entropy, train
    spec, _, Model, _, _, _, n_iter, loss = _problem(kind)
    fresh = Model(spec, tr.host_params(), "cuda")
    fresh.set_bn_stats(tr.model.get_bn_stats())
    solver = bundle_entropy.FusedSolver(fresh, xe.shape[0], n_iter, variant)
    solver.solve(fresh.context(xe, bn=bn), 0.5)
    return solver, train.FeedPlan(solver.state, loss).run(te)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_fc_test_phase_equals_a_fresh_model_and_leaves_training_alone(variant):
    from icnn_amd import train
    tr, x, t = _trainer("small", variant, eval_batch=E_OF["small"])
    twin, _, _ = _trainer("small", variant)
    assert tr.eval_bn == "batch" and tr.eval_batch == 7 != tr.batch
    xe, te = _eval_batch("small")
    for one in (tr, twin):
        one.step(x, t)
        one.step(None, None)
    before = _state(tr)
    results = {k: getattr(tr, k).clone() for k in ("loss", "f1_tallies", "rows", "fg_evals", "status_or", "row_offset", "grad")}
    y_train = tr.solver.y.clone()
    loss = tr.evaluate(xe, te)
    torch.cuda.synchronize()
    assert loss is tr.eval_loss and loss.dtype == torch.float64 and np.isfinite(float(loss.item()))
    solver, plan = _fresh_evaluation(tr, "small", variant, "batch", xe, te)
    torch.cuda.synchronize()
    assert torch.equal(tr.eval_loss, plan.loss)
    assert torch.equal(tr.eval_f1_tallies, plan.f1_tallies) and tuple(tr.eval_f1_tallies.shape) == (7, 3)
    assert torch.equal(tr.y_eval, solver.y) and tuple(tr.y_eval.shape) == (7, 12)
    assert tr.eval_macro_f1() == train.macro_f1(plan.f1_tallies)
    _same_state(tr, before)                                  # no weight, no optimiser state, no statistic
    for k, v in results.items():
        assert torch.equal(getattr(tr, k), v), k
    assert torch.equal(tr.solver.y, y_train)
    tr.step(None, None)
    twin.step(None, None)
    torch.cuda.synchronize()
    _same_state(tr, _state(twin), twin)                      # the third step: as if nothing had been evaluated
    assert tr.t_steps == 3


@pytest.mark.gpu
def test_conv_test_phase_uses_the_moving_statistics():
    tr, x, t = _trainer("conv", "pdipm", eval_batch=E_OF["conv"])
    other, _, _ = _trainer("conv", "pdipm", eval_batch=E_OF["conv"], eval_bn="batch")
    twin, _, _ = _trainer("conv", "pdipm")
    assert tr.eval_bn == "moving" and other.eval_bn == "batch" and tr.eval_batch == 4 != tr.batch
    assert tr.eval_f1_tallies is None
    xe, te = _eval_batch("conv")
    for one in (tr, other, twin):
        one.step(x, t)
        one.step(None, None)
    before = _state(tr)
    train_loss, train_rows = tr.loss.clone(), tr.rows.clone()
    tr.evaluate(xe, te)
    other.evaluate(xe, te)
    torch.cuda.synchronize()
    solver, plan = _fresh_evaluation(tr, "conv", "pdipm", "moving", xe, te)
    torch.cuda.synchronize()
    assert torch.equal(tr.eval_loss, plan.loss) and np.isfinite(float(plan.loss.item()))
    assert torch.equal(tr.y_eval, solver.y)
    assert not torch.equal(other.eval_loss, tr.eval_loss)    # the mode is in effect
    _, plan_batch = _fresh_evaluation(other, "conv", "pdipm", "batch", xe, te)
    assert torch.equal(other.eval_loss, plan_batch.loss)
    with pytest.raises(ValueError):
        tr.eval_macro_f1()
    _same_state(tr, before)
    assert torch.equal(tr.loss, train_loss) and torch.equal(tr.rows, train_rows)
    tr.step(None, None)
    twin.step(None, None)
    torch.cuda.synchronize()
    _same_state(tr, _state(twin), twin)


# ------------------------------------------------------------------------------------------------ 5. capture and refusals


@pytest.mark.gpu
@pytest.mark.parametrize("kind,variant", CASES)
def test_evaluate_captured_equals_eager(kind, variant):
    tr, x, t = _trainer(kind, variant, eval_batch=E_OF[kind], y0=_row(kind))
    xe, te = _eval_batch(kind)
    tr.step(x, t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.evaluate(xe, te)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    want = {k: getattr(tr, k).clone() for k in ("eval_loss", "y_eval")}
    if tr.eval_f1_tallies is not None:
        want["eval_f1_tallies"] = tr.eval_f1_tallies.clone()
    before = _state(tr)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.evaluate(None, None)
    for k in want:
        getattr(tr, k).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(getattr(tr, k), v), k
    assert np.isfinite(float(tr.eval_loss.item())) and float(tr.eval_loss.item()) > 0
    _same_state(tr, before)


@pytest.mark.gpu
def test_evaluate_without_a_test_phase_raises():
    tr, x, t = _trainer("small", "pdipm")
    assert tr.eval_batch is None and tr.eval_loss is None and tr.y_eval is None
    with pytest.raises(ValueError):
        tr.evaluate(x[:7], t[:7])
    with pytest.raises(ValueError):
        tr.eval_macro_f1()
