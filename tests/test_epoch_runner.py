"""Epochs as a graph (train.EpochRunner over train.DeviceDataset and train.StepLog): [draw, step, log] x steps run
eagerly, captured and replayed leaves a trainer bit for bit where a twin fed X[idx], Y[idx] through step(x, y) stands, with idx
from tests/dataset_ref.py; a skipped step still consumes its draw; a checkpoint with the dataset's control block resumes the
uninterrupted batch sequence.  The specs are the smallest of tests/test_bundle_trainer.py, tests/test_synth_picnn.py and
tests/test_conv_gd_trainer.py at batch <= 8 and n_iter <= 4, on N = 37 training rows.  Every comparison is between two orders
of the same launches: torch.equal, no tolerance."""
import numpy as np
import pytest
import torch

import dataset_ref as ref
from icnn_amd import _lib, picnn

pytestmark = pytest.mark.gpu

N, STEPS, RUNS, SEED = 37, 3, 3, (3 << 32) | 11
FC = picnn.FCSpec(20, 12, (24, 12), alpha=0.0, batchnorm=True, action_box=False)
FC_GD = picnn.FCSpec(20, 12, (24, 12), batchnorm=True, relu_last_u=True)
CONV = picnn.ConvSpec()
CONV_GD = picnn.ConvSpec(32, 32)
KINDS = ["bundle-fc", "bundle-conv", "gd-fc", "gd-conv"]


def _problem(kind):
    """(batch, make_trainer(**kw), X [N, ...] float32, Y [N, n] in the dtype of the trainer's target buffer)"""
    from icnn_amd import train
    rng = np.random.RandomState(KINDS.index(kind))
    if kind == "bundle-fc":
        params = picnn.init_params(FC, 5, "spread")
        X = rng.rand(N, FC.n_features).astype(np.float32)
        Y = (rng.rand(N, FC.n_labels) < 0.3).astype(np.float64)
        return 8, lambda **kw: train.BundleTrainer(picnn.FCModel(FC, {k: v.copy() for k, v in params.items()}, "cuda"), 8,
                                                   n_iter=4, loss="xent", variant="pdipm", lr=1e-3, **kw), X, Y
    if kind == "bundle-conv":
        params = picnn.init_conv_params(CONV, 8, "spread")
        X = rng.rand(N, CONV.H, CONV.W, 1).astype(np.float32)
        Y = rng.rand(N, CONV.n_labels)
        return 6, lambda **kw: train.BundleTrainer(picnn.ConvModel(CONV, {k: v.copy() for k, v in params.items()}, "cuda"), 6,
                                                   n_iter=3, loss="mse", variant="pdipm", lr=1e-3, **kw), X, Y
    if kind == "gd-fc":
        params = picnn.init_params(FC_GD, 3, "spread")
        X = rng.rand(N, FC_GD.n_features).astype(np.float32)
        Y = (rng.rand(N, FC_GD.n_labels) < 0.4).astype(np.float32)
        return 6, lambda **kw: train.GDTrainer(picnn.FCModel(FC_GD, {k: v.copy() for k, v in params.items()}, "cuda"), 6,
                                               n_iter=4, lr=0.1, momentum=0.3, bn_updates=1, **kw), X, Y
    params = picnn.init_conv_params(CONV_GD, 3, "spread")
    y0 = 0.2 + 0.6 * rng.rand(CONV_GD.n_labels)
    X = rng.rand(N, CONV_GD.H, CONV_GD.W, 1).astype(np.float32)
    Y = rng.rand(N, CONV_GD.n_labels).astype(np.float32)
    return 6, lambda **kw: train.ConvGDTrainer(picnn.ConvModel(CONV_GD, {k: v.copy() for k, v in params.items()}, "cuda"), 6,
                                               n_iter=4, lr=0.01, momentum=0.9, y0=y0, bn_updates=1, **kw), X, Y


def _state(tr):
    """clones of everything a later step depends on"""
    out = {"theta": tr.opt.theta, "m": tr.opt.m, "v": tr.opt.v, "arena": tr.opt.arena, "step_count": tr.opt.step_count}
    out.update({"bn:" + k: v for k, v in tr.model.bn_stats.items()})
    return {k: v.clone() for k, v in out.items()}


def _same(got, want):
    assert set(got) == set(want) and len(got) >= 7            # five tensors of the optimiser, two or more statistics
    for k, v in want.items():
        assert torch.equal(got[k], v), k


def _batch_of(X, Y, draw, batch):
    idx = ref.indices(SEED, draw, batch, N).astype(np.int64)
    return torch.from_numpy(X[idx]).cuda(), torch.from_numpy(Y[idx]).cuda()


@pytest.mark.parametrize("kind", KINDS)
def test_runner_equals_a_twin_fed_the_reference_batches(kind):
    from icnn_amd import train
    batch, make, X, Y = _problem(kind)
    tr, twin = make(), make()
    data = train.DeviceDataset((X, Y), seed=SEED)
    log = train.StepLog([("loss", tr.loss), ("updates", tr.opt.step_count[0:1])], 16)
    runner = train.EpochRunner(tr, data, STEPS, log=log)
    assert runner.buffers[0] is tr.x and runner.buffers[1] is (tr.true_y if kind.startswith("bundle") else tr.t)
    for r in range(RUNS):                                    # eager, capture + replay, replay
        runner.run()
        assert data.draws == STEPS * (r + 1) and runner.runs == r + 1
    losses = []
    for d in range(STEPS * RUNS):
        losses.append(float(twin.step(*_batch_of(X, Y, d, batch)).item()))
    got = log.read()
    _same(_state(tr), _state(twin))
    assert tr.t_steps == STEPS * RUNS == twin.t_steps
    assert got["loss"].tolist() == losses and len(set(losses)) == len(losses)
    assert got["updates"].tolist() == list(range(1, STEPS * RUNS + 1))      # the log row follows the step's update
    assert data.ctrl.cpu().tolist() == [STEPS * RUNS, 0, 0, 0, 0, 0, 0, 0]
    # the buffers hold the last batch, the index buffer its indices
    x, y = _batch_of(X, Y, STEPS * RUNS - 1, batch)
    assert torch.equal(tr.x, x.view(tr.x.shape)) and torch.equal(runner.buffers[1], y.view(runner.buffers[1].shape))


def test_a_skipped_step_still_consumes_its_draw():
    """skip_on_error: iteration 1 of the eager run is made to skip the way tests/test_bundle_trainer_loop.py does, a status
    word written by hand between the halves of the step.  The twin never sees that batch; the batches after it are the
    reference sequence's."""
    from icnn_amd import train
    batch, make, X, Y = _problem("bundle-fc")
    tr, twin = make(skip_on_error=True), make(skip_on_error=True)
    data = train.DeviceDataset((X, Y), seed=SEED)
    calls = [0]

    def step():
        tr._infer()
        if calls[0] == 1:
            tr.solver.state.status[3] = _lib.ST_SINGULAR
            tr.plan.run(tr.true_y)
        calls[0] += 1
        tr._learn()
        return tr.loss
    tr.step = step
    runner = train.EpochRunner(tr, data, STEPS, log=train.StepLog([("went", tr.went), ("skipped", tr.skipped)], 8))
    runner.run()
    for d in (0, 2):
        twin.step(*_batch_of(X, Y, d, batch))
    _same(_state(tr), _state(twin))
    assert tr.t_steps == 2 and int(tr.skipped.item()) == 1 and data.draws == 3 and int(data.ctrl[0].item()) == 3
    runner.run()                                             # captured and replayed: draws 3, 4, 5
    for d in (3, 4, 5):
        twin.step(*_batch_of(X, Y, d, batch))
    _same(_state(tr), _state(twin))
    got = runner.log.read()
    assert got["went"].tolist() == [1, 0, 1, 1, 1, 1] and got["skipped"].tolist() == [0, 1, 1, 1, 1, 1]
    assert tr.t_steps == 5 and int(data.ctrl[0].item()) == 6 and calls[0] == 6


def test_checkpoint_resumes_the_batch_sequence(tmp_path):
    """six uninterrupted iterations against three, a checkpoint, and three more in a fresh trainer + dataset whose graph was
    captured before the load; then the refusals, which leave the objects bit for bit as they were"""
    from icnn_amd import checkpoint, train
    batch, make, X, Y = _problem("bundle-fc")

    def fresh(n_rows=N, seed=SEED):
        tr = make()
        data = train.DeviceDataset((X[:n_rows], Y[:n_rows]), seed=seed)
        return tr, data, train.EpochRunner(tr, data, STEPS)
    whole, _, run_whole = fresh()
    run_whole.run()
    run_whole.run()
    first, data_first, run_first = fresh()
    run_first.run()
    path, bare = str(tmp_path / "ck.npz"), str(tmp_path / "bare.npz")
    checkpoint.save(path, first, dataset=data_first)
    checkpoint.save(bare, first)
    arrays = checkpoint.read_arrays(path)
    assert {k for k in arrays if k.startswith("data/")} == {"data/seed", "data/n_rows", "data/draws", "data/ctrl"}
    assert (int(arrays["data/seed"]), int(arrays["data/n_rows"]), int(arrays["data/draws"])) == (SEED, N, STEPS)
    assert set(checkpoint.read_arrays(bare)) == set(arrays) - {"data/seed", "data/n_rows", "data/draws", "data/ctrl"}
    later, data_later, run_later = fresh()
    run_later.run()
    run_later.run()                                          # the graph exists; the state is six iterations of its own
    assert run_later._graph is not None
    checkpoint.load(path, later, dataset=data_later)
    _same(_state(later), _state(first))
    assert data_later.draws == STEPS and data_later.ctrl.cpu().tolist() == data_first.ctrl.cpu().tolist()
    run_later.run()                                          # a replay, on the loaded state and counter
    torch.cuda.synchronize()
    _same(_state(later), _state(whole))
    assert data_later.draws == 2 * STEPS and int(data_later.ctrl[0].item()) == 2 * STEPS and later.t_steps == 2 * STEPS
    # ---- the refusals ----
    before, ctrl = _state(later), data_later.ctrl.clone()
    _, fewer, _ = fresh(n_rows=N - 1)
    _, other_seed, _ = fresh(seed=SEED + 1)
    for file, dataset, field in ((path, fewer, "data/n_rows"), (path, other_seed, "data/seed"), (path, None, "dataset"),
                                 (bare, data_later, "dataset")):
        marks = None if dataset is None else (dataset.ctrl.clone(), dataset.draws)
        with pytest.raises(ValueError, match=field):
            checkpoint.load(file, later, dataset=dataset)
        _same(_state(later), before)
        assert torch.equal(data_later.ctrl, ctrl) and data_later.draws == 2 * STEPS
        if marks is not None:
            assert torch.equal(dataset.ctrl, marks[0]) and dataset.draws == marks[1]


def test_runner_refuses_what_it_does_not_serve():
    from icnn_amd import train
    batch, make, X, Y = _problem("gd-fc")
    tr = make()
    data = train.DeviceDataset((X, Y))
    for args in [(object(), data, 3), (tr, object(), 3), (tr, data, 0)]:
        with pytest.raises((TypeError, ValueError)):
            train.EpochRunner(*args)
    with pytest.raises(TypeError):
        train.EpochRunner(tr, data, 3, log=object())
    with pytest.raises(ValueError):                          # Y in the wrong dtype for the trainer's buffer
        train.EpochRunner(tr, train.DeviceDataset((X, Y.astype(np.float64))), 1).run()
