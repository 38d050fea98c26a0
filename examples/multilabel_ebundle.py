"""A short bundle-entropy training loop on seeded synthetic multi-label data (the loop of multi-label-cls/icnn_ebundle.py:208-250)
with no host data in it: the training set lives on the device (train.DeviceDataset), and `--every` iterations of [minibatch
draw, train.BundleTrainer.step, log row] are one graph that a train.EpochRunner captures once and replays.

    python examples/multilabel_ebundle.py [--steps 60] [--batch 64] [--every 10] [--test-every 20] [--save DIR] [--resume FILE]
                                          [--dataset bibtex|bookmarks|delicious] [--layerSizes 600 [600]]

Without --dataset the network is a small one (40 features, 16 labels, hidden widths 64); with it, the network has the
dataset's shape (bibtex 1836 features / 159 labels, bookmarks 2150 / 208, delicious 500 / 983) and the hidden widths
--layerSizes of the script, on synthetic data of that shape.  Shapes whose 16-sample evaluation tile outgrows the LDS run
on tiles of 8 or 4 rows (FCModel.tile_rows).

The labels are a noisy linear function of the features; the loss falls from the first steps on (685.7 at step 10 to 642.3 at
step 60 with the defaults on an MI355X).
The host reads the per-step losses from the device log (train.StepLog) and the F1 tallies only every `--every` steps.
The minibatches are drawn with the library's Philox stream (include/icnn_be.h, icnn_be_dataset_draw), not NumPy's
Mersenne Twister: the batch sequence, and with it the printed numbers, differ from those of versions that drew on the host.
Every `--test-every` steps (0: never) the test phase of the script (:257-277) runs on a held-out split of the same
distribution: one replay of a captured train.BundleTrainer.evaluate, then the test loss and macro-F1.
--save DIR keeps the model with the best test F1 (icnn_ebundle.py:274-277, `if testF1 > bestTestF1: save`) through a
train.BestKeeper INSIDE the captured test graph -- the comparison and the snapshot happen on the device -- and writes
DIR/best.npz and the checkpoint DIR/last.npz at the end; --resume FILE continues from such a checkpoint.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import checkpoint, picnn, train  # noqa: E402


DATASETS = {"bibtex": picnn.bibtex_spec, "bookmarks": picnn.bookmarks_spec, "delicious": picnn.delicious_spec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--test-every", type=int, default=20)
    ap.add_argument("--save", default=None, metavar="DIR")
    ap.add_argument("--resume", default=None, metavar="FILE")
    ap.add_argument("--dataset", choices=sorted(DATASETS), default=None)
    ap.add_argument("--layerSizes", type=int, nargs="+", default=[600])
    a = ap.parse_args()
    if a.save and not a.test_every:
        ap.error("--save keeps the best model by test F1: it needs --test-every > 0")
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    n_features, n_labels, n_train, n_test = 40, 16, 1024, 256
    spec = picnn.FCSpec(n_features, n_labels, (64, 32), alpha=0.0, batchnorm=True, action_box=False)
    if a.dataset:
        spec = DATASETS[a.dataset](tuple(a.layerSizes))
        n_features, n_labels = spec.n_features, spec.n_labels
    held_out = np.random.RandomState(1)                    # a generator of its own: the training data stay what they were
    if a.dataset:                                          # bag-of-words features: 4 % of them set, as in the other examples
        W = rng.randn(n_features, n_labels) / np.sqrt(0.04 * n_features)

        def draw(g, rows):
            x = (g.rand(rows, n_features) < 0.04).astype(np.float32)
            return x, ((x - 0.04) @ W + 0.3 * g.randn(rows, n_labels) > 0.8).astype(np.float64)
        X, Y = draw(rng, n_train)
        Xt, Yt = draw(held_out, n_test)
    else:
        X = rng.rand(n_train, n_features).astype(np.float32)
        W = rng.randn(n_features, n_labels)
        Y = ((X - 0.5) @ W + 0.3 * rng.randn(n_train, n_labels) > 0.8).astype(np.float64)
        Xt = held_out.rand(n_test, n_features).astype(np.float32)
        Yt = ((Xt - 0.5) @ W + 0.3 * held_out.randn(n_test, n_labels) > 0.8).astype(np.float64)
    model = picnn.FCModel(spec, picnn.init_params(spec, 0, "spread"), "cuda")
    if a.dataset:
        print("%s %s: %d features, %d labels, evaluation tiles of %d rows"
              % (a.dataset, " ".join(map(str, a.layerSizes)), n_features, n_labels, model.tile_rows))
    trainer = train.BundleTrainer(model, a.batch, n_iter=10, loss="xent", lr=1e-3, eval_batch=n_test if a.test_every else None)
    # the keeper moves the BatchNorm statistics into one buffer: built before anything is captured
    keeper = train.BestKeeper(trainer, mode="max", start=0.0) if a.save else None
    data = train.DeviceDataset((X, Y), seed=0)
    every = max(1, a.every)
    log = train.StepLog([("loss", trainer.loss)], every)
    # [draw, step, log] x every: the first run is eager, the second captures the chain, later ones replay it
    runner = train.EpochRunner(trainer, data, every, log=log)
    tail = train.EpochRunner(trainer, data, 1, log=log)    # the steps behind the last whole chain
    s = torch.cuda.Stream()
    test_graph = None
    if a.test_every:                                       # the whole held-out split is one evaluation batch
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            trainer.evaluate(torch.from_numpy(Xt).cuda(), torch.from_numpy(Yt).cuda())
        torch.cuda.current_stream().wait_stream(s)
        test_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(test_graph):
            trainer.evaluate(None, None)
            if keeper is not None:
                keeper.offer_macro_f1(trainer.eval_f1_tallies)
    if a.resume:                                           # into the existing tensors: the graphs above replay on the loaded state
        checkpoint.load(a.resume, trainer, keeper=keeper, dataset=data)
        print("resumed %s at step %d, draw %d" % (a.resume, trainer.t_steps, data.draws))
    i = 0
    while i < a.steps:
        stop = min(a.steps, (i // every + 1) * every)
        if a.test_every:                                   # a test phase falls where it fell before: on its own multiples
            stop = min(stop, (i // a.test_every + 1) * a.test_every)
        if stop - i == every:
            runner.run()
        else:
            for _ in range(stop - i):
                tail.run()
        i = stop
        if i % every == 0 or i == a.steps:
            losses = log.read()["loss"]                    # synchronises
            trainer.raise_on_error()
            print("step %4d  loss %10.4f  (mean of the last %d: %.4f)  macro F1 %.3f  feed rows %d of %d  fg evaluations %d"
                  % (i, losses[-1], len(losses), losses.mean(), trainer.macro_f1(), int(trainer.rows.item()),
                     trainer.feed.row_cap, int(trainer.fg_evals.item())))
        if test_graph is not None and (i % a.test_every == 0 or i == a.steps):
            test_graph.replay()
            torch.cuda.synchronize()
            print("           test loss %10.4f  test macro F1 %.3f  (%d held-out examples)"
                  % (float(trainer.eval_loss.item()), trainer.eval_macro_f1(), n_test))
    if a.save:
        os.makedirs(a.save, exist_ok=True)
        checkpoint.save_best(os.path.join(a.save, "best.npz"), keeper)
        checkpoint.save(os.path.join(a.save, "last.npz"), trainer, keeper=keeper, dataset=data)
        print("kept %d of %d test phases, best test macro F1 %.3f: %s" % (keeper.kept, keeper.offers, keeper.best_value(),
                                                                          os.path.join(a.save, "best.npz")))


if __name__ == "__main__":
    main()
