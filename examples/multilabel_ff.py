"""The feed-forward baseline of the multi-label experiment (multi-label-cls/ff.py) on the device: the script's loop on seeded
synthetic Bibtex-shaped data, or on a data set of your own, with no host wait inside an epoch.

    python examples/multilabel_ff.py [--epochs 5] [--batch 128] [--layers 600] [--data FILE.npz] [--save DIR] [--resume FILE]

The training set lives on the device (train.DeviceDataset); an epoch is ceil(nTrain / batch) iterations of [minibatch draw,
ff.FFTrainer.step, log row], one graph that a train.EpochRunner captures once and replays.  After every epoch the host reads
the epoch's losses from the device log (train.StepLog), and the script's test phase (ff.py:187-196) runs on the whole test
split in inference mode: one replay of a captured FFTrainer.evaluate, then the test loss and macro-F1.  The script keeps no
model at its best F1 (ff.py:200-212 is commented out): the host takes the maximum of the test scores, which is the number the
ICNN examples (multilabel_ebundle.py, synthetic_cls.py) are read against.

--data FILE.npz holds trainX [N, f], trainY [N, n], testX, testY; without it the data are 0 / 1 bag-of-words rows (1836
features, 4 % ones, 159 labels) whose labels are a noisy linear function of the features.  --save DIR writes the checkpoint
DIR/last.npz at the end; --resume FILE continues from such a checkpoint (weights, Adam's state, step count, moving statistics,
the draw counter).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import checkpoint, ff, train  # noqa: E402


def synthetic(n_train, n_test, n_features=1836, n_labels=159):
    rng = np.random.RandomState(0)
    W = rng.randn(n_features, n_labels) / np.sqrt(0.04 * n_features)

    def split(n):
        X = (rng.rand(n, n_features) < 0.04).astype(np.float32)
        return X, (X @ W + 0.3 * rng.randn(n, n_labels) > 1.2).astype(np.float32)

    return split(n_train) + split(n_test)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--layers", type=int, nargs="+", default=[600])
    ap.add_argument("--data", default=None, metavar="FILE.npz")
    ap.add_argument("--n-train", type=int, default=4096)
    ap.add_argument("--n-test", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, metavar="DIR")
    ap.add_argument("--resume", default=None, metavar="FILE")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.data:
        d = np.load(a.data)
        X, Y, Xt, Yt = (np.ascontiguousarray(d[k], np.float32) for k in ("trainX", "trainY", "testX", "testY"))
    else:
        X, Y, Xt, Yt = synthetic(a.n_train, a.n_test)
    spec = ff.FFSpec(X.shape[1], Y.shape[1], tuple(a.layers))
    model = ff.FFModel(spec, seed=a.seed)
    trainer = ff.FFTrainer(model, a.batch, eval_batch=Xt.shape[0])
    data = train.DeviceDataset((X, Y), seed=a.seed)
    per_epoch = -(-X.shape[0] // a.batch)                  # ff.py:176, nIter = ceil(nTrain / batch)
    log = train.StepLog([("loss", trainer.loss)], per_epoch)
    runner = train.EpochRunner(trainer, data, per_epoch, log=log)
    # the test phase as a graph of its own: a warm-up on a side stream, then the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        trainer.evaluate(torch.from_numpy(Xt).cuda(), torch.from_numpy(Yt).cuda())
    torch.cuda.current_stream().wait_stream(s)
    test_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(test_graph):
        trainer.evaluate(None, None)
    if a.resume:                                           # into the existing tensors: the graphs replay on the loaded state
        checkpoint.load(a.resume, trainer, dataset=data)
        print("resumed %s at step %d, draw %d" % (a.resume, trainer.t_steps, data.draws))
    best = 0.0
    for epoch in range(1, a.epochs + 1):
        runner.run()                                       # eager, then captured, then replays
        losses = log.read()["loss"]                        # the one wait of the epoch
        train_f1 = trainer.macro_f1()
        test_graph.replay()
        torch.cuda.synchronize()
        test_f1 = trainer.eval_macro_f1()
        best = max(best, test_f1)
        print("epoch %3d  step %6d  train loss %10.3f (mean of the epoch %.3f)  train F1 %.4f  test loss %10.3f  test F1 %.4f"
              % (epoch, trainer.t_steps, losses[-1], losses.mean(), train_f1, float(trainer.eval_loss.item()), test_f1))
    print("best test macro F1 %.4f" % best)
    if a.save:
        os.makedirs(a.save, exist_ok=True)
        checkpoint.save(os.path.join(a.save, "last.npz"), trainer, dataset=data)
        print("saved %s" % os.path.join(a.save, "last.npz"))


if __name__ == "__main__":
    main()
