"""The back-optimisation loop of the image completion experiment (completion/icnn.back.py:210-254) on the device, on seeded
synthetic half-images (the Olivetti faces are not in the tree): each sample is a smooth random image 64 x 64, x its left half
and the target its right half.  A training step is train.ConvGDTrainer.step (30 steps of momentum GD from the mean target as
inference, the loss mean((255 (y_K - t))^2), TF-Adam with proj); every "epoch" the test phase runs on the held-out images with
the moving BatchNorm statistics.

    python examples/completion_back.py [--steps 20] [--batch 70] [--graph] [--n-train 280] [--n-test 50] [--seed 0]

The training set lives on the device (train.DeviceDataset, x h-flipped once when it is built: icnn.back.py:220 flips every
batch the same way) and a minibatch draw is one launch; the per-iteration losses go to a device log (train.StepLog) that the
host reads once per epoch.  --graph runs an epoch -- [draw, step, log row] x batches per epoch -- as one graph that a
train.EpochRunner captures once and replays, and captures the test phase.  The minibatches are drawn with the library's Philox
stream (include/icnn_be.h, icnn_be_dataset_draw), not NumPy's Mersenne Twister: the batch sequence, and with it the printed
numbers, differ from those of versions that drew on the host.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icnn_amd import picnn, train  # noqa: E402


def make_data(n, seed):
    """n images [64, 64] in [0, 1]: a few random low-frequency waves each; (left halves, right halves) as [n, 64, 32, 1]"""
    rng = np.random.RandomState(seed)
    r, c = np.meshgrid(np.arange(64) / 64.0, np.arange(64) / 64.0, indexing="ij")
    img = np.zeros((n, 64, 64))
    for _ in range(4):
        fr, fc, ph = rng.uniform(0.5, 3.0, (n, 1, 1)), rng.uniform(0.5, 3.0, (n, 1, 1)), rng.uniform(0, 2 * np.pi, (n, 1, 1))
        img += rng.uniform(0.2, 1.0, (n, 1, 1)) * np.sin(2 * np.pi * (fr * r + fc * c) + ph)
    img = (img - img.min(axis=(1, 2), keepdims=True)) / np.ptp(img, axis=(1, 2), keepdims=True)
    img = img.astype(np.float32)[..., None]
    return np.ascontiguousarray(img[:, :, :32]), np.ascontiguousarray(img[:, :, 32:])


def captured(fn):
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph.replay


def target_buffer(trainer):
    """the trainer's target buffer: true_y of a BundleTrainer, t of the GD trainers"""
    return trainer.true_y if hasattr(trainer, "true_y") else trainer.t


def epoch_loop(trainer, data, log, steps, per_epoch, graph, report, evaluate):
    """The scripts' loop: iteration i trains on a fresh minibatch, and the test phase follows every iteration with i %
    per_epoch == 0 (icnn.back.py:241).  So iteration 0 runs alone and the rest in chains of per_epoch iterations that end on
    such an i; report(first, rows) gets the log's rows of iterations first, first + 1, ... after every chain and returns
    False to stop.  graph: the chains are train.EpochRunner graphs, else eager launches of the same sequence."""
    def eager(k):
        def run():
            for _ in range(k):
                data.draw_into(trainer.x, target_buffer(trainer))
                trainer.step()
                log.append()
        return run
    one = train.EpochRunner(trainer, data, 1, log=log).run if graph else eager(1)
    chain = one if per_epoch == 1 else train.EpochRunner(trainer, data, per_epoch, log=log).run if graph else eager(per_epoch)
    done = 0
    while done < steps:
        k = 1 if done == 0 else min(per_epoch, steps - done)
        if k == per_epoch and done > 0:
            chain()
        else:
            for _ in range(k):
                one()
        if not report(done, log.read()):
            return
        done += k
        if (done - 1) % per_epoch == 0:
            evaluate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--n-train", type=int, default=280)
    ap.add_argument("--n-test", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    trainX, trainY = make_data(args.n_train, args.seed)
    valX, valY = make_data(args.n_test, args.seed + 1)
    spec = picnn.ConvSpec()
    params = picnn.make_convex(picnn.init_conv_params(spec, args.seed), divisor=2)          # makeCvx, icnn.back.py:164
    mean_y = trainY.mean(axis=0)                                                             # the start of every inference
    trainer = train.ConvGDTrainer(picnn.ConvModel(spec, params), args.batch, y0=mean_y, bn_updates=1, eval_batch=args.n_test)
    # the h-flip of x is the caller's (icnn.back.py:220, :246): once, when the set is built
    data = train.DeviceDataset((trainX[:, :, ::-1].copy(), trainY.reshape(args.n_train, -1)), seed=args.seed)
    trainer.x_eval.copy_(torch.from_numpy(valX[:, :, ::-1].copy()).cuda())
    trainer.t_eval.copy_(torch.from_numpy(valY).cuda().view(trainer.t_eval.shape))
    per_epoch = int(np.ceil(args.n_train / args.batch))
    log = train.StepLog([("loss", trainer.loss)], per_epoch)
    run_test = captured(trainer.evaluate) if args.graph else trainer.evaluate

    def report(first, rows):
        for j, loss in enumerate(rows["loss"]):
            print("=== Iteration %d (Epoch %.2f) ===\n + loss: %.5e" % (first + j, (first + j) / per_epoch, loss))
        return True

    def evaluate():
        run_test()
        print("=== Testing ===\n + test loss: %.5e" % float(trainer.eval_loss.item()))

    epoch_loop(trainer, data, log, args.steps, per_epoch, args.graph, report, evaluate)
    print("%d updates" % trainer.t_steps)


if __name__ == "__main__":
    main()
