"""The bundle-entropy loop of the image completion experiment (completion/icnn_ebundle.py:205-300) on the device, on seeded
synthetic half-images (the Olivetti faces are not in the tree): each sample is a smooth random image 64 x 64, x its left half
and the target its right half.  A training step is train.BundleTrainer.step with loss "mse": the solve starts from the mean
target (meanY, :223-227), a step whose solve reports an error is skipped on the device (skip_on_error, the script's
try/except around solveBatch, :225-237), and every "epoch" the test phase runs on the held-out images with the moving
BatchNorm statistics (evaluate, :264-300).  The loop gives up when more than --max-errors steps were skipped (maxErrors = 20).

    python examples/completion_ebundle.py [--steps 20] [--batch 70] [--graph] [--n-train 280] [--n-test 50] [--seed 0]

The training set lives on the device (train.DeviceDataset, x h-flipped once when it is built: icnn_ebundle.py:215 flips
every batch the same way) and a minibatch draw is one launch; the per-iteration loss, went and skipped words go to a device
log (train.StepLog) that the host reads once per epoch, which is also when it looks at --max-errors.  A skipped step still
consumes its minibatch, as the script draws before its try.  --graph runs an epoch -- [draw, step, log row] x batches per
epoch -- as one graph that a train.EpochRunner captures once and replays, and captures the test phase.  The minibatches are
drawn with the library's Philox stream (include/icnn_be.h, icnn_be_dataset_draw), not NumPy's Mersenne Twister: the batch
sequence, and with it the printed numbers, differ from those of versions that drew on the host.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.completion_back import captured, epoch_loop, make_data  # noqa: E402
from icnn_amd import picnn, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--n-train", type=int, default=280)
    ap.add_argument("--n-test", type=int, default=50)
    ap.add_argument("--max-errors", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    trainX, trainY = make_data(args.n_train, args.seed)
    valX, valY = make_data(args.n_test, args.seed + 1)
    spec = picnn.ConvSpec()
    params = picnn.make_convex(picnn.init_conv_params(spec, args.seed), divisor=2)          # makeCvx, icnn_ebundle.py:190
    mean_y = trainY.mean(axis=0)                                                             # the start of every solve
    trainer = train.BundleTrainer(picnn.ConvModel(spec, params), args.batch, n_iter=5, loss="mse", y0=mean_y,
                                  eval_batch=args.n_test, skip_on_error=True)
    # the h-flip of x is the caller's (icnn_ebundle.py:215, :270): once, when the set is built; true_y is float64
    data = train.DeviceDataset((trainX[:, :, ::-1].copy(), trainY.reshape(args.n_train, -1).astype(np.float64)), seed=args.seed)
    trainer.x_eval.copy_(torch.from_numpy(valX[:, :, ::-1].copy()).cuda())
    trainer.true_y_eval.copy_(torch.from_numpy(valY).cuda().view(trainer.true_y_eval.shape))
    per_epoch = int(np.ceil(args.n_train / args.batch))
    log = train.StepLog([("loss", trainer.loss), ("went", trainer.went), ("skipped", trainer.skipped)], per_epoch)
    run_test = captured(trainer.evaluate) if args.graph else trainer.evaluate

    def report(first, rows):
        for j, (loss, went) in enumerate(zip(rows["loss"], rows["went"])):
            print("=== Iteration %d (Epoch %.2f) ===\n + loss: %.5e%s"
                  % (first + j, (first + j) / per_epoch, loss, "" if went else "  (skipped)"))
        if rows["skipped"][-1] > args.max_errors:
            print("%d steps skipped on a solver error: quitting" % rows["skipped"][-1])
            return False
        return True

    def evaluate():
        run_test()
        print("=== Testing ===\n + test loss: %.5e" % float(trainer.eval_loss.item()))

    epoch_loop(trainer, data, log, args.steps, per_epoch, args.graph, report, evaluate)
    print("%d updates, %d steps skipped" % (trainer.t_steps, int(trainer.skipped.item())))


if __name__ == "__main__":
    main()
