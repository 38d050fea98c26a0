"""The bundle-entropy loop of the image completion experiment (completion/icnn_ebundle.py:205-300) on the device, on seeded
synthetic half-images (the Olivetti faces are not in the tree): each sample is a smooth random image 64 x 64, x its left half
and the target its right half.  A training step is train.BundleTrainer.step with loss "mse": the solve starts from the mean
target (meanY, :223-227), a step whose solve reports an error is skipped on the device (skip_on_error, the script's
try/except around solveBatch, :225-237), and every "epoch" the test phase runs on the held-out images with the moving
BatchNorm statistics (evaluate, :264-300).  The loop gives up when more than --max-errors steps were skipped (maxErrors = 20).

    python examples/completion_ebundle.py [--steps 20] [--batch 70] [--graph] [--n-train 280] [--n-test 50] [--seed 0]

--graph captures the training step and the test phase once and replays them.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from examples.completion_back import captured, make_data  # noqa: E402
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
    rng = np.random.RandomState(args.seed)
    trainX, trainY = make_data(args.n_train, args.seed)
    valX, valY = make_data(args.n_test, args.seed + 1)
    spec = picnn.ConvSpec()
    params = picnn.make_convex(picnn.init_conv_params(spec, args.seed), divisor=2)          # makeCvx, icnn_ebundle.py:190
    mean_y = trainY.mean(axis=0)                                                             # the start of every solve
    trainer = train.BundleTrainer(picnn.ConvModel(spec, params), args.batch, n_iter=5, loss="mse", y0=mean_y,
                                  eval_batch=args.n_test, skip_on_error=True)
    trainX, trainY = torch.from_numpy(trainX).cuda(), torch.from_numpy(trainY).cuda()
    # the h-flip of x is the caller's (icnn_ebundle.py:215, :270)
    trainer.x_eval.copy_(torch.from_numpy(valX[:, :, ::-1].copy()).cuda())
    trainer.true_y_eval.copy_(torch.from_numpy(valY).cuda().view(trainer.true_y_eval.shape))
    step, evaluate = trainer.step, trainer.evaluate
    if args.graph:
        step()                                            # a first step outside the capture (it counts as an update)
        step, evaluate = captured(trainer.step), captured(trainer.evaluate)
    per_epoch = int(np.ceil(args.n_train / args.batch))
    for i in range(args.steps):
        idx = torch.from_numpy(rng.randint(args.n_train, size=args.batch)).cuda()
        trainer.x.copy_(trainX[idx].flip(2))
        trainer.true_y.copy_(trainY[idx].view(trainer.true_y.shape))
        step()
        loss, went, skipped = float(trainer.loss.item()), int(trainer.went.item()), int(trainer.skipped.item())
        print("=== Iteration %d (Epoch %.2f) ===\n + loss: %.5e%s" % (i, i / per_epoch, loss, "" if went else "  (skipped)"))
        if skipped > args.max_errors:
            print("%d steps skipped on a solver error: quitting" % skipped)
            break
        if i % per_epoch == 0:
            evaluate()
            print("=== Testing ===\n + test loss: %.5e" % float(trainer.eval_loss.item()))
    print("%d updates, %d steps skipped" % (trainer.t_steps, int(trainer.skipped.item())))


if __name__ == "__main__":
    main()
