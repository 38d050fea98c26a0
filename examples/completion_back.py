"""The back-optimisation loop of the image completion experiment (completion/icnn.back.py:210-254) on the device, on seeded
synthetic half-images (the Olivetti faces are not in the tree): each sample is a smooth random image 64 x 64, x its left half
and the target its right half.  A training step is train.ConvGDTrainer.step (30 steps of momentum GD from the mean target as
inference, the loss mean((255 (y_K - t))^2), TF-Adam with proj); every "epoch" the test phase runs on the held-out images with
the moving BatchNorm statistics.

    python examples/completion_back.py [--steps 20] [--batch 70] [--graph] [--n-train 280] [--n-test 50] [--seed 0]

--graph captures the training step and the test phase once and replays them.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--n-train", type=int, default=280)
    ap.add_argument("--n-test", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    rng = np.random.RandomState(args.seed)
    trainX, trainY = make_data(args.n_train, args.seed)
    valX, valY = make_data(args.n_test, args.seed + 1)
    spec = picnn.ConvSpec()
    params = picnn.make_convex(picnn.init_conv_params(spec, args.seed), divisor=2)          # makeCvx, icnn.back.py:164
    mean_y = trainY.mean(axis=0)                                                             # the start of every inference
    trainer = train.ConvGDTrainer(picnn.ConvModel(spec, params), args.batch, y0=mean_y, bn_updates=1, eval_batch=args.n_test)
    trainX, trainY = torch.from_numpy(trainX).cuda(), torch.from_numpy(trainY).cuda()
    # the h-flip of x is the caller's (icnn.back.py:220, :246)
    trainer.x_eval.copy_(torch.from_numpy(valX[:, :, ::-1].copy()).cuda())
    trainer.t_eval.copy_(torch.from_numpy(valY).cuda().view(trainer.t_eval.shape))
    step, evaluate = trainer.step, trainer.evaluate
    if args.graph:
        step, evaluate = captured(trainer.step), captured(trainer.evaluate)
    per_epoch = int(np.ceil(args.n_train / args.batch))
    for i in range(args.steps):
        idx = torch.from_numpy(rng.randint(args.n_train, size=args.batch)).cuda()
        trainer.x.copy_(trainX[idx].flip(2))
        trainer.t.copy_(trainY[idx].view(trainer.t.shape))
        step()
        print("=== Iteration %d (Epoch %.2f) ===\n + loss: %.5e" % (i, i / per_epoch, float(trainer.loss.item())))
        if i % per_epoch == 0:
            evaluate()
            print("=== Testing ===\n + test loss: %.5e" % float(trainer.eval_loss.item()))
    print("%d updates" % trainer.t_steps)


if __name__ == "__main__":
    main()
