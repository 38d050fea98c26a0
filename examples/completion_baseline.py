"""The FCN baseline of the completion experiment (completion/baseline.py) on the device: the script's loop on seeded synthetic
Olivetti-shaped data, or on a data set of your own, with no host wait inside an epoch.

    python examples/completion_baseline.py [--epochs 5] [--batch 70] [--k 32] [--data FILE.npz] [--save DIR] [--resume FILE]

The training set lives on the device (train.DeviceDataset); an epoch is ceil(nTrain / batch) iterations of [minibatch draw,
fcn.FCNTrainer.step, log row], one graph that a train.EpochRunner captures once and replays.  The reference's
DataLoader(shuffle=True) walks a permutation per epoch; DeviceDataset draws WITH replacement, so an epoch here sees the same
count of images but not each exactly once.  After every epoch the script's test phase (baseline.py:102-108) runs on the whole
test split: forward and loss, nothing of the model written.  The best test loss is the minimum the HOST takes over the epochs'
eval_loss, as the script does.  train.BestKeeper serves trainers that own a DeviceAdam as .opt; this trainer's update is torch's
Adam in a kernel of its own, so the keeper is not wired (the script keeps no model at its best loss either).
That minimum is the number examples/completion_ebundle.py and examples/completion_back.py are read against.

The images are [H, W] = [64, 32] row-major, the layout of ConvGDTrainer.x / .t, so one DeviceDataset serves both completion
trainers.  The reference transposes its images to 32 x 64 first; every kernel, stride, dilation and padding of the net is
square, so the net on the untransposed images is the same family with transposed 3x3 kernels.

--data FILE.npz holds trainX [N, 64, 32] (or [N, 64, 32, 1]), trainY, testX, testY in [0, 1]; without it the data are smooth
random images whose right halves (the targets) continue the left halves.  --save DIR writes the checkpoint DIR/last.npz at
the end; --resume FILE continues from such a checkpoint (weights, Adam's state, step count, the draw counter).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import checkpoint, fcn, train  # noqa: E402


def synthetic(n_train, n_test, H=64, W=32):
    """smooth images of 64 x 64 from a few random low-frequency waves: the left half is x, the right half t"""
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:H, 0:2 * W].astype(np.float64)

    def split(n):
        img = np.zeros((n, H, 2 * W))
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.02, 0.12, (n, 1, 1)), rng.uniform(0.02, 0.12, (n, 1, 1)), rng.uniform(0, 6.28, (n, 1, 1))
            img += np.sin(fy * yy + fx * xx + ph)
        img = (img - img.min((1, 2), keepdims=True)) / (np.ptp(img, (1, 2), keepdims=True) + 1e-9)
        return img[:, :, :W].astype(np.float32), img[:, :, W:].astype(np.float32)

    return split(n_train) + split(n_test)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--data", default=None, metavar="FILE.npz")
    ap.add_argument("--n-train", type=int, default=350)
    ap.add_argument("--n-test", type=int, default=50)
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
    N, H, W = X.shape[:3]
    X, Xt = X.reshape(N, H, W, 1), Xt.reshape(-1, H, W, 1)
    Y, Yt = Y.reshape(N, H * W), Yt.reshape(-1, H * W)
    model = fcn.FCNModel(fcn.FCNSpec(H, W, a.k), seed=a.seed)
    trainer = fcn.FCNTrainer(model, a.batch, lr=a.lr, eval_batch=Xt.shape[0])
    data = train.DeviceDataset((X, Y), seed=a.seed)
    per_epoch = -(-N // a.batch)
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
    best = None
    for epoch in range(1, a.epochs + 1):
        runner.run()                                       # eager, then captured, then replays
        losses = log.read()["loss"]                        # the one wait of the epoch
        test_graph.replay()
        test_loss = float(trainer.eval_loss.item())
        if best is None or test_loss < best:               # baseline.py:106-108
            best = test_loss
        print("epoch %3d  step %6d  train loss %10.3f (mean of the epoch %.3f)  test loss %10.3f"
              % (epoch, trainer.t_steps, losses[-1], losses.mean(), test_loss))
    print("best test loss %.3f" % best)
    if a.save:
        os.makedirs(a.save, exist_ok=True)
        checkpoint.save(os.path.join(a.save, "last.npz"), trainer, dataset=data)
        print("saved %s" % os.path.join(a.save, "last.npz"))


if __name__ == "__main__":
    main()
