"""Train the FICNN or the PICNN of the synthetic classification experiment (synthetic-cls/icnn.py) on the device: moons,
circles or linearly separable points generated with NumPy, 30 steps of momentum GD as inference, full-batch TF-Adam with proj.

    python examples/synthetic_cls.py [--model ficnn|picnn] [--dataset moons|circles|linear] [--epochs 100]
                                     [--head sum|linear] [--n 100] [--save DIR]

--save DIR keeps the model with the best train loss (icnn.py:206-209) through a train.BestKeeper on the device and writes
DIR/best.npz and the checkpoint DIR/last.npz at the end.  Unlike the script's `bestMSE is None or ...` a NaN loss is never kept.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icnn_amd import checkpoint, ficnn, picnn, train  # noqa: E402


def make_data(name, n, seed):
    rng = np.random.RandomState(seed)
    h = n // 2
    if name == "moons":
        a, b = rng.rand(h) * np.pi, rng.rand(n - h) * np.pi
        X = np.r_[np.c_[np.cos(a), np.sin(a)], np.c_[1 - np.cos(b), 0.5 - np.sin(b)]] + 0.1 * rng.randn(n, 2)
        Y = np.r_[np.zeros(h), np.ones(n - h)]
    elif name == "circles":
        a = rng.rand(n) * 2 * np.pi
        r = np.r_[np.ones(h), 0.5 * np.ones(n - h)]
        X = np.c_[r * np.cos(a), r * np.sin(a)] + 0.05 * rng.randn(n, 2)
        Y = np.r_[np.zeros(h), np.ones(n - h)]
    elif name == "linear":
        X = rng.uniform(-1, 1, (n, 2))
        Y = (X[:, 0] + 0.5 * X[:, 1] + 0.2 * rng.randn(n) > 0).astype(np.float64)
    else:
        raise ValueError(name)
    return X.astype(np.float32), Y.reshape(n, 1).astype(np.float32)


def make_trainer(model, head, n, seed):
    """the trainer of --model: makeCvx after initialisation (icnn.py:172), |W| for the FICNN here, |W| / 10 (:145) for the
    PICNN; trainer.step(x, y) is one epoch"""
    if model == "picnn":
        spec = picnn.synthetic_spec()
        params = picnn.make_convex(picnn.init_params(spec, seed), divisor=10)
        return train.GDTrainer(picnn.FCModel(spec, params), n)
    spec = ficnn.synthetic_spec(head)
    params = ficnn.make_convex(ficnn.init_params(spec, seed))
    return ficnn.GDTrainer(ficnn.FICNNModel(spec, params), n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ficnn", choices=["ficnn", "picnn"])
    ap.add_argument("--dataset", default="moons", choices=["moons", "circles", "linear"])
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--head", default="sum", choices=["sum", "linear"])
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, metavar="DIR")
    args = ap.parse_args()
    X, Y = make_data(args.dataset, args.n, args.seed)
    trainer = make_trainer(args.model, args.head, args.n, args.seed)
    keeper = train.BestKeeper(trainer, mode="min") if args.save else None
    x, y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    for epoch in range(args.epochs):
        loss = trainer.step(x if epoch == 0 else None, y if epoch == 0 else None)
        if keeper is not None:
            keeper.offer(loss)
        print("=== Epoch %d ===\n + loss: %.5e" % (epoch, float(loss.item())))
    if args.save:
        os.makedirs(args.save, exist_ok=True)
        checkpoint.save_best(os.path.join(args.save, "best.npz"), keeper)
        checkpoint.save(os.path.join(args.save, "last.npz"), trainer, keeper=keeper)
        print("kept %d of %d epochs, best train loss %.5e: %s" % (keeper.kept, keeper.offers, keeper.best_value(),
                                                                  os.path.join(args.save, "best.npz")))


if __name__ == "__main__":
    main()
