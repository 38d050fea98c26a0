"""Time the FC-PICNN training gradient (icnn_amd.train.surrogate_grad, be_train_fc.hip) at the reference's training shape --
Bibtex, batch 128, nIter 10, the feed of a real solve (multi-label-cls/icnn_ebundle.py:173-288) -- against what a user has
without it: the PICNN restated in torch and differentiated twice by autograd (create_graph=True), float32, same device,
same rows.  Device events around each call; prints the row count R, both medians and one JSON line.

    python tools/train_grad_time.py [--reps 50] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icnn_amd import bundle_entropy, picnn, train  # noqa: E402


def torch_surrogate_grad(spec, theta, x_rows, y, v, c):
    """The reference graph in torch (float32) on the gathered rows, BatchNorm over them, double-backward autograd."""
    L = len(spec.szs)
    yt = y.float().requires_grad_(True)
    us, prev = [], x_rows
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                mean = u.mean(dim=0)
                var = ((u - mean) ** 2).mean(dim=0)
                u = (u - mean) / torch.sqrt(var + 1e-5) * theta["u%d/bn/gamma" % i] + theta["u%d/bn/beta" % i]
        us.append(u)
        prev = u
    prevU, prevZ = x_rows, yt
    for i in range(L + 1):
        add = prevU @ theta["z%d_u/W" % i] + theta["z%d_u/b" % i]
        if i > 0:
            gate = torch.relu(prevU @ theta["z%d_zu_u/W" % i] + theta["z%d_zu_u/b" % i])
            add = add + (prevZ * gate) @ theta["z%d_zu_proj/W" % i]
        add = add + (yt * (prevU @ theta["z%d_yu_u/W" % i] + theta["z%d_yu_u/b" % i])) @ theta["z%d_yu/W" % i]
        z = torch.where(add > 0, add, spec.alpha * add) if i < L else add
        prevU = us[i] if i < L else None
        prevZ = z
    E = z.reshape(-1)
    dEdy, = torch.autograd.grad(E.sum(), yt, create_graph=True)
    F = c.float() * E + (dEdy * v.float()).sum(dim=1)
    return torch.autograd.grad(F.sum(), list(theta.values()))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--niter", type=int, default=10)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    spec = picnn.bibtex_spec()
    params = picnn.init_params(spec, 0, "spread")
    B = args.batch
    rng = np.random.RandomState(0)
    x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
    labels = (rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)
    model = picnn.FCModel(spec, params, "cuda:0")
    res = bundle_entropy.FusedSolver(model, B, args.niter, "dual").solve(model.context(x), 0.5)
    feed = bundle_entropy.implicit_feed(res, labels, "xent")
    R = int(feed.sample.numel())
    offs = torch.searchsorted(feed.sample, torch.arange(B + 1, dtype=torch.int32, device="cuda"), out_int32=True)
    rows = (feed.y, feed.v, feed.c)
    hip_ms = timed(lambda: train.surrogate_grad(model, x, rows, row_offset=offs), args.reps, args.warmup)
    theta = {k: torch.from_numpy(np.asarray(v, np.float32)).cuda().requires_grad_(True) for k, v in params.items()}
    x_rows = x[feed.sample.long()]
    torch_ms = timed(lambda: torch_surrogate_grad(spec, theta, x_rows, feed.y, feed.v, feed.c), args.reps, args.warmup)
    print("Bibtex batch %d, nIter %d: R = %d feed rows (%.2f per sample)" % (B, args.niter, R, R / B))
    print("  surrogate_grad (HIP)           median %.3f ms  min %.3f ms" % hip_ms)
    print("  torch double-backward autograd median %.3f ms  min %.3f ms" % torch_ms)
    print(json.dumps({"tool": "train_grad_time", "batch": B, "niter": args.niter, "rows": R, "hip_ms": hip_ms[0],
                      "hip_min_ms": hip_ms[1], "torch_ms": torch_ms[0], "torch_min_ms": torch_ms[1],
                      "speedup": torch_ms[0] / hip_ms[0]}))


if __name__ == "__main__":
    main()
