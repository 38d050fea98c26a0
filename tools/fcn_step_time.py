"""Time the FCN baseline's training step (fcn.FCNTrainer) at B = 70, k = 32, 64 x 32:

    eager      the whole step enqueued from Python (icnn_be_fcn_step: forward, backward, gradients, update; 16 launches)
    captured   the step captured once in a CUDA graph and replayed
    launches   forward, backward, grads, update alone (events around each, eager)
    evaluate   the test phase on --eval-batch images
    torch      the YARDSTICK, which is not the code under test: the same net written with torch.nn.functional on torch-ROCm in
               the same process -- forward, backward(), torch.optim.Adam.step(), eager.  torch_error is set instead when
               torch's convolution backend is unavailable or fails on the machine.
    ratio      eager_ms / torch_ms: the device step should take no longer (<= 1.0)

    python tools/fcn_step_time.py [--steps 200] [--warmup 20] [--batch 70] [--k 32] [--H 64] [--W 32] [--eval-batch 50]
Two runs in one process; prints one JSON line per run.  Kernel times come from a kernel trace of this tool in a run of its own
(--no-torch keeps the yardstick's kernels out of it)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import fcn  # noqa: E402


def _ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def torch_step(spec, params, x, t, lr):
    """the same net on torch's own kernels: returns the step as a callable"""
    P = {n: torch.nn.Parameter(torch.from_numpy(a).cuda()) for n, a in params.items()}
    opt = torch.optim.Adam(list(P.values()), lr=lr)
    conv, up = dict(stride=2, dilation=2, padding=2), dict(stride=2, padding=1, output_padding=1)

    def step():
        h = x
        for name in ("conv1", "conv2", "conv3"):
            h = F.relu(F.conv2d(h, P[name + ".weight"], P[name + ".bias"], **conv))
        for name in ("up1", "up2", "up3"):
            h = F.relu(F.conv_transpose2d(h, P[name + ".weight"], P[name + ".bias"], **up))
        h = F.conv_transpose2d(h, P["up4.weight"], P["up4.bias"])
        loss = (255 * (h - t)).pow(2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    return step


def run(args):
    B, H, W = args.batch, args.H, args.W
    spec = fcn.FCNSpec(H, W, args.k)
    tr = fcn.FCNTrainer(fcn.FCNModel(spec, seed=1), B, eval_batch=args.eval_batch or None)
    rng = np.random.RandomState(1)
    x, t = rng.uniform(0, 1, (B, H, W)).astype(np.float32), rng.uniform(0, 1, (B, H, W)).astype(np.float32)
    tr.x.copy_(torch.from_numpy(x).view(B, H, W, 1))
    tr.t.copy_(torch.from_numpy(t).view(B, H * W))
    out = {"batch": B, "k": args.k, "H": H, "W": W, "params": tr.model.n}
    out["eager_ms"] = _ms(tr.step, args.steps, args.warmup)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.step()
    out["captured_ms"] = _ms(g.replay, args.steps, args.warmup)
    out["launches_ms"] = {name: _ms(getattr(tr, name), args.steps, args.warmup) for name in ("forward", "backward", "grads", "update")}
    if args.eval_batch:
        out["evaluate_ms"] = _ms(tr.evaluate, args.steps, args.warmup)
    assert np.isfinite(tr.loss.item())
    if not args.no_torch:
        try:
            step = torch_step(spec, fcn.init_params(spec, 1), torch.from_numpy(x).cuda().view(B, 1, H, W),
                              torch.from_numpy(t).cuda().view(B, 1, H, W), tr.lr)
            out["torch_ms"] = _ms(step, args.steps, args.warmup)
            out["ratio"] = out["eager_ms"] / out["torch_ms"]
        except RuntimeError as e:
            out["torch_error"] = str(e).splitlines()[0][:200]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--W", type=int, default=32)
    ap.add_argument("--eval-batch", type=int, default=50)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    for _ in range(2):
        print(json.dumps(run(args)))


if __name__ == "__main__":
    main()
