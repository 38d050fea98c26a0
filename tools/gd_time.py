"""Time the back-optimisation inference (icnn_amd.gd.solve, be_gd.hip) and its training gradient (train.unrolled_grad) against
what a user can write without them, on the same device with device events (median after warm-up):

    fc     Bibtex at B = 128 / 1024 / 4096, K = 30: gd.solve against K calls of model.fg plus the float32 update in torch
    conv   completion at B = 70 / 256, K = 30: the same two forms
    grad   unrolled_grad at Bibtex 128 x 30 and completion 70 x 30 against float32 torch autograd through the unrolled
           network (create_graph=True), the network restated in torch (tests/train_ref.py, tests/train_conv_ref.py)

Prints one line per case and a JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python
tools/gd_time.py --reps 5` in a separate run.

    python tools/gd_time.py [--reps 20] [--warmup 3] [--only fc,conv,grad]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from icnn_amd import gd, picnn, train  # noqa: E402

K = 30


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
    return float(np.median(times))


def loop_of_fg(model, ctx, y0, lr, mu):
    """what a caller has without gd.solve: K evaluations through model.fg and the float32 update in torch"""
    dev = ctx.device
    y = y0.float()
    v = torch.zeros_like(y)
    lr32, mu32, c1 = (torch.tensor(c, dtype=torch.float32, device=dev) for c in (lr, mu, 1.0 + mu))
    for _ in range(K):
        _, g = model.fg(ctx, y.double().contiguous())
        mv = mu32 * v
        vn = mv - lr32 * g
        y = (y - mv) + c1 * vn
        v = vn
    return y


def inference_cases(which, batches, reps, warmup, out):
    rng = np.random.RandomState(0)
    if which == "fc":
        spec, lr, mu = picnn.bibtex_spec(), 0.01, 0.3
        params = picnn.init_params(spec, 0, "spread")
        model = picnn.FCModel(spec, params, "cuda")
    else:
        spec, lr, mu = picnn.ConvSpec(), 0.01, 0.9
        params = picnn.init_conv_params(spec, 0, "spread")
        model = picnn.ConvModel(spec, params)
    for B in batches:
        if which == "fc":
            x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
            y0 = torch.full((B, spec.n_labels), 0.5, dtype=torch.float64, device="cuda")
        else:
            x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
            y0 = torch.from_numpy(np.repeat((0.2 + 0.6 * rng.rand(spec.n_labels))[None], B, axis=0)).cuda()
        ctx = model.context(x)
        t_gd = timed(lambda: gd.solve(model, ctx, y0, K, lr, mu), reps, warmup)
        t_loop = timed(lambda: loop_of_fg(model, ctx, y0, lr, mu), reps, warmup)
        y, _, _ = gd.solve(model, ctx, y0, K, lr, mu)
        same = bool(torch.equal(y, loop_of_fg(model, ctx, y0, lr, mu).double()))
        print("%-4s B = %4d K = %d: gd.solve %8.3f ms   loop of fg + torch update %8.3f ms   (x%.2f, same bits: %s)"
              % (which, B, K, t_gd, t_loop, t_loop / t_gd, same))
        out.append(dict(case=which, batch=B, n_iter=K, gd_solve_ms=t_gd, fg_loop_ms=t_loop, same_bits=same))


def torch_unrolled_grad(energy, theta, x, y0, t, lr, mu, scale):
    """float32 autograd through the unrolled network: the reference's graph"""
    y = y0.float().clone().requires_grad_(True)
    v = 0
    for _ in range(K):
        E = energy(theta, x, y)
        g, = torch.autograd.grad(E.sum(), y, create_graph=True)
        prev = v
        v = mu * prev - lr * g
        y = y - mu * prev + (1.0 + mu) * v
    loss = torch.mean(torch.square(scale * (y - t)))
    return torch.autograd.grad(loss, list(theta.values()), allow_unused=True)


def grad_cases(reps, warmup, out):
    import train_conv_ref
    import train_ref
    rng = np.random.RandomState(0)
    for which in ("fc", "conv"):
        if which == "fc":
            spec, lr, mu, B, scale = picnn.bibtex_spec(), 0.01, 0.3, 128, 1.0
            params = picnn.init_params(spec, 0, "spread")
            model = picnn.FCModel(spec, params, "cuda")
            x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
            y0 = torch.full((B, spec.n_labels), 0.5, dtype=torch.float64, device="cuda")
            t = torch.from_numpy((rng.rand(B, spec.n_labels) < 0.05).astype(np.float32)).cuda()

            def energy(theta, xx, yy):
                return train_ref.energy(spec, theta, xx, yy)[0]
            xr = x
        else:
            spec, lr, mu, B, scale = picnn.ConvSpec(), 0.01, 0.9, 70, 255.0
            params = picnn.init_conv_params(spec, 0, "spread")
            model = picnn.ConvModel(spec, params)
            x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
            y0 = torch.from_numpy(np.repeat((0.2 + 0.6 * rng.rand(spec.n_labels))[None], B, axis=0)).cuda()
            t = torch.from_numpy(rng.rand(B, spec.n_labels).astype(np.float32)).cuda()

            def energy(theta, xx, yy):
                return train_conv_ref._forward(theta, xx, yy.reshape(-1, spec.H, spec.W, 1))[0]
            xr = x
        ctx = model.context(x)
        y, traj, _ = gd.solve(model, ctx, y0, K, lr, mu, trajectory=True)
        ybar = 2.0 * scale ** 2 * (y - t.double()) / y.numel()

        def ours():
            train.unrolled_grad(model, x, traj, ybar, lr, mu, flat=True)

        def whole_step():
            c = model.context(x)
            yy, tr, _ = gd.solve(model, c, y0, K, lr, mu, trajectory=True)
            train.unrolled_grad(model, x, tr, 2.0 * scale ** 2 * (yy - t.double()) / yy.numel(), lr, mu, flat=True)
        theta = {k: torch.tensor(np.asarray(p, np.float32), device="cuda", requires_grad=True) for k, p in params.items()}
        t_ours = timed(ours, reps, warmup)
        t_step = timed(whole_step, reps, warmup)
        t_torch = timed(lambda: torch_unrolled_grad(energy, theta, xr, y0, t, lr, mu, scale), max(3, reps // 4), 1)
        print("grad %-4s %d x %d: unrolled_grad %8.3f ms   (context + gd.solve + unrolled_grad %8.3f ms)   "
              "torch autograd through the unroll %8.3f ms   (x%.1f)" % (which, B, K, t_ours, t_step, t_torch, t_torch / t_step))
        out.append(dict(case="grad_" + which, batch=B, n_iter=K, unrolled_grad_ms=t_ours, whole_step_ms=t_step,
                        torch_autograd_ms=t_torch))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="fc,conv,grad")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    only = args.only.split(",")
    out = []
    if "fc" in only:
        inference_cases("fc", (128, 1024, 4096), args.reps, args.warmup, out)
    if "conv" in only:
        inference_cases("conv", (70, 256), args.reps, args.warmup, out)
    if "grad" in only:
        grad_cases(args.reps, args.warmup, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
