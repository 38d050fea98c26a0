"""Time the FICNN on the device (icnn_amd.ficnn, be_ficnn.hip, be_train_ficnn.hip) against a float32 torch-autograd
restatement of the same work on the same GPU (device events, median after warm-up):

    synthetic  synthetic_spec() at B = 100 (the training batch) and B = 400 (the plot grid): fg, gd.solve (K = 30) and the
               whole GDTrainer step, against torch autograd for E / dE/dy, the unrolled loop, and loss.backward through it
    large      FICNNSpec(1836, 159, (600, 600), head="linear") at B = 4096: us per fg and the fraction of the f32-MFMA
               roof (--roof, 157.3 TFLOP/s) that its 2 (2 n s_0 + s_0 s_1 + 2 n s_1 + s_0 s_1) flops per sample reach

Prints one line per case and a JSON line.

    python tools/ficnn_time.py [--reps 20] [--warmup 3] [--roof 157.3]
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

from icnn_amd import ficnn, gd, train  # noqa: E402

K, LR, MU = 30, 0.01, 0.9


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


def torch_energy(spec, theta, x, y):
    xy = torch.cat([x, y], 1)
    L, z = len(spec.szs), None
    for i in range(L + 1):
        a = xy @ theta["z_x%d/W" % i] + theta["z_x%d/b" % i]
        if i > 0:
            a = a + z @ theta["z_z%d_proj/W" % i]
        if i < L:
            z = torch.relu(a)
        else:
            last = a
    return z.sum(1) if spec.head == "sum" else last[:, 0]


def torch_fg(spec, theta, x, y):
    y = y.detach().requires_grad_(True)
    E = torch_energy(spec, theta, x, y)
    g, = torch.autograd.grad(E.sum(), y)
    return E, g


def torch_unroll(spec, theta, x, y0, create_graph):
    y, v = y0, 0
    for _ in range(K):
        if not create_graph:
            y = y.detach()
        y = y if y.requires_grad else y.requires_grad_(True)
        g, = torch.autograd.grad(torch_energy(spec, theta, x, y).sum(), y, create_graph=create_graph)
        prev = v
        v = MU * prev - LR * g
        y = y - MU * prev + (1.0 + MU) * v
    return y


def synthetic(B, reps, warmup, out):
    spec = ficnn.synthetic_spec()
    params = ficnn.make_convex(ficnn.init_params(spec, 0))
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.randn(B, 2).astype(np.float32)).cuda()
    t = torch.from_numpy((rng.rand(B, 1) > 0.5).astype(np.float32)).cuda()
    y = torch.full((B, 1), 0.5, dtype=torch.float64, device="cuda")
    model = ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()})
    ctx = model.context(x)
    theta = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in params.items()}
    res = {}
    res["fg"] = timed(lambda: model.fg(ctx, y), reps, warmup)
    res["fg_torch"] = timed(lambda: torch_fg(spec, theta, x, y.float()), reps, warmup)
    res["gd"] = timed(lambda: gd.solve(model, ctx, 0.5, K, LR, MU), reps, warmup)
    res["gd_torch"] = timed(lambda: torch_unroll(spec, theta, x, y.float(), False), reps, warmup)
    tr = ficnn.GDTrainer(model, B)
    tr.step(x, t)
    res["step"] = timed(lambda: tr.step(), reps, warmup)
    opt = torch.optim.Adam(list(theta.values()), lr=1e-3)

    def torch_step():
        opt.zero_grad()
        yK = torch_unroll(spec, theta, x, y.float(), True)
        loss = torch.mean((yK - t) ** 2)
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k, p in theta.items():
                if "proj" in k:
                    p.clamp_(min=0)
    res["step_torch"] = timed(torch_step, reps, warmup)
    for k in ("fg", "gd", "step"):
        print("synthetic B=%4d %-5s device %8.3f ms   torch %8.3f ms   x%.2f" % (B, k, res[k], res[k + "_torch"],
                                                                              res[k + "_torch"] / res[k]))
    out["synthetic_%d" % B] = res


def large(reps, warmup, roof_tflops, out):
    spec = ficnn.FICNNSpec(1836, 159, (600, 600), "linear")
    B = 4096
    rng = np.random.RandomState(1)
    params = ficnn.make_convex(ficnn.init_params(spec, 1))
    model = ficnn.FICNNModel(spec, params)
    x = torch.from_numpy(rng.rand(B, 1836).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.rand(B, 159)).cuda()
    ctx = model.context(x)
    theta = {k: torch.from_numpy(v).cuda() for k, v in params.items()}
    ms = timed(lambda: model.fg(ctx, y), reps, warmup)
    ms_torch = timed(lambda: torch_fg(spec, theta, x, y.float()), reps, warmup)
    n, s0, s1 = 159, 600, 600
    flops = 2.0 * B * (2 * n * s0 + s0 * s1 + 2 * n * s1 + s0 * s1)
    frac = flops / (ms * 1e-3) / (roof_tflops * 1e12)
    print("large B=4096 fg device %.1f us (%.2f%% of the f32-MFMA roof %.1f TFLOP/s)   torch autograd %.1f us (context "
          "included)" % (ms * 1e3, 100 * frac, roof_tflops, ms_torch * 1e3))
    out["large"] = {"fg_us": ms * 1e3, "roof_fraction": frac, "fg_torch_us": ms_torch * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--roof", type=float, default=157.3, help="f32 MFMA peak of the device in TFLOP/s")
    args = ap.parse_args()
    out = {}
    synthetic(100, args.reps, args.warmup, out)
    synthetic(400, args.reps, args.warmup, out)
    large(args.reps, args.warmup, args.roof, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
