"""Time the back-optimisation training step of the FC PICNNs (train.GDTrainer: context, gd.solve with its trajectory, the
fused feed of be_train_gd.hip, surrogate_grad, DeviceAdam.step) with device events, median [min, max] of --reps steps
after --warmup, eager and as one captured graph, against

    composed  the hand-composed step at the same commit: context, gd.solve, the torch elementwise ops (d, loss, ybar,
              coef * ybar, zeros, arange) inside train.unrolled_grad, DeviceAdam.step -- eager and captured
    torch     a float32 torch-autograd restatement on the same GPU: the unrolled loop with create_graph, loss.backward,
              torch.optim.Adam, the proj clamp (the baseline of DESIGN.md §12 and §14)

on the synthetic PICNN (picnn.synthetic_spec()) at B = 100 and B = 400, K = 30, lr 0.01, momentum 0.9, and on
picnn.bibtex_spec() at B = 128, K = 30, momentum 0.3.  Prints one line per case and a JSON line.

    python tools/gd_step_time.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import gd, picnn, train  # noqa: E402


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
    return [float(np.median(times)), float(np.min(times)), float(np.max(times))]


def captured(fn):
    """one call of fn as a graph; returns its replay"""
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph.replay


def torch_energy(spec, th, x, y):
    L = len(spec.szs)
    us, prev = [], x
    for i in range(L):
        u = prev @ th["u%d/W" % i] + th["u%d/b" % i]
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                mean = u.mean(dim=0)
                var = ((u - mean) ** 2).mean(dim=0)
                u = (u - mean) / torch.sqrt(var + 1e-5) * th["u%d/bn/gamma" % i] + th["u%d/bn/beta" % i]
        elif spec.relu_last_u:
            u = torch.relu(u)
        us.append(u)
        prev = u
    z = None
    for i in range(L + 1):
        prev = x if i == 0 else us[i - 1]
        a = (y * (prev @ th["z%d_yu_u/W" % i] + th["z%d_yu_u/b" % i])) @ th["z%d_yu/W" % i]
        a = a + prev @ th["z%d_u/W" % i] + th["z%d_u/b" % i]
        if i > 0:
            a = a + (z * torch.relu(prev @ th["z%d_zu_u/W" % i] + th["z%d_zu_u/b" % i])) @ th["z%d_zu_proj/W" % i]
        z = torch.relu(a) if i < L else a
    return z[:, 0]


def case(name, spec, params, B, K, lr, mu, reps, warmup, out):
    rng = np.random.RandomState(0)
    if spec.n_features > 100:
        x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
        t = torch.from_numpy((rng.rand(B, spec.n_labels) < 0.05).astype(np.float32)).cuda()
    else:
        x = torch.from_numpy(rng.randn(B, spec.n_features).astype(np.float32)).cuda()
        t = torch.from_numpy((rng.rand(B, spec.n_labels) > 0.5).astype(np.float32)).cuda()
    bn = 1 if spec.batchnorm else 0
    res = {}

    def model():
        return picnn.FCModel(spec, {k: v.copy() for k, v in params.items()}, "cuda")
    for mode in ("eager", "graph"):
        tr = train.GDTrainer(model(), B, n_iter=K, lr=lr, momentum=mu, bn_updates=bn)
        tr.step(x, t)
        res["fused_" + mode] = timed(tr.step if mode == "eager" else captured(tr.step), reps, warmup)
        m = model()
        opt = train.DeviceAdam(m)
        inv = float(np.float32(1.0) / np.float32(B * spec.n_labels))

        def composed():
            ctx = m.context(x)
            yK, traj, _ = gd.solve(m, ctx, 0.5, K, lr, mu, trajectory=True)
            d = yK.to(torch.float32) - t
            loss = torch.mean(d * d)
            ybar = (d * 2.0) * inv
            opt.step(train.unrolled_grad(m, x, traj, ybar.to(torch.float64), lr, mu, bn_updates=bn, flat=True))
            return loss
        composed()
        res["composed_" + mode] = timed(composed if mode == "eager" else captured(composed), reps, warmup)
    th = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in params.items()}
    adam = torch.optim.Adam(list(th.values()), lr=1e-3)

    def torch_step():
        adam.zero_grad()
        y, v = torch.full((B, spec.n_labels), 0.5, device="cuda", requires_grad=True), 0
        for _ in range(K):
            g, = torch.autograd.grad(torch_energy(spec, th, x, y).sum(), y, create_graph=True)
            prev = v
            v = mu * prev - lr * g
            y = y - mu * prev + (1.0 + mu) * v
        torch.mean((y - t) ** 2).backward()
        adam.step()
        with torch.no_grad():
            for k, p in th.items():
                if "proj" in k:
                    p.clamp_(min=0)
    res["torch"] = timed(torch_step, reps, warmup)
    print("%-16s B=%4d K=%d  ms median [min, max]" % (name, B, K))
    for k in ("fused_eager", "composed_eager", "fused_graph", "composed_graph", "torch"):
        print("    %-15s %8.3f [%.3f, %.3f]" % ((k,) + tuple(res[k])))
    out["%s_%d" % (name, B)] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    out = {}
    syn = picnn.synthetic_spec()
    syn_params = picnn.make_convex(picnn.init_params(syn, 0), divisor=10)
    for B in (100, 400):
        case("synthetic", syn, syn_params, B, 30, 0.01, 0.9, args.reps, args.warmup, out)
    bib = picnn.bibtex_spec()
    case("bibtex", bib, picnn.init_params(bib, 0, "spread"), 128, 30, 0.01, 0.3, args.reps, args.warmup, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
