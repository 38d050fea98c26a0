"""Time the conv-PICNN training gradient (icnn_amd.train.surrogate_grad, be_train_conv.hip) on the completion model with the
feed of a real solve (completion/icnn_ebundle.py:200-335) against what a user has without it: the network restated in torch
and differentiated twice by autograd (create_graph=True), float32, same device, same rows.  Device events around each
call; prints the row count R, both medians and one JSON line.

    python tools/train_grad_conv_time.py [--batch 70] [--niter 30] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icnn_amd import bundle_entropy, picnn, train  # noqa: E402

PAD = {8: 2, 4: 1, 3: 1}


def _conv(inp, W, b, stride):
    out = Fn.conv2d(inp.permute(0, 3, 1, 2).contiguous(), W.permute(3, 2, 0, 1).contiguous(), b, stride=stride,
                    padding=PAD[W.shape[0]])
    return out.permute(0, 2, 3, 1)


def _bn(v, g, b, dims):
    mean = v.mean(dim=dims, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=dims, keepdim=True)
    return (v - mean) / torch.sqrt(var + 1e-5) * g + b


def torch_surrogate_grad(theta, x_rows, y, v, c, H, W):
    """completion/icnn_ebundle.py:337-452 in torch (float32) on the gathered rows, BatchNorm over them, double backward."""
    R = y.shape[0]
    yt = y.float().reshape(R, H, W, 1).requires_grad_(True)
    us, prev = [], x_rows
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        prev = _bn(torch.relu(_conv(prev, theta["u%d/W" % l], theta["u%d/b" % l], s)), theta["u%d/bn/gamma" % l],
                   theta["u%d/bn/beta" % l], (0, 1, 2))
        us.append(prev)
    u3 = _bn(torch.relu(prev.reshape(R, -1) @ theta["u3/W"] + theta["u3/b"]), theta["u3/bn/gamma"], theta["u3/bn/beta"], (0,))
    prevU, prevZ, y_red = x_rows, None, yt
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        acc = _conv(prevU, theta["z%d_u/W" % l], theta["z%d_u/b" % l], s)
        if l > 0:
            gate = torch.relu(_conv(prevU, theta["z%d_zu_u/W" % l], theta["z%d_zu_u/b" % l], 1))
            acc = acc + _conv(prevZ * gate, theta["z%d_zu_proj/W" % l], None, s)
        yu = _conv(prevU, theta["z%d_yu_u/W" % l], theta["z%d_yu_u/b" % l], 1)
        acc = acc + _conv(y_red * yu, theta["z%d_yu/W" % l], None, s)
        y_red = _conv(y_red, theta["z%d_y_red/W" % l], theta["z%d_y_red/b" % l], s)
        prevZ, prevU = torch.relu(acc), us[l]
    prevZ, prevU = prevZ.reshape(R, -1), prevU.reshape(R, -1)
    for l in (3, 4):
        gate = torch.relu(prevU @ theta["z%d_zu_u/W" % l] + theta["z%d_zu_u/b" % l])
        z = (prevZ * gate) @ theta["z%d_zu_proj/W" % l] + prevU @ theta["z%d_u/W" % l] + theta["z%d_u/b" % l]
        prevZ, prevU = (torch.relu(z) if l == 3 else z), u3
    E = prevZ.reshape(-1)
    dEdy, = torch.autograd.grad(E.sum(), yt, create_graph=True)
    F = c.float() * E + (dEdy.reshape(R, -1) * v.float()).sum(dim=1)
    names = [k for k in theta if not k.startswith("u4/") and not k.startswith("z2_y_red/")]    # these do not reach F
    return torch.autograd.grad(F.sum(), [theta[k] for k in names])


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=70)
    ap.add_argument("--niter", type=int, default=30)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    spec = picnn.ConvSpec()
    params = picnn.init_conv_params(spec, 0, "spread")
    B = args.batch
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
    labels = rng.rand(B, spec.n_labels)
    model = picnn.ConvModel(spec, params, "cuda:0")
    y0 = torch.from_numpy(np.repeat((0.2 + 0.6 * rng.rand(spec.n_labels))[None], B, axis=0)).cuda()
    res = bundle_entropy.FusedSolver(model, B, args.niter, "dual").solve(model.context(x), y0)
    feed = bundle_entropy.implicit_feed(res, labels, "mse")
    R = int(feed.sample.numel())
    offs = torch.searchsorted(feed.sample, torch.arange(B + 1, dtype=torch.int32, device="cuda"), out_int32=True)
    rows = (feed.y, feed.v, feed.c)
    hip_ms = timed(lambda: train.surrogate_grad(model, x, rows, row_offset=offs), args.reps, args.warmup)
    theta = {k: torch.from_numpy(np.asarray(v, np.float32)).cuda().requires_grad_(True) for k, v in params.items()}
    x_rows = x[feed.sample.long()]
    torch_ms = timed(lambda: torch_surrogate_grad(theta, x_rows, feed.y, feed.v, feed.c, spec.H, spec.W), args.reps,
                     args.warmup)
    print("completion batch %d, nIter %d: R = %d feed rows (%.2f per sample)" % (B, args.niter, R, R / B))
    print("  surrogate_grad (HIP)           median %.3f ms  min %.3f ms" % hip_ms)
    print("  torch double-backward autograd median %.3f ms  min %.3f ms" % torch_ms)
    print(json.dumps({"tool": "train_grad_conv_time", "batch": B, "niter": args.niter, "rows": R, "hip_ms": hip_ms[0],
                      "hip_min_ms": hip_ms[1], "torch_ms": torch_ms[0], "torch_min_ms": torch_ms[1],
                      "speedup": torch_ms[0] / hip_ms[0]}))


if __name__ == "__main__":
    main()
