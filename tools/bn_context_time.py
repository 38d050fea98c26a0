"""Time the BatchNorm modes of the context producer (be_context.hip) and the fold of surrogate_grad:

  1. model.context(x, bn="moving") against model.context(x) (batch statistics) at the completion test batch (conv, B = 256)
     and at Bibtex with BatchNorm (B = 4096);
  2. train.surrogate_grad(..., bn_updates=1) against bn_updates=0 on the conv model at batch 70 with a feed of 4 rows per
     sample, and on Bibtex at batch 128 with 6 rows per sample.

Device events around each call, median of --reps calls after --warmup; prints one line per case and one JSON line.

    python tools/bn_context_time.py [--reps 50] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icnn_amd import picnn, train  # noqa: E402


def median_ms(fn, reps, warmup):
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


def models():
    rng = np.random.RandomState(0)
    cspec = picnn.ConvSpec()
    conv = picnn.ConvModel(cspec, picnn.init_conv_params(cspec, 1, "spread"))
    fspec = picnn.bibtex_spec()
    fc = picnn.FCModel(fspec, picnn.init_params(fspec, 1, "spread"))
    xc = lambda B: torch.from_numpy(rng.rand(B, cspec.H, cspec.W, 1).astype(np.float32)).cuda()        # noqa: E731
    xf = lambda B: torch.from_numpy((rng.rand(B, fspec.n_features) < 0.04).astype(np.float32)).cuda()  # noqa: E731
    return [("conv", conv, xc), ("bibtex", fc, xf)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    out = {}
    for name, model, make_x in models():
        B = 256 if name == "conv" else 4096
        x = make_x(B)
        tb = median_ms(lambda: model.context(x), args.reps, args.warmup)
        tm = median_ms(lambda: model.context(x, bn="moving"), args.reps, args.warmup)
        tu = median_ms(lambda: model.context(x, bn_updates=6), args.reps, args.warmup)
        print("%-6s B=%4d context: batch %.3f ms, moving %.3f ms, batch + 6 folds %.3f ms" % (name, B, tb, tm, tu))
        out["%s_context_B%d" % (name, B)] = dict(batch_ms=tb, moving_ms=tm, batch_fold6_ms=tu)
    for name, model, make_x in models():
        B, per = (70, 4) if name == "conv" else (128, 6)
        x = make_x(B)
        R = B * per
        rng = np.random.RandomState(1)
        n = model.spec.n_labels
        y = torch.from_numpy(rng.rand(R, n)).cuda()
        v = torch.from_numpy(rng.randn(R, n)).cuda()
        c = torch.from_numpy(rng.randn(R)).cuda()
        off = torch.arange(0, R + 1, per, dtype=torch.int32).cuda()
        t0 = median_ms(lambda: train.surrogate_grad(model, x, (y, v, c), row_offset=off), args.reps, args.warmup)
        t1 = median_ms(lambda: train.surrogate_grad(model, x, (y, v, c), row_offset=off, bn_updates=1), args.reps,
                       args.warmup)
        print("%-6s B=%4d R=%5d surrogate_grad: %.3f ms, with bn_updates=1 %.3f ms" % (name, B, R, t0, t1))
        out["%s_surrogate_B%d_R%d" % (name, B, R)] = dict(plain_ms=t0, fold_ms=t1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
