"""Time pgd.solve (be_pgd.hip) with device events, median [min, max] of --reps calls after --warmup, against

    loop     what a caller can write without it: K x (model.fg + the float64 update and objective in torch)
    bundle   the fused bundle-entropy solve of the same samples (bundle_entropy.FusedSolver, FC; solveBatch's fused path
             without a callback for the conv model), variant pdipm: the other side of the comparison

at the two scripts' shapes -- bibtex FC, 10 samples, K = 10 / bundle nIter 10, and the conv model, 1 sample, K = 50 / bundle
nIter 30 -- and at the headline batch (bibtex FC, B = 4096, K = 10 / nIter 10).  Each candidate is warmed up and timed on
its own; "loop" and pgd.solve compute the same iteration (the loop's logarithms are torch's).  Reports only: nothing is
asserted.  Prints one line per case and a JSON line.

    python tools/pgd_step_time.py [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import bundle_entropy, pgd, picnn  # noqa: E402


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


def case(name, model, ctx, y0, K, n_iter, lr, reps, warmup, out):
    B = ctx.shape[0]
    res = {}
    res["pgd_solve"] = timed(lambda: pgd.solve(model, ctx, y0, K, lr), reps, warmup)

    def loop():
        y = y0.clamp(pgd.LO, pgd.HI)
        trace = []
        for _ in range(K):
            yf = y.float().double()
            E, g = model.fg(ctx, yf)
            ly, l1 = torch.log(yf), torch.log(1.0 - yf)
            trace.append(E.double() + (yf * ly + (1.0 - yf) * l1).sum(dim=1))
            y = (y - lr * ((g.double() + ly) - l1)).clamp(pgd.LO, pgd.HI)
        return y, torch.stack(trace)
    res["loop"] = timed(loop, reps, warmup)
    if isinstance(model, picnn.FCModel):
        solver = bundle_entropy.FusedSolver(model, B, n_iter=n_iter, variant="pdipm")
        res["bundle"] = timed(lambda: solver.solve(ctx, y0), reps, warmup)
    else:
        res["bundle"] = timed(lambda: bundle_entropy.solveBatch(f=model, ctx=ctx, y0=y0.clone(), nIter=n_iter, variant="pdipm",
                                                                native=True, check=False), reps, warmup)
    print("%-10s B=%4d K=%d nIter=%d  ms median [min, max]" % (name, B, K, n_iter))
    for k in ("pgd_solve", "loop", "bundle"):
        print("    %-10s %8.3f [%.3f, %.3f]" % ((k,) + tuple(res[k])))
    out["%s_%d" % (name, B)] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {}
    rng = np.random.RandomState(0)
    bib = picnn.bibtex_spec()
    fc = picnn.FCModel(bib, picnn.init_params(bib, 0, "spread"), "cuda")
    for B in (10, 4096):
        ctx = fc.context(torch.from_numpy((rng.rand(B, bib.n_features) < 0.04).astype(np.float32)))
        y0 = torch.full((B, bib.n_labels), 0.5, dtype=torch.float64, device="cuda")
        case("bibtex", fc, ctx, y0, 10, 10, 0.01, a.reps, a.warmup, out)
    cs = picnn.ConvSpec()
    conv = picnn.ConvModel(cs, picnn.init_conv_params(cs, 0, "spread"))
    ctx = conv.context(torch.from_numpy(rng.rand(1, cs.H, cs.W, 1).astype(np.float32)).cuda())
    y0 = torch.from_numpy(np.repeat((0.2 + 0.6 * rng.rand(cs.n_labels))[None], 1, axis=0)).cuda()
    case("conv", conv, ctx, y0, 50, 30, 0.01, a.reps, a.warmup, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
