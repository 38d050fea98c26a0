"""The reference's solver comparison (multi-label-cls/ebundle-vs-gd.py, completion/ebundle-iter.py) on the device: the
bundle-entropy solve's entropy-scaled objective mean(E - H(y)) per iteration against projected gradient descent on the same
objective at lr 0.1, 0.01 and 0.001 -- the data of the paper's convergence figure --, and the solve's own duality gap.

    python examples/ebundle_vs_gd.py [--model fc|conv] [--seed 0] [--variant pdipm|dual]
                                     [--dataset bibtex|bookmarks|delicious] [--layerSizes 600 [600]]

--model fc    the multi-label script's settings: 10 samples, bundle nIter 10, PGD 10 iterations from y0 = 0.5, on a network
              of the dataset's shape (bibtex 1836 features / 159 labels, bookmarks 2150 / 208, delicious 500 / 983) with the
              hidden widths --layerSizes (the script's own default is 600 600; the label count is appended).  Shapes whose
              16-sample evaluation tile outgrows the LDS run on tiles of 8 or 4 rows (model.tile_rows is printed)
--model conv  the completion script's: 1 sample, bundle nIter 30, PGD 50 iterations from the mean image

The scripts load a trained checkpoint; here the model is a seeded random draw in the "spread" regime (pre-activations of the
size a trained model has) on seeded synthetic inputs, like the other examples.  Nothing is copied to the host per iteration:
the bundle trace comes from the solve's state (pgd.bundle_trace), the PGD traces from the loop itself (pgd.solve), and
pgd.gap = objective(y*) - dual_bound bounds how far y* is above the minimum.  No plotting: the traces are printed.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import bundle_entropy, pgd, picnn  # noqa: E402

LRS = (0.1, 0.01, 0.001)                      # ebundle-vs-gd.py:119
DATASETS = {"bibtex": picnn.bibtex_spec, "bookmarks": picnn.bookmarks_spec, "delicious": picnn.delicious_spec}


def row(values):
    return " ".join("%11.5f" % v for v in values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("fc", "conv"), default="fc")
    ap.add_argument("--variant", choices=("pdipm", "dual"), default="pdipm")     # the scripts import lib/bundle_entropy.py
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dataset", choices=sorted(DATASETS), default="bibtex")
    ap.add_argument("--layerSizes", type=int, nargs="+", default=[600])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.RandomState(a.seed)
    if a.model == "fc":
        spec = DATASETS[a.dataset](tuple(a.layerSizes))
        B, n_iter, K = 10, 10, 10                                                # ebundle-vs-gd.py:85,107,132
        model = picnn.FCModel(spec, picnn.init_params(spec, a.seed, "spread"), "cuda")
        x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32))
        y0 = np.full((B, spec.n_labels), 0.5)
    else:
        spec = picnn.ConvSpec()
        B, n_iter, K = 1, 30, 50                                                 # ebundle-iter.py:81,110,139
        model = picnn.ConvModel(spec, picnn.init_conv_params(spec, a.seed, "spread"))
        x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
        y0 = np.repeat((0.2 + 0.6 * rng.rand(spec.n_labels))[None], B, axis=0)   # a mean image
    ctx = model.context(x)
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=y0.copy(), nIter=n_iter, variant=a.variant, native=True)
    obj, calls = pgd.bundle_trace(res)
    gap = pgd.gap(model, ctx, res)
    runs = {lr: pgd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, final=True) for lr in LRS}
    calls = int(calls.item())
    if a.model == "fc":
        print("%s %s: %d features, %d labels, evaluation tiles of %d rows"
              % (a.dataset, " ".join(map(str, a.layerSizes)), spec.n_features, spec.n_labels, model.tile_rows))
    print("%s, %d sample(s): mean entropy-scaled objective per iteration" % (a.model, B))
    print("bundle entropy (%s, %d of %d iterations)" % (a.variant, calls, n_iter))
    print("   ", row(obj[:calls].mean(dim=1).tolist()))
    for lr, (_, trace, final) in runs.items():
        print("PGD lr %g (%d iterations, then the final point)" % (lr, K))
        print("   ", row(trace.mean(dim=1).tolist() + [float(final.mean())]))
    print("duality gap of the bundle solve per sample: objective(y*) - dual bound")
    print("   ", row(gap.tolist()))


if __name__ == "__main__":
    main()
