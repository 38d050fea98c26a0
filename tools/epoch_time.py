#!/usr/bin/env python3
"""What keeping the best model by test F1 costs per test phase, on the multi-label model with the whole
test split as one evaluation batch (E = 2515):

    device   one replay of a captured [BundleTrainer.evaluate, BestKeeper.offer_macro_f1]: the F1, the comparison and the
             snapshot stay on the device
    host     the same decision made on the host: a replay of the captured evaluate, a synchronisation, eval_macro_f1() and,
             when the F1 is better, host_params()

each once with every offer kept and once with every offer declined.  Device events round the whole sequence (the host part of
`host` lies between them), median [min, max] of --reps after --warmup.

    python tools/epoch_time.py [--eval-batch 2515] [--reps 20] [--warmup 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import picnn, train  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return "%.3f [%.3f, %.3f] ms" % (float(np.median(ms)), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval-batch", type=int, default=2515)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    spec, E = picnn.bibtex_spec(), a.eval_batch
    rng = np.random.RandomState(0)
    model = picnn.FCModel(spec, picnn.init_params(spec, 0, "spread"), "cuda")
    trainer = train.BundleTrainer(model, a.batch, n_iter=10, loss="xent", lr=1e-3, eval_batch=E)
    keeper = train.BestKeeper(trainer, mode="max", start=0.0)
    xe = torch.from_numpy(rng.rand(E, spec.n_features).astype(np.float32)).cuda()
    te = torch.from_numpy((rng.rand(E, spec.n_labels) < 0.05).astype(np.float64)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        trainer.evaluate(xe, te)
        keeper.offer_macro_f1(trainer.eval_f1_tallies)
    torch.cuda.current_stream().wait_stream(s)
    plain, kept = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(plain):
        trainer.evaluate(None, None)
    with torch.cuda.graph(kept):
        trainer.evaluate(None, None)
        keeper.offer_macro_f1(trainer.eval_f1_tallies)
    torch.cuda.synchronize()
    f1 = trainer.eval_macro_f1()
    print("multi-label model %s, E = %d, theta %d floats, arena %d floats, test macro F1 %.4f"
          % (spec.szs, E, trainer.opt.n, trainer.opt.arena.numel(), f1))

    def device(keep):
        def fn():
            if keep:
                keeper.best.fill_(-1.0)                 # every offer is better
            kept.replay()
        return fn

    def host(keep):
        state = {"best": 2.0}

        def fn():
            if keep:
                state["best"] = -1.0
            plain.replay()
            torch.cuda.synchronize()
            f = trainer.eval_macro_f1()
            if f > state["best"]:
                state["best"] = f
                state["params"] = trainer.host_params()
        return fn
    print("evaluate alone (captured)          %s" % timed(plain.replay, a.reps, a.warmup))
    for keep in (True, False):
        what = "kept    " if keep else "declined"
        if not keep:
            keeper.best.fill_(2.0)                      # no offer is better
        print("device, every offer %s       %s" % (what, timed(device(keep), a.reps, a.warmup)))
        print("host,   every offer %s       %s" % (what, timed(host(keep), a.reps, a.warmup)))
    torch.cuda.synchronize()
    print("offers %d, kept %d" % (keeper.offers, keeper.kept))


if __name__ == "__main__":
    main()
