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

--draw times one TRAINING iteration of the same model at --batch (128) two ways instead, on a seeded
training set of --n-train rows:

    host     the minibatch drawn on the host: np.random randint, the upload of the index tensor, two torch gathers, two
             copies into trainer.x / trainer.true_y, then one replay of the captured BundleTrainer.step
    device   one iteration of a replayed train.EpochRunner chain of --chain iterations of [icnn_be_dataset_draw, step,
             icnn_be_log_row]: the replay's time over --chain

and, for scale, the captured step alone and the draw alone (a graph of 100 draws, its time over 100).  Device events round
each iteration (the host's part of `host` lies between them) or each chain replay; the two ways alternate in --rounds blocks
of --reps; median [min, max] over all of a way's samples after --warmup.

    python tools/epoch_time.py --draw [--batch 128] [--n-train 4880] [--chain 10] [--reps 20] [--rounds 3] [--warmup 3]
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


def samples(fn, reps, per=1):
    """device-event times of `reps` calls of fn, each over `per`, in ms"""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / per)
    return ms


def spread(ms):
    return "%.4f [%.4f, %.4f] ms" % (float(np.median(ms)), min(ms), max(ms))


def draw_mode(a):
    """one training iteration with the minibatch drawn on the host against one of a replayed EpochRunner chain"""
    spec, B, N, K = picnn.bibtex_spec(), a.batch, a.n_train, a.chain
    rng = np.random.RandomState(0)
    X = rng.rand(N, spec.n_features).astype(np.float32)
    Y = (rng.rand(N, spec.n_labels) < 0.05).astype(np.float64)

    def trainer():
        return train.BundleTrainer(picnn.FCModel(spec, picnn.init_params(spec, 0, "spread"), "cuda"), B, n_iter=10, loss="xent",
                                   lr=1e-3)
    # ---- host: the examples' loop before the dataset moved to the device
    th = trainer()
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    host_rng = np.random.RandomState(0)

    def host_batch():
        idx = torch.from_numpy(host_rng.randint(N, size=B)).cuda()
        th.x.copy_(Xd[idx])
        th.true_y.copy_(Yd[idx])
    host_batch()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        th.step(None, None)
    torch.cuda.current_stream().wait_stream(s)
    step_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(step_graph):
        th.step(None, None)

    def host_iteration():
        host_batch()
        step_graph.replay()
    # ---- device: [draw, step, log] x K as one graph
    td = trainer()
    data = train.DeviceDataset((X, Y), seed=0)
    log = train.StepLog([("loss", td.loss)], K * (a.reps + a.warmup + 2))      # read once per block of replays
    runner = train.EpochRunner(td, data, K, log=log)
    runner.run()
    runner.run()                                           # captured here
    log.read()
    # ---- the draw alone
    alone = train.DeviceDataset((X, Y), seed=1)
    xb, yb = torch.empty_like(td.x), torch.empty_like(td.true_y)
    alone.draw_into(xb, yb)
    torch.cuda.synchronize()
    draws = torch.cuda.CUDAGraph()
    with torch.cuda.graph(draws):
        for _ in range(100):
            alone.draw_into(xb, yb)
    for fn in (host_iteration, runner.run, step_graph.replay, draws.replay):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    host_ms, dev_ms = [], []
    for _ in range(a.rounds):                              # alternating blocks: both ways see the same machine
        host_ms += samples(host_iteration, a.reps)
        dev_ms += samples(runner.run, a.reps, per=K)
        log.read()
    print("multi-label model %s, batch %d, %d training rows (x row %d B, y row %d B), chain of %d, %d x %d samples per way"
          % (spec.szs, B, N, 4 * spec.n_features, 8 * spec.n_labels, K, a.rounds, a.reps))
    print("host draw + captured step, per iteration      %s" % spread(host_ms))
    print("EpochRunner chain replay, per iteration       %s" % spread(dev_ms))
    print("captured step alone                           %s" % spread(samples(step_graph.replay, a.reps)))
    print("icnn_be_dataset_draw alone (graph of 100 / 100) %s" % spread(samples(draws.replay, a.reps, per=100)))
    # the set is noise (random features, random labels): a solve may report an error late in such a run, on either trainer
    print("status OR of the last step: host way %d, device way %d; dataset status %d"
          % (int(th.status_or.item()), int(td.status_or.item()), data.status))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval-batch", type=int, default=2515)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--draw", action="store_true")
    ap.add_argument("--n-train", type=int, default=4880)
    ap.add_argument("--chain", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.draw:
        return draw_mode(a)
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
