"""Time one bundle-entropy training step three ways on the shapes of DESIGN.md §11 (Bibtex at batch 128 / nIter 10, the
completion conv PICNN at batch 70 / nIter 5): the host-composed step (tools/train_step_time.py's device step: solve ->
fg_evaluations() -> implicit_feed -> surrogate_grad -> DeviceAdam.step, two host waits), train.BundleTrainer.step eager, and
the same step captured in a graph and replayed -- all three with the same solver variant, from the same initial weights.
Device events around each repetition, warm-up first; prints the median, min and max in ms, the row count R of each
measurement's last step, the padded-to-true row ratio R_cap / R of the trainer's feed, and one JSON line per model.  The
weights move with every timed step and R with them: --lr 0 keeps them (same work in the update, no change).

--skip-on-error builds the trainer columns with skip_on_error=True (the gate, the shadow of the BatchNorm
statistics, the gated update and the gated restore ride along; nothing is skipped, the solves are clean).  --eval E ... also
times one train.BundleTrainer.evaluate() of the Bibtex trainer at each E (eager and captured).

    python tools/bundle_step_time.py [--reps 20] [--warmup 3] [--only bibtex|conv] [--variant dual|pdipm] [--lr 1e-3]
                                     [--mode host|eager|captured ...] [--skip-on-error] [--eval 128 2515]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import bundle_entropy, train  # noqa: E402
from tools.train_step_time import _problem, _timed  # noqa: E402


def _host_grad(model, x, y, n_iter, loss, conv, variant, seen):
    """tools/train_step_time.py::_grad with the solver variant of the trainer columns; seen["rows"]: the feed's row count"""
    B = x.shape[0]
    solver = bundle_entropy.FusedSolver(model, B, n_iter, variant)
    res = solver.solve(model.context(x), 0.5)
    if conv:
        model.context(x, bn_updates=res.fg_evaluations())
    feed = bundle_entropy.implicit_feed(res, y, loss)
    seen["rows"] = int(feed.y.shape[0])
    return train.surrogate_grad(model, x, feed, bn_updates=1 if conv else 0, flat=True)


def _side_stream(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)


def run_eval(E, reps, warmup, variant):
    """one evaluate() of the Bibtex trainer at eval batch E, from the initial weights: eager and captured"""
    import numpy as np
    spec, params, Model, x, y, n_iter, loss = _problem("bibtex")
    tr = train.BundleTrainer(Model(spec, params, "cuda"), x.shape[0], n_iter=n_iter, loss=loss, variant=variant, eval_batch=E)
    rng = np.random.RandomState(E)
    xe = torch.from_numpy((rng.rand(E, spec.n_features) < 0.04).astype(np.float32)).cuda()
    te = torch.from_numpy((rng.rand(E, spec.n_labels) < 0.05).astype(np.float64)).cuda()
    _side_stream(lambda: tr.evaluate(xe, te))
    out = {"model": "bibtex", "variant": variant, "eval_batch": E}
    out["evaluate_eager_ms"] = _timed(lambda: tr.evaluate(None, None), reps, warmup)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr.evaluate(None, None)
    out["evaluate_captured_ms"] = _timed(graph.replay, reps, warmup)
    torch.cuda.synchronize()
    out.update(eval_loss=float(tr.eval_loss.item()), eval_macro_f1=tr.eval_macro_f1())
    for k in ("eager", "captured"):
        t = out["evaluate_%s_ms" % k]
        print("bibtex  %-7s evaluate E %-5d %-9s median %8.3f ms  [%.3f, %.3f]" % (variant, E, k, t["median"], t["min"], t["max"]))
    print(json.dumps(out))
    return out


def run(which, reps, warmup, variant, lr, modes, skip=False):
    conv = which == "conv"
    spec, params, Model, x, y, n_iter, loss = _problem(which)
    B = x.shape[0]
    yd = torch.from_numpy(y).cuda()
    out = {"model": which, "variant": variant, "lr": lr, "skip_on_error": skip}
    kw = {"skip_on_error": True} if skip else {}
    if "host" in modes:          # the host-composed step: the same solver variant, the same initial weights
        host_model = Model(spec, params, "cuda")
        host_opt = train.DeviceAdam(host_model, lr=lr)
        seen = {}
        out["step_host_composed_ms"] = _timed(
            lambda: host_opt.step(_host_grad(host_model, x, y, n_iter, loss, conv, variant, seen)), reps, warmup)
        out["rows_host_composed"] = seen["rows"]
    if "eager" in modes:
        tr = train.BundleTrainer(Model(spec, params, "cuda"), B, n_iter=n_iter, loss=loss, variant=variant, lr=lr, **kw)
        tr.step(x, yd)
        out["step_trainer_eager_ms"] = _timed(lambda: tr.step(None, None), reps, warmup - 1)
        out["rows_trainer_eager"] = int(tr.rows.item())
        out["row_cap"] = tr.feed.row_cap
    if "captured" in modes:
        cap = train.BundleTrainer(Model(spec, params, "cuda"), B, n_iter=n_iter, loss=loss, variant=variant, lr=lr, **kw)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            cap.step(x, yd)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap.step(None, None)
        out["step_trainer_captured_ms"] = _timed(graph.replay, reps, warmup - 1)
        torch.cuda.synchronize()
        out.update(rows_trainer_captured=int(cap.rows.item()), row_cap=cap.feed.row_cap, loss=float(cap.loss.item()),
                   fg_evals=int(cap.fg_evals.item()))
        if skip:
            out.update(went=int(cap.went.item()), skipped=int(cap.skipped.item()), status_or=int(cap.status_or.item()))
    for k in ("host_composed", "trainer_eager", "trainer_captured"):
        t = out.get("step_%s_ms" % k)
        if t:
            print("%-7s %-7s lr %-6g %-18s median %8.3f ms  [%.3f, %.3f]  rows of the last step %d"
                  % (which, variant, lr, k, t["median"], t["min"], t["max"], out["rows_" + k]))
    if "row_cap" in out:
        rows = out.get("rows_trainer_captured", out.get("rows_trainer_eager"))
        print("%-7s R_cap %d, R_cap / R = %.2f" % (which, out["row_cap"], out["row_cap"] / max(rows, 1)))
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["bibtex", "conv"])
    ap.add_argument("--variant", choices=["dual", "pdipm"], default="pdipm")
    ap.add_argument("--lr", type=float, default=1e-3, help="0 keeps the weights, and so the row count, where they start")
    ap.add_argument("--mode", choices=["host", "eager", "captured"], action="append",
                    help="measure only these (repeatable; e.g. one mode under a kernel profiler); default all three")
    ap.add_argument("--skip-on-error", action="store_true", help="the trainer columns with skip_on_error=True")
    ap.add_argument("--eval", type=int, nargs="+", default=[], metavar="E",
                    help="also time evaluate() of the Bibtex trainer at these eval batches")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for which in ([a.only] if a.only else ["bibtex", "conv"]):
        run(which, a.reps, a.warmup, a.variant, a.lr, a.mode or ["host", "eager", "captured"], a.skip_on_error)
    for E in a.eval:
        run_eval(E, a.reps, a.warmup, a.variant)


if __name__ == "__main__":
    main()
