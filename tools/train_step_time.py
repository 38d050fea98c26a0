"""Time the parameter update of a PICNN training step: the documented host path (TFAdam.step -> picnn.project through the
host -> model.repack) against train.DeviceAdam.step (one launch of be_train_update.hip), each alone and inside a whole
training step (solve -> implicit_feed -> surrogate_grad -> update).  Shapes: Bibtex at batch 128 / nIter 10,
the completion conv PICNN at batch 70 / nIter 5.  Device events around each repetition, warm-up first; prints the median,
min and max in ms and one JSON line per model.

    python tools/train_step_time.py [--reps 20] [--warmup 3] [--only bibtex|conv]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icnn_amd import bundle_entropy, picnn, train  # noqa: E402


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "min": float(np.min(out)), "max": float(np.max(out))}


def _problem(which):
    rng = np.random.RandomState(0)
    if which == "bibtex":
        spec, B, n_iter, loss = picnn.bibtex_spec(), 128, 10, "xent"
        params, Model = picnn.init_params(spec, 0, "spread"), picnn.FCModel
        x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
        y = (rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)
    else:
        spec, B, n_iter, loss = picnn.ConvSpec(), 70, 5, "mse"
        params, Model = picnn.init_conv_params(spec, 0, "spread"), picnn.ConvModel
        x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
        y = rng.rand(B, spec.n_labels)
    return spec, params, Model, x, y, n_iter, loss


def _grad(model, x, y, n_iter, loss, conv, flat):
    B = x.shape[0]
    solver = bundle_entropy.FusedSolver(model, B, n_iter)
    res = solver.solve(model.context(x), 0.5)
    if conv:
        model.context(x, bn_updates=res.fg_evaluations())
    feed = bundle_entropy.implicit_feed(res, y, loss)
    return train.surrogate_grad(model, x, feed, bn_updates=1 if conv else 0, flat=flat)


def run(which, reps, warmup):
    conv = which == "conv"
    spec, params, Model, x, y, n_iter, loss = _problem(which)
    # host path
    host_model = Model(spec, params, "cuda")
    theta = {k: torch.from_numpy(v).cuda() for k, v in params.items()}
    ref = train.TFAdam(theta, lr=1e-3)
    g_dict = _grad(host_model, x, y, n_iter, loss, conv, False)

    def host_update(g=None):
        ref.step(g if g is not None else g_dict)
        p = picnn.project({k: t.cpu().numpy() for k, t in theta.items()})
        theta.update({k: torch.from_numpy(v).cuda() for k, v in p.items()})
        host_model.repack(p)

    def host_step():
        host_update(_grad(host_model, x, y, n_iter, loss, conv, False))

    # device path
    model = Model(spec, params, "cuda")
    opt = train.DeviceAdam(model, lr=1e-3)
    g_flat = _grad(model, x, y, n_iter, loss, conv, True)

    def device_step():
        opt.step(_grad(model, x, y, n_iter, loss, conv, True))

    out = {"model": which, "theta_floats": opt.n, "arena_floats": opt.map.arena_floats, "copies": int(opt.map.dest.size),
           "max_fanout": opt.map.max_fanout,
           "byte_floor_MB": (opt.n * 32 + opt.map.dest.size * 8) / 1e6,
           "update_host_ms": _timed(host_update, reps, warmup),
           "update_device_ms": _timed(lambda: opt.step(g_flat), reps, warmup),
           "step_host_ms": _timed(host_step, reps, warmup),
           "step_device_ms": _timed(device_step, reps, warmup)}
    for k in ("update_host_ms", "update_device_ms", "step_host_ms", "step_device_ms"):
        t = out[k]
        print("%-7s %-17s median %8.3f ms  [%.3f, %.3f]" % (which, k, t["median"], t["min"], t["max"]))
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["bibtex", "conv"])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for which in ([a.only] if a.only else ["bibtex", "conv"]):
        run(which, a.reps, a.warmup)


if __name__ == "__main__":
    main()
