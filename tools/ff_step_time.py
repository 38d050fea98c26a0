"""Time the feed-forward baseline's training step (ff.FFTrainer) at B = 128, 1836 features, [600], 159 labels:

    eager      the whole step enqueued from Python (icnn_be_ff_step: forward, backward, gradients, update, fold)
    captured   the step captured once in a CUDA graph and replayed
    launches   forward (the layer launches and the head), backward, grads, update alone (events around each, eager), and the
               first layer's forward with a head of one label (ff_layer_fwd_kernel at B x n_features x layers[0] and one
               workgroup of ff_head_kernel); a kernel trace of this tool (--eval-batch 0) gives every kernel's own time
    context    the library's other implementation of a ReLU / BatchNorm layer at that shape, for comparison: FCModel.context
               of a PICNN with the same first layer (ctx_gemm_kernel + ctx_bn_kernel).  Its stage-0 product also carries the
               yu and zu columns of the PICNN, 2 x layers[0] + 1 columns in all, so it does twice the arithmetic of the first
               layer alone; context_per_600_ms scales its time to the layer's own columns.
    evaluate   the test phase on --eval-batch rows

    python tools/ff_step_time.py [--steps 200] [--warmup 20] [--batch 128] [--features 1836] [--layers 600] [--labels 159]
Two runs in one process; prints one JSON line per run."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import _lib, ff, picnn  # noqa: E402


def _ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def run(args):
    B = args.batch
    spec = ff.FFSpec(args.features, args.labels, tuple(args.layers))
    tr = ff.FFTrainer(ff.FFModel(spec, seed=1), B, eval_batch=args.eval_batch or None)
    rng = np.random.RandomState(1)
    tr.x.copy_(torch.from_numpy((rng.rand(B, args.features) < 0.04).astype(np.float32)))
    tr.true_y.copy_(torch.from_numpy((rng.rand(B, args.labels) < 0.02).astype(np.float32)))
    out = {"batch": B, "features": args.features, "layers": list(args.layers), "labels": args.labels, "params": tr.model.n}
    out["eager_ms"] = _ms(tr.step, args.steps, args.warmup)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.step()
    out["captured_ms"] = _ms(g.replay, args.steps, args.warmup)
    out["launches_ms"] = {name: _ms(getattr(tr, name), args.steps, args.warmup) for name in ("forward", "backward", "grads", "update")}
    # the first layer alone: a one-layer model's forward without targets is that launch and a head of one label
    one = ff.FFModel(ff.FFSpec(args.features, 1, (args.layers[0],)), seed=1)
    work, yhat = one.work(B), torch.empty(B, 1, dtype=torch.float32, device="cuda")
    a = one.args(B, work)
    a.x, a.yhat = tr.x.data_ptr(), yhat.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    both = _ms(lambda: _lib.check(one._lib.icnn_be_ff_forward(C.byref(a), 0, stream), "icnn_be_ff_forward"), args.steps, args.warmup)
    out["layer1_fwd_and_head_ms"] = both
    # the same arithmetic through the context producer
    pspec = picnn.FCSpec(args.features, 1, (args.layers[0], 1), alpha=0.0, batchnorm=True, action_box=False)
    pm = picnn.FCModel(pspec, picnn.init_params(pspec, 0, "spread"), "cuda")
    ctx = torch.empty(B, pspec.ctx_width, dtype=torch.float32, device="cuda")
    cwork = torch.empty(pm.context_work_floats(B), dtype=torch.float32, device="cuda")
    out["context_ms"] = _ms(lambda: pm.context(tr.x, out=ctx, work=cwork), args.steps, args.warmup)
    out["context_per_600_ms"] = out["context_ms"] * args.layers[0] / (2 * args.layers[0] + 1)
    if args.eval_batch:
        tr.x_eval.copy_(torch.from_numpy((rng.rand(args.eval_batch, args.features) < 0.04).astype(np.float32)))
        out["evaluate_ms"] = _ms(tr.evaluate, args.steps, args.warmup)
    assert np.isfinite(tr.loss.item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--features", type=int, default=1836)
    ap.add_argument("--layers", type=int, nargs="+", default=[600])
    ap.add_argument("--labels", type=int, default=159)
    ap.add_argument("--eval-batch", type=int, default=2515)
    args = ap.parse_args()
    for _ in range(2):
        print(json.dumps(run(args)))


if __name__ == "__main__":
    main()
