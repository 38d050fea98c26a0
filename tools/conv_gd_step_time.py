"""Time the back-optimisation training step of the completion model (train.ConvGDTrainer: context, gd.solve with its
trajectory, the fused feed icnn_be_gd_feed_px, surrogate_grad, DeviceAdam.step) with device events, median [min, max] of --reps
calls after --warmup, eager and as one captured graph, at ConvSpec(), B = 70, K = 30, lr 0.01, momentum 0.9, against

    composed  the hand-composed step at the same commit: context, gd.solve, the torch elementwise ops (d, u, ybar,
              coef * ybar, zeros, arange) around train.unrolled_grad, DeviceAdam.step -- eager and captured

then evaluate() at eval_batch 50, and the feed kernel alone on (70, 2048, 30) inputs in the same process:

    feed_px   icnn_be_gd_feed_px with px = 1 (the B x S grid)
    feed      icnn_be_gd_feed (one workgroup per sample), the same outputs bit for bit
    feed_alt  icnn_be_gd_feed_px of ANOTHER build of the library (--alt-lib PATH), e.g. one compiled with
              ICNN_BE_EXTRA_FLAGS=-DICNN_BE_GD_FEED_PX_CHUNK=4096 into a directory of its own (icnn_amd.build.build(out_dir=))

each feed figure the time of --inner back-to-back launches divided by --inner.  Prints one line per figure and a JSON line.

    python tools/conv_gd_step_time.py [--reps 20] [--warmup 3] [--inner 20] [--alt-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import _lib, gd, picnn, train  # noqa: E402

B, K, LR, MU, PX, EVAL_B = 70, 30, 0.01, 0.9, 255.0, 50


def timed(fn, reps, warmup, inner=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
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


def whole_step(reps, warmup, res):
    spec = picnn.ConvSpec()
    n = spec.n_labels
    rng = np.random.RandomState(0)
    params = picnn.init_conv_params(spec, 0, "spread")
    x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
    t = torch.from_numpy(rng.rand(B, n).astype(np.float32)).cuda()
    y0 = 0.2 + 0.6 * rng.rand(n)
    y0d = torch.from_numpy(y0).cuda()

    def model():
        return picnn.ConvModel(spec, {k: v.copy() for k, v in params.items()}, "cuda")
    for mode in ("eager", "graph"):
        tr = train.ConvGDTrainer(model(), B, n_iter=K, lr=LR, momentum=MU, y0=y0, bn_updates=1)
        tr.step(x, t)
        res["fused_" + mode] = timed(tr.step if mode == "eager" else captured(tr.step), reps, warmup)
        m = model()
        opt = train.DeviceAdam(m)
        inv = float(np.float32(1.0) / np.float32(B * n))

        def composed():
            ctx = m.context(x)
            yK, traj, _ = gd.solve(m, ctx, y0d, K, LR, MU, trajectory=True)
            u = PX * (yK.to(torch.float32) - t)
            loss = torch.mean(u * u)
            ybar = ((u * 2.0) * inv) * PX
            opt.step(train.unrolled_grad(m, x, traj, ybar.to(torch.float64), LR, MU, bn_updates=1, flat=True))
            return loss
        composed()
        res["composed_" + mode] = timed(composed if mode == "eager" else captured(composed), reps, warmup)
    tr = train.ConvGDTrainer(model(), B, n_iter=K, lr=LR, momentum=MU, y0=y0, bn_updates=1, eval_batch=EVAL_B)
    tr.step(x, t)
    tr.evaluate(x[:EVAL_B], t[:EVAL_B])
    res["evaluate_eager"] = timed(tr.evaluate, reps, warmup)
    res["evaluate_graph"] = timed(captured(tr.evaluate), reps, warmup)


def feed_alone(reps, warmup, inner, alt_lib, res):
    lib = _lib.load()
    n = picnn.ConvSpec().n_labels
    rng = np.random.RandomState(1)
    yK = torch.from_numpy(rng.rand(B, n).astype(np.float32).astype(np.float64)).cuda()
    t = torch.from_numpy(rng.rand(B, n).astype(np.float32)).cuda()
    coef = train.unrolled_coefficients(K, LR, MU, torch.device("cuda"))
    scale = float(np.float32(1) / np.float32(B * n))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def buffers():
        return dict(v=torch.zeros(B * K, n, dtype=torch.float64, device="cuda"),
                    c=torch.zeros(B * K, dtype=torch.float64, device="cuda"),
                    off=torch.zeros(B + 1, dtype=torch.int32, device="cuda"),
                    loss=torch.zeros((), dtype=torch.float32, device="cuda"),
                    work=torch.zeros((int(lib.icnn_be_gd_feed_work_bytes(B)) + 7) // 8, dtype=torch.float64, device="cuda"))

    def px_call(handle, o):
        def call():
            _lib.check(handle.icnn_be_gd_feed_px(yK.data_ptr(), t.data_ptr(), coef.data_ptr(), B, n, K, scale, 1.0,
                                                 o["v"].data_ptr(), o["c"].data_ptr(), o["off"].data_ptr(), o["loss"].data_ptr(),
                                                 o["work"].data_ptr(), stream), "icnn_be_gd_feed_px")
        return call
    new, old = buffers(), buffers()

    def old_call():
        _lib.check(lib.icnn_be_gd_feed(yK.data_ptr(), t.data_ptr(), coef.data_ptr(), B, n, K, scale, old["v"].data_ptr(),
                                       old["c"].data_ptr(), old["off"].data_ptr(), old["loss"].data_ptr(), None,
                                       old["work"].data_ptr(), stream), "icnn_be_gd_feed")
    calls = [("feed_px", px_call(lib, new)), ("feed", old_call)]
    outs = [new, old]
    if alt_lib:
        alt = _lib.declare(C.CDLL(os.path.abspath(alt_lib)), ["icnn_be_gd_feed_px"])
        outs.append(buffers())
        calls.append(("feed_alt", px_call(alt, outs[-1])))
    for _ in range(2):                                   # alternate the candidates: two rounds each, the later one kept
        for name, call in calls:
            res[name] = timed(call, reps, warmup, inner)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert all(torch.equal(new[k], o[k]) for k in ("v", "c", "off", "loss")), "the feeds disagree"
    res["feed_bytes_written"] = 8 * B * K * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--feed-only", action="store_true")
    args = ap.parse_args()
    res = {}
    if not args.feed_only:
        whole_step(args.reps, args.warmup, res)
    feed_alone(args.reps, args.warmup, args.inner, args.alt_lib, res)
    print("ConvSpec() B=%d K=%d  ms median [min, max]" % (B, K))
    for k, v in res.items():
        if isinstance(v, list):
            print("    %-15s %8.4f [%.4f, %.4f]" % ((k,) + tuple(v)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
