"""Time the NAF training step (naf.NAFTrainer) at B = 256, dimO 17, dimA 6, l1 = l2 = 200:

    eager      the whole step enqueued from Python (icnn_be_naf_step: chain, gradients, update)
    captured   the step captured once in a CUDA graph and replayed
    launches   each of the three parts alone (events around it, eager)
    act        the latency of NAFAgent.act() for one observation, the copy of the action to the host included (wall clock),
               and of the u launch alone (events)

    python tools/naf_step_time.py [--steps 200] [--warmup 20] [--batch 256] [--dimO 17] [--dimA 6] [--l1 200] [--l2 200]
                                  [--bn] [--repeats 5]
Prints one JSON line.  --bn: the same measurements of NAFTrainer(bn=True) (its step has a fourth part, the
fold) next to the plain ones in the same run: {"plain": {...}, "bn": {...}}.  captured_ms and act_launch_ms are the median
of --repeats measurements; captured_spread_ms and act_launch_spread_ms their smallest and largest."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import naf, rl_agent  # noqa: E402


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


def _repeated(fn, steps, warmup, repeats):
    ms = sorted(_ms(fn, steps, warmup if i == 0 else 2) for i in range(repeats))
    return ms[len(ms) // 2], [ms[0], ms[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dimO", type=int, default=17)
    ap.add_argument("--dimA", type=int, default=6)
    ap.add_argument("--l1", type=int, default=200)
    ap.add_argument("--l2", type=int, default=200)
    ap.add_argument("--bn", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.bn:
        print(json.dumps({"plain": measure(args, False), "bn": measure(args, True)}))
    else:
        print(json.dumps(measure(args, False)))


def measure(args, bn):
    B = args.batch
    tr = naf.NAFTrainer(args.dimO, args.dimA, args.l1, args.l2, batch=B, bn=bn)
    rng = np.random.RandomState(1)
    tr.obs.copy_(torch.from_numpy(rng.randn(B, args.dimO).astype(np.float32)))
    tr.ob2.copy_(tr.obs + 0.1 * torch.randn_like(tr.obs))
    tr.act.copy_(torch.from_numpy(np.clip(0.6 * rng.randn(B, args.dimA), -1, 1)))
    tr.rew.copy_(torch.from_numpy(rng.randn(B).astype(np.float32)))
    tr.term.copy_(torch.from_numpy((rng.rand(B) < 0.2).astype(np.uint8)))
    # the 0.01 initialisation leaves every product near zero; time the step at weights of the usual size instead
    for w in naf.TRAINED:
        tr.theta[w].copy_(torch.from_numpy(rng.uniform(-0.07, 0.07, tr.n[w]).astype(np.float32)))
    tr.theta["target_v"].copy_(tr.theta["v"][:tr.theta["target_v"].numel()])
    out = {"batch": B, "dimO": args.dimO, "dimA": args.dimA, "l1": args.l1, "l2": args.l2, "params": dict(tr.n)}
    out["eager_ms"] = _ms(tr.step_buffers, args.steps, args.warmup)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.step_buffers()
    out["captured_ms"], out["captured_spread_ms"] = _repeated(g.replay, args.steps, args.warmup, args.repeats)
    out["launches_ms"] = {name: _ms(getattr(tr, name), args.steps, args.warmup) for name in ("chain", "grads", "update")}
    assert np.isfinite(tr.loss.item())

    agent = rl_agent.NAFAgent(args.dimO, args.dimA, args.l1, args.l2, bsize=B, rmsize=16, naf_bn=bn)
    agent.reset(rng.randn(args.dimO).astype(np.float32))
    for _ in range(args.warmup):
        agent.act()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        agent.act()
    out["act_ms"] = (time.perf_counter() - t0) / args.steps * 1e3
    out["act_launch_ms"], out["act_launch_spread_ms"] = _repeated(lambda: agent.trainer.policy(agent._obs1, out=agent._act1),
                                                                  args.steps, args.warmup, args.repeats)
    return out


if __name__ == "__main__":
    main()
