"""Time one training observe() of rl_agent.Agent (enqueue one transition, then `iters` x [sample on the device,
CriticTrainer.step_buffers]) with device events, median [min, max] of --reps after --warmup, eager and with the iterations
captured in one graph, against

    host    the same work the way it was done before the memory moved to the device: a NumPy replay memory with the
            reference's sampling rule (np.random), and per iteration CriticTrainer.step on the five host arrays, i.e. its
            five copies to the device

at the HalfCheetah shapes (dimO 17, dimA 6, bsize 256, the 200-200 critic), iters 1 and 5, on a memory of --fill transitions
with 5 % terminals.  act() is not part of the timed region.  Prints one line per case and a JSON line.

    python tools/rl_agent_step_time.py [--reps 20] [--warmup 3] [--fill 1000]
"""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from icnn_amd import picnn, rl_agent, rl_train  # noqa: E402


class HostMemory:
    """RL/src/replay_memory.py's rule in NumPy (float32 actions widened on the way out, as CriticTrainer.act holds them)"""

    def __init__(self, size, dimO, dimA, seed):
        self.size, self.n, self.i, self.rng = size, 0, 0, np.random.RandomState(seed)
        self.observations, self.actions = np.zeros((size, dimO), np.float32), np.zeros((size, dimA), np.float32)
        self.rewards, self.terminals = np.zeros(size, np.float32), np.zeros(size, bool)

    def enqueue(self, obs, term, act, rew):
        self.observations[self.i], self.terminals[self.i], self.actions[self.i], self.rewards[self.i] = obs, term, act, rew
        self.i = (self.i + 1) % self.size
        self.n = min(self.size - 1, self.n + 1)

    def minibatch(self, size):
        idx = np.zeros(size, np.int64)
        for k in range(size):
            while True:
                c = self.rng.randint(0, self.n - 1)
                if c != self.i and not self.terminals[c]:
                    break
            idx[k] = c
        return (self.observations[idx], self.actions[idx].astype(np.float64), self.rewards[idx], self.observations[idx + 1],
                self.terminals[idx + 1])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fill", type=int, default=1000)
    args = ap.parse_args()
    spec = dataclasses.replace(picnn.halfcheetah_spec(), action_box=False)
    params = picnn.init_params(spec, 0, "spread", yu_bias=1.0, gate_bias=1.0)
    rng = np.random.RandomState(0)
    count = args.fill + 2 * (args.reps + args.warmup) + 8
    obs = rng.randn(count + 1, spec.n_features).astype(np.float32)
    act = np.clip(rng.randn(count, spec.n_labels) * 0.6, -1, 1)
    rew = rng.randn(count).astype(np.float32)
    term = rng.rand(count) < 0.05
    out = {}

    def models():
        return picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda")
    for iters in (1, 5):
        res = {}
        for mode in ("eager", "graph"):
            agent = rl_agent.Agent(*models(), bsize=256, warmup=args.fill, iters=iters, rmsize=500000, capture=mode == "graph")
            at = [0]

            def observe():
                e = at[0]
                agent.observation, agent.action = obs[e], act[e]
                agent.observe(rew[e], term[e], obs[e + 1])
                at[0] += 1
            for _ in range(args.fill):
                observe()
            res["device_" + mode] = timed(observe, args.reps, args.warmup)
            agent.memory.raise_on_error()
        trainer = rl_train.CriticTrainer(*models(), 256)
        trainer.initialise()
        memory = HostMemory(500000, spec.n_features, spec.n_labels, 0)
        at = [0]

        def host_observe():
            e = at[0]
            memory.enqueue(obs[e], term[e], act[e], rew[e])
            at[0] += 1
            if e >= args.fill:
                for _ in range(iters):
                    trainer.step(*memory.minibatch(256))
        for _ in range(args.fill):
            host_observe()
        res["host"] = timed(host_observe, args.reps, args.warmup)
        print("observe, iters=%d  ms median [min, max]" % iters)
        for k in ("device_eager", "device_graph", "host"):
            print("    %-13s %8.3f [%.3f, %.3f]" % ((k,) + tuple(res[k])))
        out["iters_%d" % iters] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
