#!/usr/bin/env python3
"""Environment steps per second of act + observe + train with E environments a step (GPU box only):
    python tools/rl_vec_step_time.py [--steps N] [--envs 1,4,16,64,256]
The three agents and both ICNN inner optimisers on the HalfCheetah shapes (dimO 17, dimA 6, minibatch 256, one captured
training iteration per vector step), next to the single-environment agent measured in the same run on the same GPU; the
environment is a stream of random observations, so the figures are the agent's side alone.  Then icnn_be_adam_fc_each against
icnn_be_adam_fc at equal batch on the critic (the per-state rule runs every state to ITS stop, the batch rule all of them to the
batch's)."""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DIMO, DIMA = 17, 6


def make(kind, n_envs, seed=0):
    from icnn_amd import picnn, rl_agent
    E = n_envs or 1
    kw = dict(bsize=256, warmup=max(2 * E, 256), iters=1, rmsize=1 << 16, seed=seed, capture=True)
    if n_envs is not None:
        kw["n_envs"] = n_envs
    if kind == "DDPG":
        return rl_agent.DDPGAgent(DIMO, DIMA, **kw)
    if kind == "NAF":
        return rl_agent.NAFAgent(DIMO, DIMA, **kw)
    spec = dataclasses.replace(picnn.halfcheetah_spec(), action_box=False)
    params = picnn.init_params(spec, seed)
    return rl_agent.Agent(picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda"),
                          opt="adam" if kind == "ICNN adam" else "bundle_entropy", **kw)


def steps_per_second(agent, n_envs, steps):
    import torch
    E = n_envs or 1
    rng = np.random.RandomState(1)
    shape = (E, DIMO) if n_envs is not None else (DIMO,)
    obs = rng.randn(steps + 1, *shape).astype(np.float32)
    rew = rng.randn(steps, E).astype(np.float32)
    term = np.zeros(E, bool)
    agent.reset(obs[0])
    warm = agent.warmup // E + 4                      # past the warm-up, the eager iteration and the capture
    t0 = None
    for s in range(warm + steps):
        if s == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        agent.act()
        k = s % steps
        if n_envs is not None:
            agent.observe(rew[k], term, obs[k + 1])
        else:
            agent.observe(float(rew[k, 0]), False, obs[k + 1])
    torch.cuda.synchronize()
    agent.memory.raise_on_error()
    return steps * E / (time.perf_counter() - t0)


def adam_rules(batches, reps=20):
    import torch
    from icnn_amd import _lib, picnn, rl_adam
    spec = dataclasses.replace(picnn.halfcheetah_spec(), action_box=False)
    model = picnn.FCModel(spec, picnn.init_params(spec, 1, "spread", yu_bias=1.0, gate_bias=1.0), "cuda")     # actions that move
    obs = torch.from_numpy(np.random.RandomState(2).randn(max(batches), DIMO).astype(np.float32))
    ctx_all = model.context(obs)
    print("\n%6s  %-22s %10s  %-16s %10s  %s" % ("B", "adam_fc plan", "us", "adam_fc_each plan", "us", "iters: batch | each min..max"))
    for B in batches:
        ctx = ctx_all[:B].contiguous()
        row = []
        for stop in ("batch", "each"):
            solver = rl_adam.AdamSolver(model, B, 1000, stop=stop)
            for _ in range(3):
                res = solver.solve(ctx)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                solver.solve(ctx)
            b.record()
            torch.cuda.synchronize()
            row.append((a.elapsed_time(b) / reps * 1e3, res.iters.cpu().numpy()))
        print("%6d  %-22s %10.1f  %-16s %10.1f  %d | %d..%d" % (
            B, "%s %dx%d" % _lib.adam_plan(model.c_model, B)[:3], row[0][0], "%s %dx%d" % _lib.adam_each_plan(model.c_model, B),
            row[1][0], int(row[0][1]), int(row[1][1].min()), int(row[1][1].max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--envs", default="1,4,16,64,256")
    ap.add_argument("--adam-only", action="store_true", help="only the comparison of the two stopping rules")
    args = ap.parse_args()
    if args.adam_only:
        return adam_rules([1, 4, 16, 64, 256, 1024, 1040, 2048, 4096])
    envs = [int(e) for e in args.envs.split(",")]
    print("environment steps per second (act + observe + one captured training iteration at minibatch 256)")
    print("%-20s %12s " % ("agent", "single-env") + " ".join("%11s" % ("E = %d" % e) for e in envs))
    for kind in ("ICNN adam", "ICNN bundle_entropy", "DDPG", "NAF"):
        cells = [steps_per_second(make(kind, None), None, max(args.steps, 100))]
        cells += [steps_per_second(make(kind, e), e, args.steps) for e in envs]
        print("%-20s %12.0f " % (kind, cells[0]) + " ".join("%11.0f" % c for c in cells[1:]), flush=True)
    adam_rules([1, 4, 16, 64, 256, 1024, 1040, 2048, 4096])


if __name__ == "__main__":
    main()
