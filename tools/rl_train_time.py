"""Time the RL critic's training step (rl_train.CriticTrainer) at B = 256 on the halfcheetah critic:

    captured   the whole step captured once in a CUDA graph and replayed
    eager      the whole step enqueued from Python
    launches   each stage of the step alone (events around it, eager)
    host       the host-composed path: the existing device pieces (context, AdamSolver, fg, surrogate_grad, DeviceAdam)
               with TD, decay and the Polyak update in torch ops and a host repack of the target FCModel
    oracle     tests/rl_train_ref.py's NumPy step (CPU; one step)

    python tools/rl_train_time.py [--steps 20] [--warmup 3] [--no-oracle] [--opt {adam,bundle_entropy}]

--opt bundle_entropy: the step with the bundle-entropy inner optimiser -- captured, eager, per launch --, the
target solve as the one-launch entry against the three-step composition (--repeats timings of --steps calls each: min, median,
max) and act() at B = 1 (context + inner optimiser, wall clock, median of 50 as tools/act_latency.py) for both optimisers.
The host-composed path and the oracle are the adam branch's.
Prints one JSON line."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from icnn_amd import picnn, rl_adam, rl_bundle, rl_train, train  # noqa: E402


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


def _act_us(model, solver, obs):
    """context + inner optimiser at one observation: wall clock, median of 50 (tools/act_latency.py)"""
    for _ in range(5):
        solver.solve(model.context(obs))
    torch.cuda.synchronize()
    ts = []
    for _ in range(50):
        t0 = time.perf_counter()
        solver.solve(model.context(obs))
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--opt", choices=rl_train.OPTS, default="adam")
    ap.add_argument("--n-iter", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    bundle = args.opt == "bundle_entropy"
    B = args.batch
    spec = dataclasses.replace(picnn.halfcheetah_spec(), action_box=False)
    params = picnn.init_params(spec, 0, "spread", yu_bias=1.0, gate_bias=1.0)
    rng = np.random.RandomState(1)
    obs = torch.from_numpy(rng.randn(B, spec.n_features).astype(np.float32)).cuda()
    act = torch.from_numpy(np.clip(0.6 * rng.randn(B, spec.n_labels), -0.999, 0.999)).cuda()
    rew = torch.from_numpy((2 * rng.randn(B)).astype(np.float32)).cuda()
    ob2 = obs + 0.1 * torch.randn_like(obs)
    term = torch.from_numpy(rng.rand(B) < 0.2).cuda()
    out = {"batch": B, "params": None, "opt": args.opt}

    tr = rl_train.CriticTrainer(picnn.FCModel(spec, params), picnn.FCModel(spec, params), B, opt=args.opt, n_iter=args.n_iter)
    tr.initialise()
    out["params"] = tr.opt.n
    out["eager_ms"] = _ms(lambda: tr.step(obs, act, rew, ob2, term), args.steps, args.warmup)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.step(obs, act, rew, ob2, term)
    out["captured_ms"] = _ms(g.replay, args.steps, args.warmup)

    # per launch (eager, one stage at a time on the trainer's buffers)
    ctx2 = tr.target.context(tr.ob2)
    res = tr.solver.solve(ctx2)
    ctx = tr.critic.context(tr.obs)
    e, _ = tr.critic.fg(ctx, tr.act)
    grad = train.surrogate_grad(tr.critic, tr.obs, (tr.act, tr.c), flat=True)
    stages = {
        "target_context": lambda: tr.target.context(tr.ob2),
        ("target_bundle" if bundle else "target_adam"): lambda: tr.solver.solve(ctx2),
        "critic_context": lambda: tr.critic.context(tr.obs),
        "critic_fg": lambda: tr.critic.fg(ctx, tr.act),
        "rl_td": (lambda: tr.td_loss(e, res.q, res.act)) if bundle else (lambda: tr.td_loss(e, res.f_best, None)),
        "surrogate_grad": lambda: train.surrogate_grad(tr.critic, tr.obs, (tr.act, tr.c), flat=True),
        "rl_critic_update": lambda: tr.update(grad),
    }
    out["launch_ms"] = {k: _ms(f, args.steps, args.warmup) for k, f in stages.items()}
    if bundle:
        # the target solve alone: the one-launch entry against [solve_fc_reset, 2y - 1, fc_fg] on the same build, interleaved
        solvers = {"entry": rl_bundle.BundleActionSolver(tr.target, B, args.n_iter, entry=True),
                   "composed": rl_bundle.BundleActionSolver(tr.target, B, args.n_iter, entry=False)}
        times = {k: [] for k in solvers}
        for _ in range(args.repeats):
            for k, sv in solvers.items():
                times[k].append(_ms(lambda: sv.solve(ctx2), args.steps, args.warmup))
        assert solvers["entry"].used_entry and not solvers["composed"].used_entry
        out["solve_ms"] = {k: {"min": min(t), "median": float(np.median(t)), "max": max(t)} for k, t in times.items()}
        # act() at B = 1, both optimisers on one critic (tools/act_latency.py's model)
        model1 = picnn.FCModel(spec, picnn.init_params(spec, 11, "spread", yu_bias=1.0, gate_bias=1.0))
        obs1 = torch.from_numpy(np.random.RandomState(12).randn(1, spec.n_features).astype(np.float32)).cuda()
        out["act_us"] = {"adam": _act_us(model1, rl_adam.AdamSolver(model1, 1, 1000), obs1),
                         "bundle_entropy": _act_us(model1, rl_bundle.BundleActionSolver(model1, 1, args.n_iter), obs1),
                         "bundle_entropy_composed": _act_us(model1, rl_bundle.BundleActionSolver(model1, 1, args.n_iter, entry=False), obs1)}
        print(json.dumps(out))
        return

    # the host-composed path: the existing pieces, torch ops for TD / decay / Polyak, a host repack of the target
    critic, target = picnn.FCModel(spec, params), picnn.FCModel(spec, params)
    opt = train.DeviceAdam(critic)
    mask = torch.from_numpy(rl_train.decay_mask(spec).astype(bool)).cuda()
    theta_t = opt.theta.clone()
    solver = rl_adam.AdamSolver(target, B)

    def entropy(a):
        p = ((a.float() + 1) * 0.5).clamp(1e-4, 0.9999)
        return -(p * torch.log(p) + (1 - p) * torch.log(1 - p)).sum(1)

    def host_step():
        r = solver.solve(target.context(ob2))
        q2 = -r.f_best
        e_c, _ = critic.fg(critic.context(obs), act)
        q = -(e_c - entropy(act))
        y = torch.where(term, rew, rew + 0.99 * q2)
        y = torch.minimum(q + 1, torch.maximum(q - 1, y))
        td = q - y
        loss = (td * td).mean() + 1e-4 * 1e-3 * (opt.theta[mask] ** 2).sum() / 2
        c = (-(2.0 / B) * td).double()
        gr = train.surrogate_grad(critic, obs, (act, c), flat=True)
        gr = torch.where(mask, gr + 1e-7 * opt.theta, gr)
        theta_t.sub_(0.01 * (theta_t - opt.theta))
        opt.step(gr)
        target.repack(train.unpack_grad(spec, theta_t.cpu()))                        # host repack of the target
        return loss
    out["host_composed_ms"] = _ms(host_step, max(args.steps // 2, 3), 1)

    if not args.no_oracle:
        import rl_train_ref as ref
        obs_h, act_h, rew_h, ob2_h, term_h = (t.cpu().numpy() for t in (obs, act, rew, ob2, term))
        ctx2_h = tr.target.context(ob2).cpu().numpy()
        ph = tr.host_params()
        theta_h = tr.opt.theta.cpu().numpy()
        t0 = time.perf_counter()
        act2, _, fbest = ref.target_actions(spec, tr.host_params(target=True), ctx2_h)
        th64 = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in ph.items()}
        E = ref.train_ref.energy(spec, th64, torch.as_tensor(obs_h.astype(np.float64)), torch.as_tensor(act_h))[0].numpy()
        _, _, tdv, c = ref.td(E.astype(np.float32), act_h, rew_h, term_h, fbest, None, 0.99, B)
        ref.loss(tdv, theta_h, rl_train.decay_mask(spec), 1e-4, 1e-3)
        g64, _, _ = ref.train_ref.surrogate_grad64(spec, ph, obs_h, act_h, None, c)
        gflat = np.concatenate([g64[k].reshape(-1) for k, _ in train.grad_layout(spec)]).astype(np.float32)
        ref.critic_update(theta_h, theta_h, np.zeros_like(theta_h), np.zeros_like(theta_h), gflat, 1,
                          rl_train.decay_mask(spec), tr.opt.map.proj, 1e-3, 0.01, 1e-4, 1e-3)
        out["oracle_ms"] = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
