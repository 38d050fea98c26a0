"""The RL experiment's loop (RL/src/main.py:82-149) around icnn_amd.rl_agent.Agent (--model ICNN, the default) or
icnn_amd.rl_agent.DDPGAgent / NAFAgent (--model DDPG / NAF; RL/src/main.py:49-57) on a small built-in environment: test
episodes, then training episodes until the next multiple of --train, up to --total training steps, with --tmax and the
returns logged.  The environment is NumPy: a damped point mass in dimA dimensions that the action pushes and the reward
wants at the origin; the observation is (position, velocity), truncated or zero-padded to dimO.

    python examples/rl_agent.py [--total 2000] [--train 200] [--test 2] [--tmax 50] [--warmup 100] [--bsize 64] [--iter 1]
                                [--dimO 4] [--dimA 2] [--capture] [--save FILE] [--resume FILE] [--model {ICNN,DDPG,NAF}]
                                [--naf-bn] [--icnn-opt {adam,bundle_entropy}]

--icnn-opt (with --model ICNN): the agent's inner optimiser, FLAGS.icnn_opt of RL/src/icnn.py:39-44.
--naf-bn (with --model NAF): the NAF networks with BatchNorm, agent.py:22's naf_bn.
--resume FILE restores the agent from a checkpoint before the loop (RL/src/icnn.py:134-137 restores the latest one at
construction) and --save FILE writes one after it (RL/src/main.py:113-115): weights, optimiser state, noise, the random
state and the replay memory, so that the agent continues as if it had not stopped.
"""
import argparse
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class PointMass:
    """v <- (1 - damping) v + dt a,  p <- p + dt v,  reward -(|p|^2 + 0.1 |v|^2 + 0.01 |a|^2); an episode ends after
    `horizon` steps or when the mass leaves the arena |p| <= 4."""

    def __init__(self, dimO=4, dimA=2, horizon=40, dt=0.1, damping=0.1, seed=0):
        self.dimO, self.dimA, self.horizon, self.dt, self.damping = dimO, dimA, horizon, dt, damping
        self.rng = np.random.RandomState(seed)
        self.reset()

    def _obs(self):
        full = np.concatenate([self.p, self.v])
        out = np.zeros(self.dimO, np.float32)
        k = min(self.dimO, full.size)
        out[:k] = full[:k]
        return out

    def reset(self):
        self.p = self.rng.uniform(-1, 1, self.dimA)
        self.v = np.zeros(self.dimA)
        self.steps = 0
        return self._obs()

    def step(self, action):
        a = np.clip(np.asarray(action, np.float64).reshape(self.dimA), -1, 1)
        self.v = (1 - self.damping) * self.v + self.dt * a
        self.p = self.p + self.dt * self.v
        self.steps += 1
        reward = -(float(self.p @ self.p) + 0.1 * float(self.v @ self.v) + 0.01 * float(a @ a))
        term = self.steps >= self.horizon or float(np.linalg.norm(self.p)) > 4.0
        return self._obs(), reward, term


class VecPointMass:
    """E independent PointMass environments stepped as arrays: step() returns obs [E, dimO], reward [E], term [E] and restarts
    the environments that ended (their returned observation is the new episode's first)."""

    def __init__(self, n_envs, dimO=4, dimA=2, horizon=40, dt=0.1, damping=0.1, seed=0):
        self.E, self.dimO, self.dimA, self.horizon, self.dt, self.damping = n_envs, dimO, dimA, horizon, dt, damping
        self.rng = np.random.RandomState(seed)
        self.p, self.v = np.zeros((n_envs, dimA)), np.zeros((n_envs, dimA))
        self.steps = np.zeros(n_envs, np.int64)

    def _obs(self):
        full = np.concatenate([self.p, self.v], axis=1)
        out = np.zeros((self.E, self.dimO), np.float32)
        k = min(self.dimO, full.shape[1])
        out[:, :k] = full[:, :k]
        return out

    def reset(self, mask=None):
        mask = np.ones(self.E, bool) if mask is None else mask
        self.p[mask] = self.rng.uniform(-1, 1, (int(mask.sum()), self.dimA))
        self.v[mask] = 0.0
        self.steps[mask] = 0
        return self._obs()

    def step(self, action):
        a = np.clip(np.asarray(action, np.float64).reshape(self.E, self.dimA), -1, 1)
        self.v = (1 - self.damping) * self.v + self.dt * a
        self.p = self.p + self.dt * self.v
        self.steps += 1
        reward = -((self.p * self.p).sum(1) + 0.1 * (self.v * self.v).sum(1) + 0.01 * (a * a).sum(1))
        term = (self.steps >= self.horizon) | (np.linalg.norm(self.p, axis=1) > 4.0)
        return self._obs(), reward, term


def run_vector(env, agent, total):
    """`total` training observations, E a step: an environment that ends is restarted and its noise row zeroed"""
    agent.reset(env.reset())
    returns, running = [], np.zeros(env.E)
    while agent.t < total:
        observation, reward, term = env.step(agent.act())
        agent.observe(reward, term, observation)
        running += reward
        if term.any():
            returns += running[term].tolist()
            running[term] = 0.0
            agent.reset(env.reset(term), mask=term)
    return returns


def run_episode(env, agent, test, tmax):
    """main.py:117-149"""
    agent.reset(env.reset())
    sum_reward, timestep, term = 0.0, 0, False
    while not term:
        action = agent.act(test=test)
        observation, reward, term = env.step(action)
        term = (not test and timestep + 1 >= tmax) or term
        agent.observe(reward, term, observation, test=test)
        sum_reward += reward
        timestep += 1
    return sum_reward, timestep


def main():
    import torch

    from icnn_amd import picnn, rl_agent

    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=2000)
    ap.add_argument("--train", type=int, default=200)
    ap.add_argument("--test", type=int, default=2)
    ap.add_argument("--tmax", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--bsize", type=int, default=64)
    ap.add_argument("--iter", type=int, default=1)
    ap.add_argument("--rmsize", type=int, default=100000)
    ap.add_argument("--dimO", type=int, default=4)
    ap.add_argument("--dimA", type=int, default=2)
    ap.add_argument("--l1size", type=int, default=64)
    ap.add_argument("--l2size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--capture", action="store_true")
    ap.add_argument("--save", default=None, metavar="FILE")
    ap.add_argument("--resume", default=None, metavar="FILE")
    ap.add_argument("--model", choices=("ICNN", "DDPG", "NAF"), default="ICNN")
    ap.add_argument("--naf-bn", action="store_true")
    ap.add_argument("--icnn-opt", choices=("adam", "bundle_entropy"), default="adam")
    ap.add_argument("--envs", type=int, default=None, metavar="E", help="E environments a step (a vectorised PointMass)")
    args = ap.parse_args()
    vec = dict(n_envs=args.envs) if args.envs is not None else {}
    if args.naf_bn and args.model != "NAF":
        ap.error("--naf-bn needs --model NAF")
    if args.model == "DDPG":
        agent = rl_agent.DDPGAgent(args.dimO, args.dimA, l1=args.l1size, l2=args.l2size, bsize=args.bsize, warmup=args.warmup,
                                   iters=args.iter, rmsize=args.rmsize, seed=args.seed, capture=args.capture, **vec)
    elif args.model == "NAF":
        agent = rl_agent.NAFAgent(args.dimO, args.dimA, l1=args.l1size, l2=args.l2size, bsize=args.bsize, warmup=args.warmup,
                                  iters=args.iter, rmsize=args.rmsize, seed=args.seed, capture=args.capture, naf_bn=args.naf_bn, **vec)
    else:
        spec = dataclasses.replace(picnn.halfcheetah_spec(), n_features=args.dimO, n_labels=args.dimA,
                                   szs=(args.l1size, args.l2size), action_box=False)
        params = picnn.init_params(spec, args.seed)
        critic, target = picnn.FCModel(spec, params, "cuda"), picnn.FCModel(spec, params, "cuda")
        agent = rl_agent.Agent(critic, target, bsize=args.bsize, warmup=args.warmup, iters=args.iter, rmsize=args.rmsize,
                               seed=args.seed, capture=args.capture, opt=args.icnn_opt, **vec)
    env = PointMass(args.dimO, args.dimA, seed=args.seed)
    if args.resume:
        from icnn_amd import checkpoint
        checkpoint.load(args.resume, agent)
        print("resumed {} at {} training observations".format(args.resume, agent.t))
    if args.envs is not None:
        returns = run_vector(VecPointMass(args.envs, args.dimO, args.dimA, seed=args.seed), agent, args.total)
        loss = float(agent.loss.item()) if agent.t > agent.warmup and agent.iters else float("nan")
        print("{} environments, {} training observations, {} episodes, mean return {:.4f}, loss {:.5e}".format(
            args.envs, agent.t, len(returns), np.mean(returns) if returns else float("nan"), loss))
        args.total = 0
    train_timestep = 0
    while train_timestep < args.total:
        rewards = [run_episode(env, agent, True, args.tmax)[0] for _ in range(args.test)]
        print("Average test return {} after {} timestep of training.".format(np.mean(rewards), train_timestep))
        rewards, checkpoint = [], train_timestep // args.train
        while train_timestep // args.train == checkpoint:
            reward, timestep = run_episode(env, agent, False, args.tmax)
            rewards.append(reward)
            train_timestep += timestep
            if agent.t > agent.warmup:
                loss = float(agent.loss.item())
                if not np.isfinite(loss):
                    raise RuntimeError("the critic's loss is not finite")
                print("  + train {}\treturn {:.4f}\tloss {:.5e}".format(train_timestep, reward, loss))
            else:
                print("  + train {}\treturn {:.4f}\t(warm-up: no training yet)".format(train_timestep, reward))
        print("Average train return {} after {} timestep of training.".format(np.mean(rewards), train_timestep))
    agent.memory.raise_on_error()
    torch.cuda.synchronize()
    if args.save:
        from icnn_amd import checkpoint
        checkpoint.save(args.save, agent)
        print("saved {}".format(args.save))


if __name__ == "__main__":
    main()
