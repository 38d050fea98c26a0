"""NumPy statement of the device replay memory (icnn_amd/csrc/be_rl_replay.hip, icnn_amd/rl_agent.ReplayMemory): Philox4x32-10,
the memory of RL/src/replay_memory.py:10-34 and its sampling rule :36-55 with the candidates of include/icnn_be.h
(icnn_be_replay_sample) -- or with a recorded candidate stream, which is how tests/golden/replay__wrap.npz pins this
restatement on the reference's own class."""
import numpy as np

MAX_ATTEMPTS = 256
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """the four output words of Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3;
    SC'11) at a counter of four and a key of two 32-bit words"""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def candidate(seed, draw, k, attempt, n):
    """candidate number `attempt` of sample k in draw `draw` at fill n: uniform on [0, n - 2]"""
    word = philox4x32_10((draw, k, attempt, 0), (seed & MASK, (seed >> 32) & MASK))[0]
    return (word * (n - 1)) >> 32


class ReplayMemory:
    """replay_memory.py's class with the arrays of the device memory: float32 observations, actions and rewards, uint8
    terminals, zero before the first enqueue."""

    def __init__(self, size, dimO, dimA, seed=0):
        self.size, self.dimO, self.dimA, self.seed = size, dimO, dimA, int(seed)
        self.observations = np.zeros((size, dimO), np.float32)
        self.actions = np.zeros((size, dimA), np.float32)
        self.rewards = np.zeros(size, np.float32)
        self.terminals = np.zeros(size, np.uint8)
        self.reset()

    def reset(self):
        self.n = self.i = self.draws = 0

    def enqueue(self, observation, terminal, action, reward):
        self.observations[self.i] = observation
        self.terminals[self.i] = bool(terminal)
        self.actions[self.i] = np.asarray(action, np.float64).astype(np.float32)
        self.rewards[self.i] = reward
        self.i = (self.i + 1) % self.size
        self.n = min(self.size - 1, self.n + 1)

    def minibatch(self, size, candidates=None):
        """(obs, act float64, rew, ob2, term uint8, idx int32, attempts int32 [size], exhausted bool [size]).  candidates
        None: the device's Philox candidates at this memory's seed and draw counter, at most MAX_ATTEMPTS per sample (the
        last one is kept); else an iterator that yields the candidates in the order the reference's loop asks for them
        (unbounded, as the reference is).  Either way the draw counter advances by one."""
        idx = np.zeros(size, np.int32)
        attempts = np.zeros(size, np.int32)
        exhausted = np.zeros(size, bool)
        for k in range(size):
            while True:
                if candidates is None:
                    c = candidate(self.seed, self.draws, k, int(attempts[k]), self.n)
                else:
                    c = int(next(candidates))
                attempts[k] += 1
                if c != self.i and not self.terminals[c]:
                    break
                if candidates is None and attempts[k] == MAX_ATTEMPTS:
                    exhausted[k] = True
                    break
            idx[k] = c
        self.draws += 1
        return (self.observations[idx].copy(), self.actions[idx].astype(np.float64), self.rewards[idx].copy(),
                self.observations[idx + 1].copy(), self.terminals[idx + 1].copy(), idx, attempts, exhausted)
