#!/usr/bin/env python3
"""Golden vectors for the replay memory from the REFERENCE's own class (needs the reference tree; the tests only read the
fixture).

RL/src/replay_memory.py is loaded by path and run unmodified (nothing is copied into this repository; bytecode writing is
off; np.int / np.bool, which it uses and NumPy 2 dropped, are shimmed).  Its `np.random.randint` is replaced by a recorded
candidate stream: seeded draws from the range each call asks for, written down in call order, so that a restatement fed the
same stream must make the same decisions.  The `info` slot of every transition carries the slot it was written to, so the
`info` array a minibatch returns IS the index vector, which the class does not return otherwise.

    python tools/gen_golden_replay.py --reference /path/to/reference

Output: tests/golden/replay__wrap.npz -- a memory of 64 slots, 200 enqueues with about a quarter terminals, and a minibatch
of 32 at several fill states before and after the wrap: the inputs, the candidate stream, the five arrays and the indices.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, DIMO, DIMA, ENQUEUES, BATCH = 64, 5, 3, 200, 32
SAMPLE_AT = (9, 40, 63, 64, 70, 129, 200)          # enqueues done when a minibatch is taken


def load_reference(root):
    for name, kind in (("int", int), ("bool", bool)):
        if name not in np.__dict__:
            setattr(np, name, kind)
    path = os.path.join(root, "RL", "src", "replay_memory.py")
    spec = importlib.util.spec_from_file_location("reference_replay_memory", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ReplayMemory


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds RL/src/replay_memory.py)")
    args = ap.parse_args()
    rm = load_reference(args.reference)(SIZE, DIMO, DIMA)
    rng = np.random.RandomState(20)
    obs = rng.randn(ENQUEUES, DIMO).astype(np.float32)
    act = np.clip(rng.randn(ENQUEUES, DIMA) * 0.7, -1, 1)          # float64, not representable in float32
    rew = rng.randn(ENQUEUES).astype(np.float32)
    term = rng.rand(ENQUEUES) < 0.25
    term[:2] = False                                               # the first minibatch can draw index 0 .. n - 2
    stream_rng = np.random.RandomState(21)
    stream, out = [], {k: [] for k in ("o", "a", "r", "o2", "t2", "idx", "n", "i", "stream_end")}

    def recorded_randint(low, high):
        c = int(stream_rng.randint(low, high))
        stream.append(c)
        return c

    true_randint = np.random.randint
    for e in range(ENQUEUES):
        rm.enqueue(obs[e], term[e], act[e], rew[e], info=rm.i)
        if e + 1 in SAMPLE_AT:
            np.random.randint = recorded_randint
            try:
                o, a, r, o2, t2, info = rm.minibatch(BATCH)
            finally:
                np.random.randint = true_randint
            for k, v in (("o", o), ("a", a), ("r", r), ("o2", o2), ("t2", t2), ("idx", info.astype(np.int32)), ("n", rm.n),
                         ("i", rm.i), ("stream_end", len(stream))):
                out[k].append(np.array(v))
    assert out["a"][0].dtype == np.float32 and out["t2"][0].dtype == np.bool_
    path = os.path.join(REPO, "tests", "golden", "replay__wrap.npz")
    np.savez_compressed(
        path, size=np.int32(SIZE), batch=np.int32(BATCH), sample_at=np.array(SAMPLE_AT, np.int32), obs_in=obs, act_in=act,
        rew_in=rew, term_in=term.astype(np.uint8), stream=np.array(stream, np.int32),
        stream_end=np.array(out["stream_end"], np.int32), n=np.array(out["n"], np.int32), i=np.array(out["i"], np.int32),
        o=np.stack(out["o"]), a=np.stack(out["a"]), r=np.stack(out["r"]), o2=np.stack(out["o2"]),
        t2=np.stack(out["t2"]).astype(np.uint8), idx=np.stack(out["idx"]))
    print(path, os.path.getsize(path), "bytes;", len(stream), "candidates for", len(SAMPLE_AT) * BATCH, "samples; n", out["n"],
          "i", out["i"])


if __name__ == "__main__":
    main()
