"""Checkpoint files: save a trainer or the RL agent and resume it as if it had not stopped.

The reference saves `best.tf` (multi-label-cls/icnn_ebundle.py:274-277), one checkpoint per epoch
(completion/icnn_ebundle.py:300) and the RL agent's latest checkpoint (RL/src/icnn.py:134-137, RL/src/main.py:113-115) with
tf.train.Saver.  Here a checkpoint is one .npz of plain arrays (no pickles) that holds every piece of state a later step's
result depends on:

    every trainer        theta, Adam's m and v, the device step count; the BatchNorm moving statistics of a model that has them
    BundleTrainer        with skip_on_error, the gate words (the skipped count among them)
    CriticTrainer        also the target's theta and moving statistics (the critic update keeps no state beyond m, v, step),
                         and `opt`, `n_iter`: its inner optimiser; load() refuses a file of the other one (a file without
                         `opt` was written by the adam branch)
    ddpg.DDPGTrainer     the four flat nets (theta/q, theta/p, theta/target_q, theta/target_p), m and v of both nets, the step counts
    naf.NAFTrainer       the four flat nets (theta/l, theta/u, theta/v, theta/target_v), m and v of the three nets, the step count;
                         with bn=True the betas and their moments lie inside those, and bn/l, bn/u, bn/v are the moving pairs
    ff.FFTrainer         the flat theta/ff, m/ff, v/ff, the step count and the moving statistics bn/mean<i>, bn/var<i>
    fcn.FCNTrainer       the flat theta/fcn, m/fcn, v/fcn and the step count
    Agent, DDPGAgent, NAFAgent   its trainer, t, noise, observation, action, the RandomState (as arrays), the sampler's seed and,
                         with memory=True, the filled part of the four replay arrays and the control block (cursor, fill, draw
                         counter, status); memory=False leaves the memory out, as the reference's checkpoint does, and load()
                         then resets it.  An agent of n_envs environments also records n_envs, the device noise [E, dimA], the
                         exploration's step counter and seed, and its memory's arrays by time rows; load() refuses a file of
                         another n_envs, and a single-environment file for a vector agent or the other way round
    train.BestKeeper     best, the gate counters, the snapshots of theta and of the statistics
    train.DeviceDataset  seed, n_rows, the draw counter and the control block -- not the data: a resumed run rebuilds the
                         set from its arrays and continues the uninterrupted run's batch sequence

The arenas (the packed copies of theta the kernels read) are not stored: load() rewrites them from theta.

File layer (host only): write_arrays / read_arrays.  Every file carries `format` (FORMAT), and the files of save() a `kind`
string and the model spec as a JSON string in `spec`.

load() COPIES INTO THE EXISTING TENSORS: nothing is reallocated and no address changes, so a graph captured before the load
replays on the loaded state.  It checks format, kind, spec, every array's presence, shape and dtype (for the agent rmsize,
dimO and dimA too) BEFORE it writes anything; on a mismatch it raises ValueError naming the field and the object is bit for
bit what it was.
"""
import dataclasses
import json
import os
from typing import Dict

import numpy as np

FORMAT = 1


# --------------------------------------------------------------------------------------------- #
# The file layer
# --------------------------------------------------------------------------------------------- #
def write_arrays(path, arrays: Dict[str, np.ndarray]):
    """One .npz (np.savez) of `arrays` plus the key `format` (unless given).  Written to path + ".tmp" and moved over `path`
    with os.replace: a write that fails leaves an existing file as it was."""
    out = {"format": np.asarray(FORMAT, np.int64)}
    for k, v in arrays.items():
        a = np.asarray(v)
        if a.dtype == object:
            raise ValueError("%s: object arrays would need pickling" % k)
        out[k] = a
    path = os.fspath(path)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **out)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def read_arrays(path) -> Dict[str, np.ndarray]:
    """The arrays of a file of write_arrays (allow_pickle=False).  ValueError for a missing or unknown `format`."""
    with np.load(os.fspath(path), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    if "format" not in arrays or arrays["format"].shape != () or int(arrays["format"]) != FORMAT:
        raise ValueError("format: %s is not a checkpoint of format %d (found %s)"
                         % (path, FORMAT, arrays["format"].tolist() if "format" in arrays else "none"))
    return arrays


def spec_json(spec) -> str:
    """a model spec (a frozen dataclass of numbers, strings and tuples) as a JSON string"""
    d = dataclasses.asdict(spec)
    if d.get("tile_rows", 0) is None:       # FCSpec's default (the library picks the tile): files from before the field still match
        del d["tile_rows"]
    return json.dumps(d, sort_keys=True)


# --------------------------------------------------------------------------------------------- #
# What each object's state is made of
# --------------------------------------------------------------------------------------------- #
def _kind(obj) -> str:
    from . import ddpg, fcn, ff, ficnn, naf, rl_agent, rl_train, train
    for cls, kind in ((ff.FFTrainer, "FFTrainer"), (fcn.FCNTrainer, "FCNTrainer"), (train.BundleTrainer, "BundleTrainer"), (train.GDTrainer, "GDTrainer"),
                      (train.ConvGDTrainer, "ConvGDTrainer"), (ficnn.GDTrainer, "ficnn.GDTrainer"),
                      (rl_train.CriticTrainer, "CriticTrainer"), (rl_agent.Agent, "Agent"),
                      (ddpg.DDPGTrainer, "DDPGTrainer"), (rl_agent.DDPGAgent, "DDPGAgent"),
                      (naf.NAFTrainer, "NAFTrainer"), (rl_agent.NAFAgent, "NAFAgent")):
        if isinstance(obj, cls):
            return kind
    raise TypeError("checkpoint serves BundleTrainer, GDTrainer, ConvGDTrainer, ficnn.GDTrainer, CriticTrainer, Agent, "
                    "DDPGTrainer, DDPGAgent, NAFTrainer, NAFAgent, ff.FFTrainer and fcn.FCNTrainer, got %s" % type(obj).__name__)


FLAT_TRAINERS = ("DDPGTrainer", "NAFTrainer", "FFTrainer", "FCNTrainer")  # trainers whose state is flat vectors in dicts theta, m, v
AGENTS = {"Agent": "CriticTrainer", "DDPGAgent": "DDPGTrainer", "NAFAgent": "NAFTrainer"}     # an agent's kind -> its trainer's


def _model_stats(prefix, model, out):
    if getattr(model, "has_bn", False):
        for k in sorted(model.bn_stats):
            out[prefix + "bn/" + k] = model.bn_stats[k]


def _trainer_tensors(kind, obj) -> dict:
    """name -> the live device tensor, for everything of a trainer that is a device tensor"""
    if kind in FLAT_TRAINERS:
        out = {"theta/" + w: t for w, t in obj.theta.items()}
        for w in obj.m:
            out["m/" + w], out["v/" + w] = obj.m[w], obj.v[w]
        out["step"] = obj.step_count
        if kind == "FFTrainer":
            _model_stats("", obj.model, out)
        if getattr(obj, "bn", False):                           # naf.NAFTrainer(bn=True): a net's moving pairs, one vector
            for w, t in obj.mv.items():
                out["bn/" + w] = t
        return out
    out = {"theta": obj.opt.theta, "m": obj.opt.m, "v": obj.opt.v, "step": obj.opt.step_count}
    if kind == "CriticTrainer":
        _model_stats("", obj.critic, out)
        out["target/theta"] = obj.follower.theta
        _model_stats("target/", obj.target, out)
    else:
        _model_stats("", obj.model, out)
    if kind == "BundleTrainer" and obj.skip_on_error:
        out["gate"] = obj._gate
    return out


def _keeper_tensors(keeper) -> dict:
    out = {"keeper/best": keeper.best, "keeper/gate": keeper.gate, "keeper/theta": keeper.theta}
    if keeper.bn is not None:
        out["keeper/bn"] = keeper.bn
    return out


def _arena_owners(kind, obj, keeper):
    """(theta, arena, ParamMap) of every arena that load() rewrites from its theta"""
    if AGENTS.get(kind, kind) in FLAT_TRAINERS:              # their kernels read the flat vectors themselves
        return []
    trainer = obj.trainer if kind == "Agent" else obj
    owners = [(trainer.opt.theta, trainer.opt.arena, trainer.opt.map)]
    if kind in ("CriticTrainer", "Agent"):
        owners.append((trainer.follower.theta, trainer.follower.arena, trainer.follower.map))
    if keeper is not None:
        owners.append((keeper.theta, keeper.arena, keeper.opt.map))
    return owners


def _filled(memory) -> int:
    """rows of the replay arrays that hold a transition: the fill n before the cursor has wrapped, all of them after"""
    return memory.size if memory.n >= memory.size - 1 else memory.n


def _agent_host(agent, with_memory) -> dict:
    """the agent's host state, and the filled part of its memory, as arrays"""
    name, keys, pos, has_gauss, cached = agent.rng.get_state()
    if name != "MT19937":
        raise ValueError("the agent's RandomState is %s, not MT19937" % name)
    mem = agent.memory

    def optional(a, dtype=None):
        return np.zeros(0, np.float64) if a is None else np.array(a, dtype=dtype)

    out = {
        "agent/t": np.asarray(agent.t, np.int64), "agent/trained": np.asarray(int(agent._trained), np.int64),
        "agent/noise": np.array(agent.noise, np.float64) if agent.n_envs is None else agent.explorer.noise.cpu().numpy(),
        "agent/has_observation": np.asarray(int(agent.observation is not None), np.int64),
        "agent/observation": optional(agent.observation),
        "agent/has_action": np.asarray(int(agent.action is not None), np.int64),
        "agent/action": optional(agent.action),
        "rng/keys": np.asarray(keys, np.uint32), "rng/pos": np.asarray(pos, np.int64),
        "rng/has_gauss": np.asarray(has_gauss, np.int64), "rng/cached_gaussian": np.asarray(cached, np.float64),
        "memory/rmsize": np.asarray(mem.size, np.int64), "memory/dimO": np.asarray(mem.dimO, np.int64),
        "memory/dimA": np.asarray(mem.dimA, np.int64), "memory/seed": np.asarray(mem.seed, np.uint64),
        "memory/saved": np.asarray(int(with_memory), np.int64),
    }
    if agent.n_envs is not None:       # E environments a step: the file says so, and carries the device noise's step counter
        out["agent/n_envs"] = np.asarray(agent.n_envs, np.int64)
        out["explore/counter"] = agent.explorer.counter.cpu().numpy()
        out["explore/seed"] = np.asarray(agent.explorer.seed, np.uint64)
    if with_memory:
        rows = _filled(mem)
        out["memory/ctrl"] = mem.ctrl.cpu().numpy()
        out["memory/observations"] = mem.observations[:rows].cpu().numpy()
        out["memory/actions"] = mem.actions[:rows].cpu().numpy()
        out["memory/rewards"] = mem.rewards[:rows].cpu().numpy()
        out["memory/terminals"] = mem.terminals[:rows].cpu().numpy()
    return out


def _torch_dtype_name(t) -> str:
    return str(t.dtype).replace("torch.", "")


# --------------------------------------------------------------------------------------------- #
# save / load
# --------------------------------------------------------------------------------------------- #
def _dataset_host(dataset) -> dict:
    """the control block of a train.DeviceDataset and what identifies its stream, as arrays (reads the device)"""
    ctrl = dataset.ctrl.cpu().numpy()
    return {"data/seed": np.asarray(dataset.seed, np.uint64), "data/n_rows": np.asarray(dataset.n_rows, np.int64),
            "data/draws": np.asarray(int(ctrl[0]), np.int64), "data/ctrl": ctrl}


def save(path, obj, keeper=None, memory=True, dataset=None):
    """Write a checkpoint of `obj` (and of `keeper`, a train.BestKeeper on it, and of `dataset`, the train.DeviceDataset that
    feeds it) to `path`.  Reads the device: one wait.  memory (the Agent only): include the replay memory."""
    kind = _kind(obj)
    trainer = obj.trainer if kind in AGENTS else obj
    if keeper is not None and keeper.opt is not trainer.opt:
        raise ValueError("keeper: it keeps another trainer's model")
    arrays = {"kind": np.asarray(kind), "spec": np.asarray(spec_json(trainer.spec)),
              "has_keeper": np.asarray(int(keeper is not None), np.int64)}
    if AGENTS.get(kind, kind) == "CriticTrainer":             # the inner optimiser the step was run with (FLAGS.icnn_opt)
        arrays["opt"], arrays["n_iter"] = np.asarray(trainer.opt_name), np.asarray(trainer.n_iter, np.int64)
    tensors = _trainer_tensors(AGENTS.get(kind, kind), trainer)
    if keeper is not None:
        arrays["keeper/mode"] = np.asarray(keeper.mode)
        tensors.update(_keeper_tensors(keeper))
    for name, t in tensors.items():
        arrays[name] = t.detach().cpu().numpy()
    if kind in AGENTS:
        arrays.update(_agent_host(obj, bool(memory)))
    if dataset is not None:
        arrays.update(_dataset_host(dataset))
    write_arrays(path, arrays)


def save_best(path, keeper):
    """The kept model of a train.BestKeeper as a file of its own (the reference's best.tf): kind "best", the spec, `best`,
    the weights as theta/<name> keyed like grad_layout and the BatchNorm moving statistics as bn/<name>.  One wait."""
    arrays = {"kind": np.asarray("best"), "spec": np.asarray(spec_json(keeper.opt.spec)),
              "best": np.asarray(keeper.best_value(), np.float64), "mode": np.asarray(keeper.mode)}
    for name, a in keeper.host_params().items():
        arrays["theta/" + name] = a
    for name, a in keeper.bn_stats().items():
        arrays["bn/" + name] = a
    write_arrays(path, arrays)


def _scalar(arrays, name, dtype_kind="iu"):
    if name not in arrays:
        raise ValueError("%s: missing from the file" % name)
    a = arrays[name]
    if a.shape != () or a.dtype.kind not in dtype_kind:
        raise ValueError("%s: not a scalar of the expected type (shape %s, dtype %s)" % (name, a.shape, a.dtype))
    return a.item()


def _check_array(arrays, name, shape, dtype):
    if name not in arrays:
        raise ValueError("%s: missing from the file" % name)
    a = arrays[name]
    if tuple(a.shape) != tuple(shape):
        raise ValueError("%s: shape %s in the file, %s here" % (name, tuple(a.shape), tuple(shape)))
    if a.dtype != np.dtype(dtype):
        raise ValueError("%s: dtype %s in the file, %s here" % (name, a.dtype, np.dtype(dtype)))
    return a


def load(path, obj, keeper=None, dataset=None):
    """Copy the checkpoint at `path` into `obj` (and `keeper`, and `dataset`): into the existing tensors, so captured graphs
    stay valid.  Everything is checked first; a ValueError names the field that does not fit and nothing has been written
    then.  A dataset's seed and row count must be the file's (a captured draw carries them), and the file holds a dataset's
    state exactly when the call gives one."""
    import torch
    kind = _kind(obj)
    trainer = obj.trainer if kind in AGENTS else obj
    if keeper is not None and keeper.opt is not trainer.opt:
        raise ValueError("keeper: it keeps another trainer's model")
    arrays = read_arrays(path)
    # ---- checks: nothing is written before all of them pass ----
    for name in ("kind", "spec"):
        if name not in arrays or arrays[name].shape != () or arrays[name].dtype.kind != "U":
            raise ValueError("%s: missing from the file or not a string" % name)
    if str(arrays["kind"]) != kind:
        raise ValueError("kind: the file holds a %s, the object is a %s" % (arrays["kind"], kind))
    if str(arrays["spec"]) != spec_json(trainer.spec):
        raise ValueError("spec: the file's model is %s, the object's %s" % (arrays["spec"], spec_json(trainer.spec)))
    if AGENTS.get(kind, kind) == "CriticTrainer":             # a file from before the bundle-entropy branch is an adam one
        if "opt" in arrays and (arrays["opt"].shape != () or arrays["opt"].dtype.kind != "U"):
            raise ValueError("opt: not a string")
        opt = str(arrays["opt"]) if "opt" in arrays else "adam"
        if opt != trainer.opt_name:
            raise ValueError("opt: the file was written with the %s inner optimiser, this object runs %s" % (opt, trainer.opt_name))
        if opt == "bundle_entropy" and _scalar(arrays, "n_iter") != trainer.n_iter:
            raise ValueError("n_iter: %d in the file, %d here" % (_scalar(arrays, "n_iter"), trainer.n_iter))
    has_keeper = bool(_scalar(arrays, "has_keeper"))
    if has_keeper != (keeper is not None):
        raise ValueError("keeper: the file %s a keeper's state, the call %s a keeper"
                         % ("holds" if has_keeper else "does not hold", "gives" if keeper is not None else "gives no"))
    tensors = _trainer_tensors(AGENTS.get(kind, kind), trainer)
    if keeper is not None:
        if "keeper/mode" not in arrays or str(arrays["keeper/mode"]) != keeper.mode:
            raise ValueError("keeper/mode: the file's keeper is %s, this one %r" % (arrays.get("keeper/mode"), keeper.mode))
        tensors.update(_keeper_tensors(keeper))
    for name, t in tensors.items():
        _check_array(arrays, name, t.shape, _torch_dtype_name(t))
    state_prefixes = ("bn/", "target/", "keeper/")
    for name in arrays:                                         # state in the file that this object has no place for
        if (name in ("gate",) or name.startswith(state_prefixes)) and name not in tensors and name != "keeper/mode":
            raise ValueError("%s: in the file, but this object keeps no such state" % name)
    has_data = any(name.startswith("data/") for name in arrays)
    if has_data != (dataset is not None):
        raise ValueError("dataset: the file %s a dataset's state, the call %s a dataset"
                         % ("holds" if has_data else "does not hold", "gives" if dataset is not None else "gives no"))
    if dataset is not None:
        for name, mine in (("data/n_rows", dataset.n_rows), ("data/seed", dataset.seed)):
            if _scalar(arrays, name) != mine:
                raise ValueError("%s: %d in the file, %d here" % (name, _scalar(arrays, name), mine))
        data_ctrl = _check_array(arrays, "data/ctrl", dataset.ctrl.shape, np.int32)
        if _scalar(arrays, "data/draws") != int(data_ctrl[0]):
            raise ValueError("data/draws: %d in the file, its control block says %d" % (_scalar(arrays, "data/draws"), data_ctrl[0]))
    host = None
    if kind in AGENTS:
        mem = obj.memory
        E = obj.n_envs
        file_envs = _scalar(arrays, "agent/n_envs") if "agent/n_envs" in arrays else None
        if file_envs != E:
            raise ValueError("n_envs: the file is of %s, the object of %s" % tuple(
                "a single-environment agent" if e is None else "an agent of %d environments" % e for e in (file_envs, E)))
        for name, mine in (("memory/rmsize", mem.size), ("memory/dimO", mem.dimO), ("memory/dimA", mem.dimA)):
            if _scalar(arrays, name) != mine:
                raise ValueError("%s: %d in the file, %d here" % (name.split("/")[1], _scalar(arrays, name), mine))
        host = {k: _scalar(arrays, "agent/" + k) for k in ("t", "trained", "has_observation", "has_action")}
        host["seed"] = _scalar(arrays, "memory/seed")
        host["saved"] = bool(_scalar(arrays, "memory/saved"))
        _check_array(arrays, "agent/noise", (obj.dimA,) if E is None else (E, obj.dimA), np.float64)
        if E is not None:
            _check_array(arrays, "explore/counter", (1,), np.int32)
            host["explore_seed"] = _scalar(arrays, "explore/seed")
        for name in ("agent/observation", "agent/action"):
            if name not in arrays:
                raise ValueError("%s: missing from the file" % name)
        if host["has_observation"] and arrays["agent/observation"].size != (E or 1) * obj.dimO:
            raise ValueError("agent/observation: %d values in the file, dimO is %d" % (arrays["agent/observation"].size, obj.dimO))
        if host["has_action"] and arrays["agent/action"].size != (E or 1) * obj.dimA:
            raise ValueError("agent/action: %d values in the file, dimA is %d" % (arrays["agent/action"].size, obj.dimA))
        _check_array(arrays, "rng/keys", (624,), np.uint32)
        _check_array(arrays, "rng/cached_gaussian", (), np.float64)
        host["pos"], host["has_gauss"] = _scalar(arrays, "rng/pos"), _scalar(arrays, "rng/has_gauss")
        if host["saved"]:
            ctrl = _check_array(arrays, "memory/ctrl", mem.ctrl.shape, np.int32)
            cursor, fill = int(ctrl[0]), int(ctrl[1])
            if not (0 <= cursor < mem.size and 0 <= fill <= mem.size - 1):
                raise ValueError("memory/ctrl: cursor %d and fill %d lie outside a memory of %d" % (cursor, fill, mem.size))
            rows = mem.size if fill >= mem.size - 1 else fill
            for name, t in (("observations", mem.observations), ("actions", mem.actions), ("rewards", mem.rewards),
                            ("terminals", mem.terminals)):
                _check_array(arrays, "memory/" + name, (rows,) + tuple(t.shape[1:]), _torch_dtype_name(t))
    # ---- the copies ----
    with torch.no_grad():
        for name, t in tensors.items():
            t.copy_(torch.from_numpy(arrays[name]))
        for theta, arena, pmap in _arena_owners(kind, obj, keeper):
            arena.copy_(torch.from_numpy(pmap.scatter(theta.cpu().numpy())))
        if dataset is not None:
            dataset.ctrl.copy_(torch.from_numpy(arrays["data/ctrl"]))
            dataset.draws = int(arrays["data/ctrl"][0])
        if kind in AGENTS:
            mem = obj.memory
            obj.t, obj._trained = int(host["t"]), bool(host["trained"])
            obj.observation = arrays["agent/observation"].copy() if host["has_observation"] else None
            obj.action = arrays["agent/action"].copy() if host["has_action"] else None
            if obj.n_envs is None:
                obj.noise = arrays["agent/noise"].copy()
            else:                                               # the device side of the vector cycle
                ex = obj.explorer
                ex.noise.copy_(torch.from_numpy(arrays["agent/noise"]))
                ex.counter.copy_(torch.from_numpy(arrays["explore/counter"]))
                ex.seed = int(host["explore_seed"])
                if obj.observation is not None:
                    obj.observation = obj.observation.astype(np.float32).reshape(obj.n_envs, obj.dimO)
                    obj._obs_dev.copy_(torch.from_numpy(obj.observation))
                if obj.action is not None:
                    ex.action.copy_(torch.from_numpy(obj.action.reshape(obj.n_envs, obj.dimA)))
            obj.rng.set_state(("MT19937", arrays["rng/keys"], int(host["pos"]), int(host["has_gauss"]),
                               float(arrays["rng/cached_gaussian"])))
            if int(host["seed"]) != mem.seed:                   # a captured sampler launch carries the seed it was captured with
                mem.seed = int(host["seed"])
                obj._graph = None
            if host["saved"]:
                for name, t in (("observations", mem.observations), ("actions", mem.actions), ("rewards", mem.rewards),
                                ("terminals", mem.terminals)):
                    a = arrays["memory/" + name]
                    t[:a.shape[0]].copy_(torch.from_numpy(a))
                    t[a.shape[0]:].zero_()
                mem.ctrl.copy_(torch.from_numpy(arrays["memory/ctrl"]))
                mem.i, mem.n = int(arrays["memory/ctrl"][0]), int(arrays["memory/ctrl"][1])
            else:
                mem.reset()
