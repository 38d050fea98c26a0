"""What the C entries that are defined beside their kernels refuse, and with which code.

Every call here is refused before anything is launched: a NULL descriptor, each required pointer NULL, each pointer that
must be 8- or 16-byte aligned off by 4, each size at 0 and one past its limit, each constant at a bad value, the stream at
address 4.  The pointers are made-up integer addresses; a refusing path dereferences none of them, so the module needs no
GPU.  No well-formed call is made.  The expected codes are those of the library before the entries moved out of be_api.hip:
ICNN_BE_EINVAL unless a case says otherwise, 0 from a size query, and 0 from the entries that return early on an empty batch.
"""
import ctypes as C

import pytest

from icnn_amd import _lib

EINVAL, ELIMIT = -1, -2
NAN, INF = float("nan"), float("inf")
BIG = (65536, 32768)                     # two ints whose product is 2^31


def P(k):
    """A made-up address, a multiple of 256."""
    return 0x100000 + 0x100 * k


def fill(cls, **kw):
    """A descriptor with every pointer field at an address of its own."""
    s = cls()
    for i, (name, typ) in enumerate(cls._fields_):
        if typ is C.c_void_p:
            setattr(s, name, P(i + 1))
    for name, v in kw.items():
        setattr(s, name, v)
    return s


def pointers(cls, skip=()):
    return [name for name, typ in cls._fields_ if typ is C.c_void_p and name not in skip]


def put(args, path, value):
    """path: the index of an argument, or (index, field or element, ...) into a descriptor or an array."""
    if isinstance(path, int):
        args[path] = value
        return
    obj = args[path[0]]
    for key in path[1:-1]:
        obj = getattr(obj, key) if isinstance(key, str) else obj[key]
    if isinstance(path[-1], str):
        setattr(obj, path[-1], value)
    else:
        obj[path[-1]] = value


def get(args, path):
    if isinstance(path, int):
        return args[path]
    obj = args[path[0]]
    for key in path[1:]:
        obj = getattr(obj, key) if isinstance(key, str) else obj[key]
    return obj


ENTRIES = {}


def entry(name, make, null=(), align=(), zero=(), over=(), bad=(), stream=None, other=(), expect=EINVAL):
    """The refused calls of one entry.  make() gives the arguments of a well-formed call (never made); each case changes them:
    null: paths set to NULL; align: paths of 8- / 16-byte aligned pointers moved by 4; zero: sizes set to 0; over: (path, limit)
    set to limit + 1; bad: (path, value); stream: its index, set to 4; other: (label, [(path, value), ...], code)."""
    cases = [("null %s" % (p,), [(p, None)], expect) for p in null]
    cases += [("misaligned %s" % (p,), [(p, "+4")], expect) for p in align]
    cases += [("zero %s" % (p,), [(p, 0)], expect) for p in zero]
    cases += [("over %s" % (p,), [(p, limit + 1)], expect) for p, limit in over]
    cases += [("bad %s = %r" % (p, v), [(p, v)], expect) for p, v in bad]
    if stream is not None:
        cases.append(("stream", [(stream, 4)], expect))
    cases += list(other)
    assert name not in ENTRIES and cases
    ENTRIES[name] = (make, cases)


def field(*names, at=0):
    return [(at, n) for n in names]


# ---- the replay-step descriptors: DDPG, NAF, NAF with BatchNorm ----
SIZES = dict(batch=4, dimO=3, dimA=2, l1=8, l2=8)
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)
STEP = dict(rate=1e-3, tau=1e-3, discount=0.99, l2norm=0.0, **ADAM)
STEP_BAD = field("tau", "beta1", "beta2", "eps", "rate", "discount", "l2norm", "l2norm")
STEP_BAD = list(zip(STEP_BAD, (1.5, 1.0, -0.1, 0.0, NAN, INF, -1.0, INF)))


def dims(limits, first=0):
    """(zero, over) of four consecutive int arguments dimO, dimA, l1, l2"""
    return list(range(first, first + 4)), [(first + i, m) for i, m in enumerate(limits)]


def step_entries(prefix, cls, make, limits, bad, batch_limit=None):
    nets = pointers(cls, skip=("obs", "act", "rew", "ob2", "term", "step", "loss", "work", "mv_l", "mv_u", "mv_v"))
    over = [((0, n), m) for n, m in zip(("dimO", "dimA", "l1", "l2"), limits)]
    if batch_limit:
        over.append(((0, "batch"), batch_limit))
    for name in ("chain", "grads", "update", "step"):
        loss = ("loss",) if name == "step" else ()          # elsewhere loss may be NULL
        entry(prefix + name, lambda: [make(), None], null=[0] + field(*pointers(cls, skip=("loss",)), *loss),
              align=field("act", "work", *nets), zero=field("batch", "dimO", "dimA", "l1", "l2"), over=over,
              bad=STEP_BAD + bad, stream=1)


DDPG_LIMITS = (_lib.DDPG_MAX_OBS, _lib.DDPG_MAX_ACT, _lib.DDPG_MAX_HIDDEN, _lib.DDPG_MAX_HIDDEN)
NAF_LIMITS = (_lib.NAF_MAX_OBS, _lib.NAF_MAX_ACT, _lib.NAF_MAX_HIDDEN, _lib.NAF_MAX_HIDDEN)
D4 = [3, 2, 8, 8]                        # dimO, dimA, l1, l2


def ll(n=1):
    return [C.byref(C.c_longlong()) for _ in range(n)]          # a host out-parameter is declared void *: no implicit byref


step_entries("icnn_be_ddpg_", _lib.DdpgArgs, lambda: fill(_lib.DdpgArgs, prate=1e-4, pl2norm=0.0, **SIZES, **STEP), DDPG_LIMITS,
             list(zip(field("pl2norm", "pl2norm", "prate"), (-1.0, INF, NAN))))
zero, over = dims(DDPG_LIMITS)
entry("icnn_be_ddpg_param_floats", lambda: D4 + ll(2), null=[4, 5], zero=zero, over=over)
entry("icnn_be_ddpg_act", lambda: D4 + [P(1), P(2), 4, P(3), None], null=[4, 5, 7], align=[4], zero=zero + [6], over=over,
      stream=8)
entry("icnn_be_ddpg_q", lambda: D4 + [P(1), P(2), P(3), 4, P(4), None], null=[4, 5, 6, 8], align=[4, 6], zero=zero + [7],
      over=over, stream=9)
zero, over = dims(DDPG_LIMITS, 1)
entry("icnn_be_ddpg_work_bytes", lambda: [4] + D4, zero=[0] + zero, over=over, expect=0)
entry("icnn_be_ddpg_work_offsets", lambda: [4] + D4 + [(C.c_longlong * len(_lib.DDPG_WORK))()], null=[5], zero=[0] + zero,
      over=over)

step_entries("icnn_be_naf_", _lib.NafArgs, lambda: fill(_lib.NafArgs, **SIZES, **STEP), NAF_LIMITS, [])
zero, over = dims(NAF_LIMITS)
entry("icnn_be_naf_param_floats", lambda: D4 + ll(3), null=[4, 5, 6], zero=zero, over=over)
entry("icnn_be_naf_act", lambda: D4 + [P(1), P(2), 4, P(3), None], null=[4, 5, 7], align=[4], zero=zero + [6], over=over,
      stream=8)
entry("icnn_be_naf_q", lambda: D4 + [P(1), P(2), P(3), P(4), P(5), 4, P(6), None], null=[4, 5, 6, 7, 8, 10], align=[4, 5, 6, 8],
      zero=zero + [9], over=over, stream=11)
zero, over = dims(NAF_LIMITS, 1)
entry("icnn_be_naf_work_bytes", lambda: [4] + D4, zero=[0] + zero, over=over, expect=0)
entry("icnn_be_naf_work_offsets", lambda: [4] + D4 + [(C.c_longlong * len(_lib.NAF_WORK))()], null=[5], zero=[0] + zero,
      over=over)

step_entries("icnn_be_naf_bn_", _lib.NafBnArgs, lambda: fill(_lib.NafBnArgs, bn_decay=0.9, bn_eps=1e-5, **SIZES, **STEP),
             NAF_LIMITS, list(zip(field("bn_eps", "bn_decay", "bn_decay"), (0.0, 1.5, NAN))), batch_limit=_lib.NAF_BN_MAX_BATCH)
zero, over = dims(NAF_LIMITS)
entry("icnn_be_naf_bn_param_floats", lambda: D4 + ll(5), null=[4, 5, 6, 7, 8], zero=zero, over=over)
entry("icnn_be_naf_bn_layout", lambda: D4 + [1, (C.c_longlong * len(_lib.NAF_BN_VARS))()], null=[5], zero=zero, over=over,
      bad=[(4, -1), (4, 3)])
entry("icnn_be_naf_bn_act", lambda: D4 + [P(1), P(2), 1e-5, 0, P(3), 4, P(4), P(5), None], null=[4, 5, 8, 10, 11],
      align=[4, 11], zero=zero + [9], over=over + [(9, _lib.NAF_BN_MAX_BATCH)], bad=[(6, 0.0), (7, 2)], stream=12)
entry("icnn_be_naf_bn_q", lambda: D4 + [P(i) for i in range(1, 7)] + [1e-5, 1, P(7), P(8), 4, P(9), P(10), None],
      null=[4, 5, 6, 7, 8, 9, 12, 13, 15, 16], align=[4, 5, 6, 13, 16], zero=zero + [14],
      over=over + [(14, _lib.NAF_BN_MAX_BATCH)], bad=[(10, 0.0), (11, 2)], stream=17)
zero, over = dims(NAF_LIMITS, 1)
over.append((0, _lib.NAF_BN_MAX_BATCH))
entry("icnn_be_naf_bn_work_bytes", lambda: [4] + D4, zero=[0] + zero, over=over, expect=0)
entry("icnn_be_naf_bn_work_offsets", lambda: [4] + D4 + [(C.c_longlong * len(_lib.NAF_BN_WORK))()], null=[5], zero=[0] + zero,
      over=over)


# ---- the feed-forward baseline ----
def ff_args():
    a = fill(_lib.FfArgs, batch=8, n_features=5, n_labels=3, n_layers=2, lr=1e-3, bn_eps=1e-5, **ADAM)
    a.width[0], a.width[1] = 6, 7
    for i in range(_lib.MAX_LAYERS):
        a.mv.mean[i], a.mv.var[i] = P(40 + i), P(60 + i)
    a.mv.decay = 0.9
    return a


def ff_entry(name, need, train_batch, adam=False, moving=False, mode=None):
    """need: the pointer fields the entry requires; true_y is not among forward's, where a NULL one selects another form"""
    make = (lambda: [ff_args(), None]) if mode is None else (lambda: [ff_args(), mode, None])
    null = [0] + field(*need)
    bad = [((0, "bn_eps"), 0.0)]
    over = [((0, "n_features"), _lib.FF_MAX_FEATURES), ((0, "n_labels"), _lib.FF_MAX_WIDTH), ((0, "n_layers"), _lib.FF_MAX_LAYERS),
            ((0, "width", 1), _lib.FF_MAX_WIDTH)]
    if train_batch:
        bad.append(((0, "batch"), 1))
        over.append(((0, "batch"), _lib.FF_MAX_BATCH))
    if adam:
        bad += list(zip(field("beta1", "beta2", "eps", "lr", "lr"), (1.0, -0.1, 0.0, NAN, INF)))
    if moving:
        null += [(0, "mv", "mean", 0), (0, "mv", "var", 1)]
        bad += [((0, "mv", "decay"), 1.5), ((0, "mv", "decay"), NAN)]
    if mode is not None:
        bad += [(1, 2), (1, -1)]
    entry(name, make, null=null, align=field(*(n for n in need if n in ("theta", "work", "grad", "m", "v"))),
          zero=field("batch", "n_features", "n_labels", "n_layers") + [(0, "width", 0)], over=over, bad=bad,
          stream=1 if mode is None else 2)


ff_entry("icnn_be_ff_forward", ("theta", "work", "x", "yhat", "loss"), True, mode=0)
ff_entry("icnn_be_ff_backward", ("theta", "work", "grad"), True)
ff_entry("icnn_be_ff_grads", ("theta", "x", "work", "grad"), True)
ff_entry("icnn_be_ff_update", ("theta", "grad", "m", "v", "step"), False, adam=True)
ff_entry("icnn_be_ff_step", ("theta", "x", "true_y", "yhat", "loss", "m", "v", "grad", "step", "work"), True, adam=True, moving=True)
ff_entry("icnn_be_ff_eval", ("theta", "x", "true_y", "yhat", "loss", "work"), False, moving=True)


def widths():
    return (C.c_int * _lib.FF_MAX_LAYERS)(6, 7, 0, 0)


def ff_dims(first):
    zero = [first, first + 1, first + 2, (first + 3, 0)]
    over = [(first, _lib.FF_MAX_FEATURES), (first + 1, _lib.FF_MAX_WIDTH), (first + 2, _lib.FF_MAX_LAYERS),
            ((first + 3, 1), _lib.FF_MAX_WIDTH)]
    return zero, over


zero, over = ff_dims(0)
entry("icnn_be_ff_param_floats", lambda: [5, 3, 2, widths()] + ll(), null=[3, 4], zero=zero, over=over)
zero, over = ff_dims(1)
entry("icnn_be_ff_work_bytes", lambda: [8, 5, 3, 2, widths()], null=[4], zero=[0] + zero, over=over, expect=0)
entry("icnn_be_ff_work_offsets", lambda: [8, 5, 3, 2, widths(), (C.c_longlong * len(_lib.FF_WORK))()], null=[4, 5],
      zero=[0] + zero, over=over)


# ---- the replay memories and the exploration noise ----
def replay():
    return fill(_lib.Replay, size=100, dimO=3, dimA=2)


def vec_replay(**kw):
    return fill(_lib.VecReplay, **dict(dict(steps=100, n_envs=4, dimO=3, dimA=2), **kw))


MEMORY = ("observations", "actions", "rewards", "terminals", "ctrl")
entry("icnn_be_replay_enqueue", lambda: [replay(), P(20), None], null=[0, 1] + field(*MEMORY), align=[1],
      zero=field("size", "dimO", "dimA"), bad=[((0, "size"), 2)], stream=2)
entry("icnn_be_replay_sample", lambda: [replay(), 50, 8, 7] + [P(20 + i) for i in range(6)] + [None],
      null=[0, 4, 5, 6, 7, 8, 9] + field(*MEMORY), align=[5], zero=field("size", "dimO", "dimA") + [2],
      bad=[(1, 1), (1, 100), ((0, "size"), 2)], stream=10)
over_idx = ("index beyond an int", [((0, "steps"), BIG[0]), ((0, "n_envs"), BIG[1])], ELIMIT)
over_idx_null = ("index beyond an int, a NULL array", over_idx[1] + [((0, "ctrl"), None)], ELIMIT)
entry("icnn_be_vec_replay_enqueue", lambda: [vec_replay()] + [P(20 + i) for i in range(4)] + [None],
      null=[0, 1, 2, 3, 4] + field(*MEMORY), align=[2], zero=field("steps", "n_envs", "dimO", "dimA"), bad=[((0, "steps"), 2)],
      stream=5, other=[over_idx, over_idx_null])
entry("icnn_be_vec_replay_sample", lambda: [vec_replay(), 50, 8, 7] + [P(20 + i) for i in range(6)] + [None],
      null=[0, 4, 5, 6, 7, 8, 9] + field(*MEMORY), align=[5], zero=field("steps", "n_envs", "dimO", "dimA") + [2],
      bad=[(1, 1), (1, 100), ((0, "steps"), 2)], stream=10, other=[over_idx, over_idx_null])
entry("icnn_be_explore", lambda: [4, 2, P(1), 0, P(2), P(3), 0.15, 0.2, 7, 0, P(4), None], null=[2, 4, 5, 10],
      align=[2, 4, 10], zero=[0, 1], bad=[(6, NAN), (7, NAN)], stream=11,
      other=[("count beyond an int", [(0, BIG[0]), (1, BIG[1])], ELIMIT),
             ("count beyond an int, theta NaN", [(0, BIG[0]), (1, BIG[1]), (6, NAN)], ELIMIT),
             ("count beyond an int, raw NULL", [(0, BIG[0]), (1, BIG[1]), (2, None)], EINVAL)])


# ---- the training set and the step log ----
def dataset():
    d = fill(_lib.Dataset, n_rows=50, n_arrays=2)
    for i in range(_lib.DATASET_MAX_ARRAYS):
        d.src[i], d.row_words[i] = P(30 + i), 4
    return d


def step_log():
    L = fill(_lib.StepLog, cap=16, width=2)
    for i in range(_lib.LOG_MAX_COLUMNS):
        L.col[i], L.kind[i] = P(30 + i), _lib.LOG_KIND["float64"]
    return L


def draw_dst():
    return (C.c_void_p * _lib.DATASET_MAX_ARRAYS)(*[P(50 + i) for i in range(_lib.DATASET_MAX_ARRAYS)])


entry("icnn_be_dataset_draw", lambda: [dataset(), 8, 7, draw_dst(), P(60), None],
      null=[0, 3, 4, (0, "ctrl"), (0, "src", 0), (3, 1)], align=[4, (0, "src", 1), (3, 0)],
      zero=[1, (0, "n_rows"), (0, "n_arrays"), (0, "row_words", 1)], over=[((0, "n_arrays"), _lib.DATASET_MAX_ARRAYS)], stream=5)
entry("icnn_be_log_row", lambda: [step_log(), None], null=[0, (0, "rows"), (0, "ctrl"), (0, "col", 1)],
      align=[(0, "rows"), (0, "col", 0)], zero=field("cap", "width"), over=[((0, "width"), _lib.LOG_MAX_COLUMNS)],
      bad=[((0, "kind", 0), -1), ((0, "kind", 1), 3)], stream=1)


# ---- parameter updates and the RL critic's loss ----
def update_args(cls=_lib.ParamUpdateArgs):
    return fill(cls, n=1000, arena_floats=4000, lr=1e-3, n_proj=0, **ADAM)


def rl_update_args():
    a = fill(_lib.RlUpdateArgs, tau=1e-3, l2norm=0.0, wd=1e-4)
    a.adam = update_args()
    return a


def update_cases(at):
    """null, align, zero, over, bad, other of an icnn_be_param_update_args at path `at`"""
    f = lambda *names: [at + (n,) for n in names]
    return dict(null=f("theta", "m", "v", "grad", "dest_off", "dest", "arena", "step"), align=f("theta", "m", "v", "grad", "dest_off"),
                zero=f("n"), over=[(at + ("arena_floats",), 2 ** 31 - 1), (at + ("n_proj",), _lib.MAX_PROJ_RANGES)],
                bad=list(zip(f("arena_floats", "n_proj", "beta1", "beta2", "eps", "lr"), (-1, -1, 1.0, -0.1, 0.0, NAN))),
                other=[("projection range", [(at + ("n_proj",), 1), (at + ("proj_begin", 0), 5), (at + ("proj_end", 0), 4)], EINVAL),
                       ("projection past n", [(at + ("n_proj",), 1), (at + ("proj_end", 0), 1001)], EINVAL)])


u = update_cases((0,))
entry("icnn_be_param_update", lambda: [update_args(), None], **dict(u, null=[0] + u["null"]))
entry("icnn_be_param_update_gated", lambda: [update_args(), P(30), None], **dict(u, null=[0, 1] + u["null"]))
u = update_cases((0, "adam"))
entry("icnn_be_rl_critic_update", lambda: [rl_update_args(), None],
      **dict(u, null=[0] + u["null"] + field("target_theta", "target_arena", "decay"), align=u["align"] + field("target_theta"),
             bad=u["bad"] + list(zip(field("tau", "tau", "l2norm", "l2norm", "wd", "wd"), (1.5, -0.1, -1.0, INF, -1.0, INF))),
             stream=1))
entry("icnn_be_gated_copy", lambda: [P(1), P(2), 100, P(3), 1, None], null=[0, 1, 3], bad=[(2, -1)],
      other=[("nothing to copy", [(2, 0)], 0)])
# batch, n, e_critic, act, rew, term, q2_src, act2, discount, theta, n_theta, decay, l2norm, wd, td, c, loss, work, stream
entry("icnn_be_rl_td", lambda: [8, 3, P(1), P(2), P(3), P(4), P(5), P(6), 0.99, P(7), 1000, P(8), 0.0, 1e-4, P(9), P(10), P(11),
                                P(12), None],
      null=[2, 3, 4, 5, 6, 9, 11, 14, 15, 16, 17], align=[3, 7, 15, 17], zero=[0, 1, 10], over=[(10, 2 ** 31 - 1)],
      bad=[(8, NAN), (8, INF), (12, -1.0), (12, INF), (13, -1.0), (13, INF)], stream=18)

# ---- the feeds and the epoch level of the training steps ----
entry("icnn_be_feed_plan_work_bytes", lambda: [8], bad=[(0, -1)], expect=0)
entry("icnn_be_feed_pad", lambda: [P(1), 8, 5, 64, P(2), P(3), P(4), P(5), None], null=[0, 4, 5, 6, 7], zero=[1, 2], bad=[(3, -1)],
      other=[("no rows", [(3, 0)], 0)])
entry("icnn_be_step_gate", lambda: [P(1), 15, P(2), None], null=[0, 2])
entry("icnn_be_gd_feed_work_bytes", lambda: [8], bad=[(0, -1)], expect=0)
# yK, t, coef, B, n, K, scale, v_rows, c_rows, row_offset, loss, f1_tallies, work, stream
entry("icnn_be_gd_feed", lambda: [P(1), P(2), P(3), 8, 5, 4, 0.025, P(4), P(5), P(6), P(7), P(8), P(9), None],
      null=[0, 1, 2, 7, 8, 9, 10, 12], zero=[3, 4, 5],
      other=[("rows beyond an int", [(3, BIG[0]), (5, BIG[1])], ELIMIT),
             ("rows beyond an int, yK NULL", [(3, BIG[0]), (5, BIG[1]), (0, None)], EINVAL)])
entry("icnn_be_gd_feed_px_work_bytes", lambda: [8, 5, 4], zero=[0, 1, 2], bad=[(0, -1)], expect=0)
# yK, t, coef, B, n, K, scale, px, v_rows, c_rows, row_offset, loss, work, stream
entry("icnn_be_gd_feed_px", lambda: [P(1), P(2), P(3), 8, 5, 4, 0.025, 255.0, P(4), P(5), P(6), P(7), P(8), None],
      null=[0, 1, 2, 8, 9, 10, 11, 12], zero=[3, 4, 5],
      other=[("rows beyond an int", [(3, BIG[0]), (5, BIG[1])], ELIMIT),
             ("rows beyond an int, loss NULL", [(3, BIG[0]), (5, BIG[1]), (11, None)], EINVAL),
             ("more chunks than a grid has", [(3, 1), (4, 65536), (5, 8192)], ELIMIT),
             ("two of the three row arrays", [(8, None), (9, None)], EINVAL)])
entry("icnn_be_gd_eval_work_bytes", lambda: [8], zero=[0], bad=[(0, -1)], expect=0)
entry("icnn_be_gd_eval", lambda: [P(1), P(2), 8, 5, P(3), P(4), P(5), None], null=[0, 1, 4, 6], zero=[2, 3])
entry("icnn_be_macro_f1", lambda: [P(1), 8, P(2), None], null=[0, 2], zero=[1])
entry("icnn_be_keep_best", lambda: [P(1), 0, 0, P(2), P(3), None], null=[0, 3, 4], bad=[(2, 2), (2, -1)])
entry("icnn_be_entropy_objective", lambda: [P(1), P(2), 8, 5, P(3), None], null=[0, 1, 4], zero=[3], bad=[(2, -1)],
      other=[("empty batch", [(2, 0)], 0)])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refusals(name):
    make, cases = ENTRIES[name]
    fn = getattr(_lib.load(), name)
    wrong = []
    for label, changes, expect in cases:
        args = make()
        for path, value in changes:
            put(args, path, get(args, path) + 4 if value == "+4" else value)
        got = fn(*args)
        if got != expect:
            wrong.append("%s: %d, expected %d" % (label, got, expect))
    assert not wrong, "%s:\n  %s" % (name, "\n  ".join(wrong))


def test_debug_dual_step_body_refusals():
    """icnn_be_debug_dual_step_body (be_api.hip; it takes a state, so it is not one of ENTRIES): what it refuses before any
    launch, next to the nearest call it accepts.  Every state here has batch 0, where an accepted call returns 0 and launches
    nothing either."""
    fn = _lib.load().icnn_be_debug_dual_step_body
    MFMA, GLB, SLICE = _lib.FLAG_MFMA_CONTRACTION, _lib.FLAG_GLOBAL_BUNDLE, _lib.FLAG_TIME_SLICE

    def call(t=3, which=1, rows_mode=0, f=P(40), g=P(41), st="state", **kw):
        s = fill(_lib.State, **dict(dict(batch=0, n=159, slots=10, cut_dtype=_lib.CUT_F32, variant=_lib.VARIANT["dual"], flags=0, iters=0), **kw))
        return fn(C.byref(s) if st == "state" else st, t, f, g, which, rows_mode, None)

    accepted = [dict(), dict(which=2), dict(rows_mode=1), dict(t=0), dict(t=9), dict(which=2, t=7), dict(which=1, flags=MFMA),
                dict(slots=15), dict(which=2, slots=15), dict(which=3, slots=16), dict(which=3, slots=31, t=30, rows_mode=1),
                dict(which=3, slots=16, flags=MFMA), dict(slots=10, iters=24, t=20), dict(which=2, slots=5, t=4),
                dict(flags=_lib.FLAG_F64_ENERGY)]
    refused = [dict(st=None), dict(f=None), dict(g=None), dict(t=-1), dict(t=10), dict(slots=10, iters=24, t=24),
               dict(variant=_lib.VARIANT["rl"]), dict(variant=_lib.VARIANT["pdipm"]), dict(cut_dtype=_lib.CUT_F64),
               dict(n=158), dict(n=160), dict(n=48),
               dict(which=0), dict(which=4), dict(which=-1), dict(rows_mode=-1), dict(rows_mode=2), dict(which=2, rows_mode=1),
               dict(which=3), dict(which=3, slots=15), dict(which=1, slots=16), dict(which=2, slots=16),
               dict(which=2, t=8), dict(which=2, t=9), dict(which=2, slots=10, iters=24, t=8), dict(which=2, flags=MFMA),
               dict(flags=GLB), dict(which=3, slots=31, flags=GLB), dict(flags=SLICE), dict(which=2, flags=SLICE)]
    refused += [{name: None} for name in pointers(_lib.State, skip=("scratch", "fvals"))]
    wrong = ["accepted case %r: %d" % (kw, call(**kw)) for kw in accepted if call(**kw) != 0]
    wrong += ["refused case %r: %d" % (kw, call(**kw)) for kw in refused if call(**kw) != EINVAL]
    if call(slots=_lib.MAX_SLOTS + 1, which=3) != ELIMIT:
        wrong.append("more slots than ICNN_BE_MAX_SLOTS")
    assert not wrong, "\n  ".join(wrong)


def test_every_moved_entry_is_covered():
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    assert len(ENTRIES) == 61
