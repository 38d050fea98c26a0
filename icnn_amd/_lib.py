"""ctypes binding of libicnn_be.so -- the C ABI declared in include/icnn_be.h, read from that header (_header.py).

There is no CPU fallback: if the HIP library cannot be loaded the import of the
solver fails loudly.  Build it with `python -m icnn_amd.build` (or
`__graft_entry__.build()`).
"""
import ctypes as C
import os

# torch first: its wheel carries its own HIP runtime (torch/lib/libamdhip64.so), and the process must end up with
# ONE runtime.  Loaded after torch, libicnn_be.so binds to the copy torch already mapped (same SONAME); loaded
# before, it maps /opt/rocm's copy and the second runtime to initialise finds "no ROCm-capable device".
import torch  # noqa: F401

from . import _header

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libicnn_be.so")
if os.environ.get("ICNN_BE_LIB"):          # diagnostic: another build of the same ABI (tools/lib_ab.py: same-box A/B of two builds)
    LIB_PATH = os.path.abspath(os.environ["ICNN_BE_LIB"])

_H = _header.read()
PROTOTYPES = _H.prototypes                 # C name -> _header.Prototype (restype, argtypes, the parameters as declared)
EXPORTS = list(PROTOTYPES)

# Every ICNN_BE_<NAME> of the header is this module's <NAME>: ABI_VERSION, MAX_*, CUT_*, ST_*, FLAG_*, CLAMP_*, RL_TD_*,
# REPLAY_*, DATASET_*, LOG_*, DDPG_* / NAF_* / NAF_BN_* / FF_* / FCN_* limits, ...
K = {name[len("ICNN_BE_"):]: value for name, value in _H.constants.items()}
globals().update(K)
ST_ERROR_MASK = K["ST_SINGULAR"] | K["ST_NONFINITE"] | K["ST_UNFINISHED"] | K["ST_OVERFLOW"]      # what stops a training step (icnn_be_step_gate)
ERRORS = {K["EINVAL"]: "ICNN_BE_EINVAL (bad argument)", K["ELIMIT"]: "ICNN_BE_ELIMIT (size beyond a compiled-in limit)",
          K["ELAUNCH"]: "ICNN_BE_ELAUNCH (HIP launch failed)"}


def _family(prefix, case=str.lower):
    """[(suffix, value)] of the constants ICNN_BE_<prefix>*, ordered by value"""
    return sorted(((case(name[len(prefix):]), value) for name, value in K.items() if name.startswith(prefix)), key=lambda kv: kv[1])


def _names(prefix, case=str.lower):
    """The suffixes of a family that counts 0, 1, 2, ...: a list the value indexes"""
    family = _family(prefix, case)
    if [value for _, value in family] != list(range(len(family))):
        raise ImportError("icnn_be.h: the constants ICNN_BE_%s* do not count from 0 upwards: %r" % (prefix, family))
    return [name for name, _ in family]


def _pieces(unit, suffixes="0123456789"):
    """The pieces of a unit's workspace (ICNN_BE_<unit>_W_*, ICNN_BE_<unit>_WORK_PIECES of them), in order.  A constant followed
    by a gap is the first of a run (`+ i` in the header): one name per member, told apart by `suffixes`."""
    family = _family(unit + "_W_")
    ends = [value for _, value in family[1:]] + [K[unit + "_WORK_PIECES"]]
    return [name + (suffixes[i] if end - value > 1 else "") for (name, value), end in zip(family, ends) for i in range(end - value)]


VARIANT = dict(_family("VARIANT_"))
SHAPE_INSTANCES = _names("SHAPE_")         # which instance of the persistent tile kernel a solve launches (icnn_be_debug_shape_instance)
PATHS = _names("PATH_", str.upper)         # how icnn_be_solve_fc runs a solve (icnn_be_debug_solve_plan)
ADAM_KERNELS = _names("ADAM_", str.upper)  # which kernel icnn_be_adam_fc launches (icnn_be_debug_adam_plan)
DUAL_KERNELS = _names("DUAL_PLAN_")        # which kernel icnn_be_dual_step launches (icnn_be_debug_dual_plan)
UNIT_KINDS = _names("UNIT_")               # the units of a tile evaluation's deal (icnn_be_debug_fc_deal)
FICNN_HEAD = dict(_family("FICNN_HEAD_"))
BN_MODE = dict(_family("BN_"))
KEEP_MODE = dict(_family("KEEP_"))
LOSS = {"xent": K["LOSS_XENT"], "mse": K["LOSS_MSE"]}
LOG_KIND = {"float32": K["LOG_F32"], "float64": K["LOG_F64"], "int32": K["LOG_I32"]}
DDPG_WORK = _pieces("DDPG")
NAF_WORK = _pieces("NAF")
NAF_BN_PASSES = ("l", "u", "v", "t")       # ICNN_BE_NAF_BN_PASSES of them: the three nets at obs, the target at ob2
NAF_BN_VARS = ["W1", "b1", "W2", "b2", "W3", "b3", "beta0", "beta1", "beta2"]     # ICNN_BE_NAF_BN_VARS of them
NAF_BN_WORK = _pieces("NAF_BN", "".join(NAF_BN_PASSES))     # a piece per pass carries the pass's letter
FF_WORK = _pieces("FF")                    # a / h / stat / dz of hidden layer i + 1 at "a%d" % i, ...
FCN_WORK = _pieces("FCN")                  # h<i> / dz<i>: output and delta of conv1..3, up1..3
if (len(NAF_BN_PASSES), len(NAF_BN_VARS)) != (K["NAF_BN_PASSES"], K["NAF_BN_VARS"]):
    raise ImportError("icnn_be.h: ICNN_BE_NAF_BN_PASSES / ICNN_BE_NAF_BN_VARS differ from the names _lib.py gives them")


def replay_stage_bytes(dimO, dimA):
    """ICNN_BE_REPLAY_STAGE_BYTES, the header's one function-like macro, by hand: action float64 [dimA], observation float32
    [dimO], reward float32, terminal uint32"""
    return 8 * dimA + 4 * dimO + 8


# C struct -> (the class's name here, its index in icnn_be_struct_size: the header states those in that entry's comment only)
STRUCTS = {
    "icnn_be_state": ("State", 0), "icnn_be_fc_model": ("FcModel", 1), "icnn_be_fc_ctx": ("FcCtx", 2),
    "icnn_be_conv_model": ("ConvModel", 3), "icnn_be_conv_ctx": ("ConvCtx", 4), "icnn_be_bn_moving": ("BnMoving", 5),
    "icnn_be_param_update_args": ("ParamUpdateArgs", 6), "icnn_be_rl_update_args": ("RlUpdateArgs", 7),
    "icnn_be_ficnn_model": ("FicnnModel", 8), "icnn_be_replay": ("Replay", 9), "icnn_be_dataset": ("Dataset", 10),
    "icnn_be_step_log": ("StepLog", 11), "icnn_be_ddpg_args": ("DdpgArgs", 13), "icnn_be_naf_args": ("NafArgs", 14),
    "icnn_be_ff_args": ("FfArgs", 16), "icnn_be_fcn_args": ("FcnArgs", 18), "icnn_be_naf_bn_args": ("NafBnArgs", 20),
    "icnn_be_vec_replay": ("VecReplay", 22),
}
if set(STRUCTS) != set(_H.structs):
    raise ImportError("icnn_be.h and _lib.STRUCTS name different structs: %s" % sorted(set(STRUCTS) ^ set(_H.structs)))
for _c_name, (_py_name, _) in STRUCTS.items():
    _H.structs[_c_name].__name__ = _H.structs[_c_name].__qualname__ = _py_name
    globals()[_py_name] = _H.structs[_c_name]

_lib = None


def use_profiling_build():
    """Make load() take the PROFILING variant of the library (csrc/prof/libicnn_be.so: the same sources with the cycle-counter
    laps behind icnn_be_debug_profile* compiled in, `python -m icnn_amd.build --prof`), building it when missing or stale.
    The production library is built without the laps -- there the hooks set a pointer nothing reads.  Diagnostic tools call
    this before anything loads the library (tools/*_phase_profile.py)."""
    global LIB_PATH
    from . import build as _build
    if _lib is not None and LIB_PATH != _build.PROF_LIB:
        raise RuntimeError("the production library is already loaded in this process")
    LIB_PATH = _build.build(prof=True)
    return LIB_PATH


def declare(lib, names=None):
    """Give the entries of a CDLL handle of the library the header's argtypes and restype: all of them, or those in `names`.
    An entry the handle lacks is an ImportError: a build older than the header (ABI 12 only grows)."""
    for name in EXPORTS if names is None else names:
        fn = getattr(lib, name, None)
        if fn is None:
            raise ImportError("%s has no symbol %s that include/icnn_be.h declares: a stale build; rebuild with "
                              "python -m icnn_amd.build" % (getattr(lib, "_name", "the library"), name))
        fn.argtypes, fn.restype = PROTOTYPES[name].argtypes, PROTOTYPES[name].restype
    return lib


def load():
    """Load the shared library (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: the HIP extension has not been built.  Run `python -m icnn_amd.build` "
            "(needs hipcc; there is no CPU fallback for the bundle-entropy kernels)." % LIB_PATH)
    lib = declare(C.CDLL(LIB_PATH))
    for c_name, (_, which) in STRUCTS.items():
        if lib.icnn_be_struct_size(which) != C.sizeof(_H.structs[c_name]):
            raise ImportError("ctypes struct layout of %s differs from libicnn_be.so's (%d bytes here, %d there); rebuild with "
                              "python -m icnn_amd.build" % (c_name, C.sizeof(_H.structs[c_name]), lib.icnn_be_struct_size(which)))
    if lib.icnn_be_abi_version() != K["ABI_VERSION"]:
        raise ImportError("libicnn_be.so ABI %d != binding ABI %d; rebuild with python -m icnn_amd.build"
                          % (lib.icnn_be_abi_version(), K["ABI_VERSION"]))
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    msg = ERRORS.get(rc, "error %d" % rc)
    if rc == K["ELAUNCH"]:
        msg += ": " + load().icnn_be_last_hip_error().decode()
    raise RuntimeError("%s failed: %s" % (what, msg))


def solve_plan(model, state, cus=0):
    """(path name, samples per workgroup, Newton budget per round, value icnn_be_solve_fc returns) for an FcModel and a State
    (icnn_be_debug_solve_plan; cus < 1: the current device's CU count).  Host arithmetic: no GPU, no buffers needed."""
    out = (C.c_int * 3)()
    rc = load().icnn_be_debug_solve_plan(C.byref(model), C.byref(state), cus, C.byref(out))
    if rc < 0:
        check(rc, "icnn_be_debug_solve_plan")
    return (PATHS[rc],) + tuple(out)


def shape_instance(model, state):
    """Name (SHAPE_INSTANCES) of the persistent tile kernel's instance icnn_be_solve_fc launches for an FcModel and a State:
    'generic', or the instance compiled for that network's shape (icnn_be_debug_shape_instance).  Host arithmetic."""
    rc = load().icnn_be_debug_shape_instance(C.byref(model), C.byref(state))
    if rc < 0:
        check(rc, "icnn_be_debug_shape_instance")
    return SHAPE_INSTANCES[rc]


def fc_deal(model):
    """The deal of one tile evaluation of an FcModel (icnn_be_debug_fc_deal): a list of (kind, layer, tile, interval, wave,
    interval of the result), kind one of UNIT_KINDS.  Host arithmetic."""
    lib = load()
    count = lib.icnn_be_debug_fc_deal(C.byref(model), None, 0)
    if count < 0:
        check(count, "icnn_be_debug_fc_deal")
    out = (C.c_int * (6 * count))()
    lib.icnn_be_debug_fc_deal(C.byref(model), out, count)
    return [(UNIT_KINDS[out[6 * k]],) + tuple(out[6 * k + 1:6 * k + 6]) for k in range(count)]


def adam_plan(model, batch, ctx=None):
    """(kernel name, states per workgroup, workgroups, cooperative, obs form accepted) of icnn_be_adam_fc for an FcModel and
    a batch on the current device (icnn_be_debug_adam_plan); `ctx`: the FcCtx icnn_be_adam_fc_obs would get, for the last
    entry (False without one).  Enqueues nothing; asks the runtime for the kernels' occupancy, so it needs a device."""
    out = (C.c_int * 4)()
    rc = load().icnn_be_debug_adam_plan(C.byref(model), C.byref(ctx) if ctx is not None else None, int(batch), C.byref(out))
    if rc < 0:
        check(rc, "icnn_be_debug_adam_plan")
    return (ADAM_KERNELS[rc], out[0], out[1], bool(out[2]), bool(out[3]))


def adam_each_plan(model, batch):
    """(kernel name, states per workgroup, workgroups) of icnn_be_adam_fc_each for an FcModel and a batch on the current
    device (icnn_be_debug_adam_each_plan): the per-state stopping rule, one ordinary launch, no residency limit."""
    out = (C.c_int * 2)()
    rc = load().icnn_be_debug_adam_each_plan(C.byref(model), int(batch), C.byref(out))
    if rc < 0:
        check(rc, "icnn_be_debug_adam_each_plan")
    return (ADAM_KERNELS[rc], out[0], out[1])


def dual_plan(state, t):
    """(cut type 'float' | 'double', KT or KS, waves per workgroup, variant name, bundle staged in scratch, 'small' | 'body' |
    'wide', LDS bytes, staged rows) of the launch icnn_be_dual_step(state, t, ...) makes (icnn_be_debug_dual_plan).  Host
    arithmetic on the State's shape fields, flags and on whether `scratch` is set: no GPU, no buffers needed."""
    out = (C.c_int * 8)()
    rc = load().icnn_be_debug_dual_plan(C.byref(state), int(t), C.byref(out))
    if rc < 0:
        check(rc, "icnn_be_debug_dual_plan")
    variant = [name for name, code in VARIANT.items() if code == out[3]][0]
    return ("double" if out[0] == K["CUT_F64"] else "float", out[1], out[2], variant, bool(out[4]), DUAL_KERNELS[out[5]], out[6], out[7])
