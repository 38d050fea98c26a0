"""ctypes binding of libicnn_be.so -- the C ABI declared in include/icnn_be.h.

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

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libicnn_be.so")
if os.environ.get("ICNN_BE_LIB"):          # diagnostic: another build of the same ABI (tools/lib_ab.py: same-box A/B of two builds)
    LIB_PATH = os.path.abspath(os.environ["ICNN_BE_LIB"])

ABI_VERSION = 12
MAX_LAYERS = 8
MAX_SLOTS = 31
MAX_ITERS = 64
MAX_ROUNDS = 128
VARIANT = {"dual": 0, "rl": 1, "pdipm": 2}
CUT_F32, CUT_F64 = 0, 1
ST_SINGULAR, ST_NONFINITE, ST_OVERFLOW, ST_UNFINISHED = 1, 2, 4, 8
ST_ERROR_MASK = ST_SINGULAR | ST_NONFINITE | ST_UNFINISHED | ST_OVERFLOW      # what stops a training step (icnn_be_step_gate)
FLAG_NO_CYCLE_SHORTCUT = 1
FLAG_TIME_SLICE = 2
FLAG_LOCKSTEP = 4
FLAG_TWO_KERNELS = 8
FLAG_PERSISTENT = 16
FLAG_F64_ENERGY = 32
FLAG_GLOBAL_BUNDLE = 64
FLAG_WAVE_PER_SAMPLE = 128
FLAG_MFMA_CONTRACTION = 256
FLAG_GENERIC_SHAPE = 512
FLAG_NO_ROUND_CLASSES = 1024
# ICNN_BE_SHAPE_*: which instance of the persistent tile kernel a solve launches (icnn_be_debug_shape_instance)
SHAPE_INSTANCES = ["generic", "bibtex_kt16", "bibtex_kt32_grouped"]
LOSS = {"xent": 0, "mse": 1}
# ICNN_BE_PATH_*: how icnn_be_solve_fc runs a solve (icnn_be_debug_solve_plan)
PATHS = ["ROWS", "TILE", "TILE_BUDGETED_THEN_ROWS", "ROUNDS_LOCKSTEP", "ROUNDS_SLICED_THEN_ROWS", "ROUNDS_SLICED_EXTRA"]
# ICNN_BE_ADAM_*: which kernel icnn_be_adam_fc launches (icnn_be_debug_adam_plan)
ADAM_KERNELS = ["NONE", "ROWS", "TILE"]
# ICNN_BE_DUAL_PLAN_*: which kernel icnn_be_dual_step launches (icnn_be_debug_dual_plan)
DUAL_KERNELS = ["small", "body", "wide"]
ERRORS = {-1: "ICNN_BE_EINVAL (bad argument)", -2: "ICNN_BE_ELIMIT (size beyond a compiled-in limit)",
          -3: "ICNN_BE_ELAUNCH (HIP launch failed)"}

EXPORTS = [
    "icnn_be_abi_version", "icnn_be_last_hip_error", "icnn_be_struct_size", "icnn_be_dual_lds_bytes", "icnn_be_bundle_capacity", "icnn_be_scratch_bytes",
    "icnn_be_state_init",
    "icnn_be_dual_step", "icnn_be_fc_pack_floats", "icnn_be_fc_pack", "icnn_be_fc_fg",
    "icnn_be_solve_fc", "icnn_be_solve_fc_reset", "icnn_be_conv_pack_floats", "icnn_be_conv_work_floats", "icnn_be_conv_pack", "icnn_be_conv_fg", "icnn_be_solve_conv",
    "icnn_be_implicit_feed", "icnn_be_export_active", "icnn_be_adam_workspace_bytes", "icnn_be_adam_fc", "icnn_be_adam_fc_obs",
    "icnn_be_adam_fc_each", "icnn_be_debug_adam_each_plan",
    "icnn_be_fc_context_work_floats", "icnn_be_fc_context", "icnn_be_fc_context_stage", "icnn_be_fc_context_norm", "icnn_be_fc_clamp",
    "icnn_be_conv_context_work_floats", "icnn_be_conv_context", "icnn_be_conv_clamp",
    "icnn_be_debug_profile", "icnn_be_debug_profile_fc", "icnn_be_debug_profile_conv", "icnn_be_debug_profile_phases",
    "icnn_be_debug_fast_math", "icnn_be_debug_trace", "icnn_be_debug_solve_plan", "icnn_be_debug_adam_plan", "icnn_be_debug_dual_plan",
    "icnn_be_debug_dual_step_body",
    "icnn_be_debug_shape_instance", "icnn_be_debug_fc_deal",
    "icnn_be_fc_grad_floats", "icnn_be_fc_surrogate_grad_work_floats", "icnn_be_fc_surrogate_grad",
    "icnn_be_conv_grad_floats", "icnn_be_conv_surrogate_grad_work_floats", "icnn_be_conv_surrogate_grad",
    "icnn_be_fc_context_bn_work_floats", "icnn_be_fc_context_bn", "icnn_be_conv_context_bn_work_floats", "icnn_be_conv_context_bn",
    "icnn_be_fc_surrogate_grad_bn", "icnn_be_conv_surrogate_grad_bn", "icnn_be_param_update",
    "icnn_be_gd_workspace_bytes", "icnn_be_fc_gd", "icnn_be_conv_gd",
    "icnn_be_rl_td", "icnn_be_rl_critic_update", "icnn_be_rl_bundle_solve",
    "icnn_be_ficnn_pack_floats", "icnn_be_ficnn_pack", "icnn_be_ficnn_context_work_floats", "icnn_be_ficnn_context",
    "icnn_be_ficnn_fg", "icnn_be_ficnn_gd", "icnn_be_solve_ficnn", "icnn_be_ficnn_grad_floats",
    "icnn_be_ficnn_surrogate_grad_work_floats", "icnn_be_ficnn_surrogate_grad",
    "icnn_be_feed_plan_work_bytes", "icnn_be_feed_plan", "icnn_be_feed_pad", "icnn_be_fc_surrogate_grad_dev",
    "icnn_be_conv_surrogate_grad_dev", "icnn_be_fc_context_bn_dev", "icnn_be_conv_context_bn_dev",
    "icnn_be_fc_surrogate_grad_dev_work_floats", "icnn_be_conv_surrogate_grad_dev_work_floats",
    "icnn_be_gd_feed_work_bytes", "icnn_be_gd_feed", "icnn_be_gd_feed_px_work_bytes", "icnn_be_gd_feed_px",
    "icnn_be_step_gate", "icnn_be_param_update_gated", "icnn_be_gated_copy",
    "icnn_be_replay_enqueue", "icnn_be_replay_sample",
    "icnn_be_vec_replay_enqueue", "icnn_be_vec_replay_sample", "icnn_be_explore",
    "icnn_be_gd_eval_work_bytes", "icnn_be_gd_eval", "icnn_be_macro_f1", "icnn_be_keep_best",
    "icnn_be_dataset_draw", "icnn_be_log_row",
    "icnn_be_ddpg_param_floats", "icnn_be_ddpg_work_bytes", "icnn_be_ddpg_work_offsets", "icnn_be_ddpg_chain", "icnn_be_ddpg_grads",
    "icnn_be_ddpg_update", "icnn_be_ddpg_step", "icnn_be_ddpg_act", "icnn_be_ddpg_q",
    "icnn_be_naf_param_floats", "icnn_be_naf_work_bytes", "icnn_be_naf_work_offsets", "icnn_be_naf_chain", "icnn_be_naf_grads",
    "icnn_be_naf_update", "icnn_be_naf_step", "icnn_be_naf_act", "icnn_be_naf_q",
    "icnn_be_ff_param_floats", "icnn_be_ff_work_bytes", "icnn_be_ff_work_offsets", "icnn_be_ff_forward", "icnn_be_ff_backward",
    "icnn_be_ff_grads", "icnn_be_ff_update", "icnn_be_ff_step", "icnn_be_ff_eval",
    "icnn_be_fcn_param_floats", "icnn_be_fcn_work_bytes", "icnn_be_fcn_work_offsets", "icnn_be_fcn_forward", "icnn_be_fcn_backward",
    "icnn_be_fcn_grads", "icnn_be_fcn_update", "icnn_be_fcn_step", "icnn_be_fcn_eval",
    "icnn_be_naf_bn_param_floats", "icnn_be_naf_bn_layout", "icnn_be_naf_bn_work_bytes", "icnn_be_naf_bn_work_offsets",
    "icnn_be_naf_bn_chain", "icnn_be_naf_bn_grads", "icnn_be_naf_bn_update", "icnn_be_naf_bn_step", "icnn_be_naf_bn_act",
    "icnn_be_naf_bn_q",
    "icnn_be_pgd_workspace_bytes", "icnn_be_fc_pgd", "icnn_be_conv_pgd", "icnn_be_entropy_objective", "icnn_be_bundle_trace",
    "icnn_be_dual_bound",
]
FICNN_HEAD = {"sum": 0, "linear": 1}     # ICNN_BE_FICNN_HEAD_*
CLAMP_ABS, CLAMP_RELU, CLAMP_ABS_HALF = 0, 1, 2
BN_MODE = {"batch": 0, "moving": 1}     # ICNN_BE_BN_BATCH / ICNN_BE_BN_MOVING
KEEP_MODE = {"min": 0, "max": 1}        # ICNN_BE_KEEP_MIN / ICNN_BE_KEEP_MAX
MAX_PROJ_RANGES = 8
RL_TD_MAX_BLOCKS = 256
RL_TD_WORK_BYTES = 8 * RL_TD_MAX_BLOCKS + 16
REPLAY_CTRL_INTS = 8                       # ICNN_BE_REPLAY_CTRL_INTS: cursor, fill, draws, status, ticket
REPLAY_MAX_ATTEMPTS = 256
REPLAY_ST_EXHAUSTED, REPLAY_ST_STATE = 1, 2
DATASET_MAX_ARRAYS = 4                     # ICNN_BE_DATASET_MAX_ARRAYS
DATASET_CTRL_INTS = 8                      # ICNN_BE_DATASET_CTRL_INTS: draws, status, ticket
DATASET_ST_STATE = 1
LOG_MAX_COLUMNS = 8                        # ICNN_BE_LOG_MAX_COLUMNS
LOG_CTRL_INTS = 4                          # ICNN_BE_LOG_CTRL_INTS: the cursor
LOG_KIND = {"float32": 0, "float64": 1, "int32": 2}     # ICNN_BE_LOG_F32 / _F64 / _I32
DDPG_MAX_OBS, DDPG_MAX_ACT, DDPG_MAX_HIDDEN = 600, 32, 600     # ICNN_BE_DDPG_MAX_*
DDPG_STEP_INTS = 4                         # ICNN_BE_DDPG_STEP_INTS: updates of the critic, of the policy, the ticket
# ICNN_BE_DDPG_W_*: the pieces of the DDPG workspace, in order
DDPG_WORK = ["a2", "y", "q", "td", "a", "qpi", "xa", "h2q", "d3q", "d2q", "d1q", "h1p", "h2p", "h2c", "d3p", "d2p", "d1p", "sq",
             "upd"]
NAF_MAX_OBS, NAF_MAX_ACT, NAF_MAX_HIDDEN = 600, 32, 600        # ICNN_BE_NAF_MAX_*
NAF_STEP_INTS = 4                          # ICNN_BE_NAF_STEP_INTS: the updates, the ticket
# ICNN_BE_NAF_W_*: the pieces of the NAF workspace, in order
NAF_WORK = ["y", "u", "l", "ld", "h", "adv", "q", "td", "h1l", "h2l", "h1u", "h2u", "h1v", "h2v", "d3l", "d2l", "d1l", "d3u", "d2u",
            "d1u", "d3v", "d2v", "d1v", "sq", "upd"]
NAF_BN_MAX_BATCH = 512                     # ICNN_BE_NAF_BN_MAX_BATCH
NAF_BN_PASSES = ("l", "u", "v", "t")       # ICNN_BE_NAF_BN_PASSES: the three nets at obs, the target at ob2
NAF_BN_VARS = ["W1", "b1", "W2", "b2", "W3", "b3", "beta0", "beta1", "beta2"]     # ICNN_BE_NAF_BN_VARS
# ICNN_BE_NAF_BN_W_*: the pieces of the NAF-BN workspace, in order; a piece per pass carries the pass's letter
NAF_BN_WORK = (["y", "u", "l", "ld", "h", "adv", "q", "td"] + ["d3" + p for p in "luv"]
               + [k + p for k in ("h0", "h1", "h2", "xh1", "xh2") for p in "luvt"]
               + [k + p for k in ("d1", "d2") for p in "luv"] + ["stat" + p for p in "luvt"] + ["sq", "upd"])
FF_MAX_LAYERS, FF_MAX_FEATURES, FF_MAX_WIDTH, FF_MAX_BATCH = 4, 4096, 1024, 512     # ICNN_BE_FF_MAX_*
FF_STEP_INTS = 4                           # ICNN_BE_FF_STEP_INTS: the updates, the ticket
# ICNN_BE_FF_W_*: the pieces of the feed-forward workspace, in order; a / h / stat / dz of hidden layer i + 1 at "a%d" % i, ...
FF_WORK = (["a%d" % i for i in range(4)] + ["h%d" % i for i in range(4)] + ["stat%d" % i for i in range(4)]
           + ["dz%d" % i for i in range(4)] + ["dlogit", "part", "ctl"])
FCN_MAX_K, FCN_MAX_HW, FCN_MAX_BATCH, FCN_MAX_EVAL_BATCH = 64, 128, 128, 65536     # ICNN_BE_FCN_MAX_*
FCN_STEP_INTS = 4                          # ICNN_BE_FCN_STEP_INTS: the updates, the ticket
# ICNN_BE_FCN_W_*: the pieces of the FCN workspace, in order; h<i> / dz<i>: output and delta of conv1..3, up1..3
FCN_WORK = ["h%d" % i for i in range(6)] + ["dy"] + ["dz%d" % i for i in range(6)] + ["wpart", "lpart", "ctl"]


def replay_stage_bytes(dimO, dimA):
    """ICNN_BE_REPLAY_STAGE_BYTES: action float64 [dimA], observation float32 [dimO], reward float32, terminal uint32"""
    return 8 * dimA + 4 * dimO + 8


class State(C.Structure):
    """struct icnn_be_state"""
    _fields_ = [
        ("batch", C.c_int), ("n", C.c_int), ("slots", C.c_int), ("cut_dtype", C.c_int),
        ("variant", C.c_int), ("flags", C.c_int),
        ("y", C.c_void_p), ("G", C.c_void_p), ("h", C.c_void_p), ("ys", C.c_void_p),
        ("lam", C.c_void_p), ("active", C.c_void_p), ("count", C.c_void_p),
        ("n_iters", C.c_void_p), ("finished", C.c_void_p), ("status", C.c_void_p),
        ("newton_iters", C.c_void_p),
        ("t_next", C.c_void_p), ("phase", C.c_void_p), ("skip_fg", C.c_void_p), ("pending", C.c_void_p),
        ("park", C.c_void_p), ("scratch", C.c_void_p), ("fvals", C.c_void_p), ("iters", C.c_int),
    ]


class FcModel(C.Structure):
    """struct icnn_be_fc_model"""
    _fields_ = [
        ("n", C.c_int), ("n_layers", C.c_int), ("width", C.c_int * MAX_LAYERS),
        ("alpha", C.c_float), ("action_box", C.c_int), ("ctx_width", C.c_int),
        ("wpack", C.c_void_p),
    ]


class FcCtx(C.Structure):
    """struct icnn_be_fc_ctx"""
    _fields_ = [
        ("n_features", C.c_int), ("n", C.c_int), ("n_layers", C.c_int), ("width", C.c_int * MAX_LAYERS),
        ("batchnorm", C.c_int), ("bn_eps", C.c_float), ("u_last_relu", C.c_int),
        ("w_stage", C.c_void_p * MAX_LAYERS), ("b_stage", C.c_void_p * MAX_LAYERS),
        ("bn_gamma", C.c_void_p * MAX_LAYERS), ("bn_beta", C.c_void_p * MAX_LAYERS),
    ]


class FicnnModel(C.Structure):
    """struct icnn_be_ficnn_model"""
    _fields_ = [
        ("n_features", C.c_int), ("n", C.c_int), ("n_layers", C.c_int), ("width", C.c_int * MAX_LAYERS),
        ("head", C.c_int), ("ctx_width", C.c_int), ("wpack", C.c_void_p),
    ]


class ConvModel(C.Structure):
    """struct icnn_be_conv_model"""
    _fields_ = [
        ("H", C.c_int), ("W", C.c_int), ("filters", C.c_int * 3), ("ksize", C.c_int * 3),
        ("stride", C.c_int * 3), ("fc_hidden", C.c_int), ("ctx_width", C.c_int), ("wpack", C.c_void_p),
        ("work", C.c_void_p), ("work_batch", C.c_int),
    ]


class ConvCtx(C.Structure):
    """struct icnn_be_conv_ctx"""
    _fields_ = [
        ("w_stage", C.c_void_p * 7), ("b_stage", C.c_void_p * 7), ("bn_gamma", C.c_void_p * 4), ("bn_beta", C.c_void_p * 4),
        ("bn_eps", C.c_float),
    ]


class BnMoving(C.Structure):
    """struct icnn_be_bn_moving"""
    _fields_ = [("mean", C.c_void_p * MAX_LAYERS), ("var", C.c_void_p * MAX_LAYERS), ("decay", C.c_float)]


class ParamUpdateArgs(C.Structure):
    """struct icnn_be_param_update_args"""
    _fields_ = [
        ("n", C.c_longlong), ("theta", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("grad", C.c_void_p),
        ("dest_off", C.c_void_p), ("dest", C.c_void_p), ("arena", C.c_void_p), ("arena_floats", C.c_longlong),
        ("step", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_float),
        ("n_proj", C.c_int), ("proj_begin", C.c_longlong * MAX_PROJ_RANGES), ("proj_end", C.c_longlong * MAX_PROJ_RANGES),
    ]


class RlUpdateArgs(C.Structure):
    """struct icnn_be_rl_update_args"""
    _fields_ = [
        ("adam", ParamUpdateArgs), ("target_theta", C.c_void_p), ("target_arena", C.c_void_p), ("decay", C.c_void_p),
        ("tau", C.c_float), ("l2norm", C.c_float), ("wd", C.c_float),
    ]


class Replay(C.Structure):
    """struct icnn_be_replay"""
    _fields_ = [
        ("size", C.c_int), ("dimO", C.c_int), ("dimA", C.c_int), ("observations", C.c_void_p), ("actions", C.c_void_p),
        ("rewards", C.c_void_p), ("terminals", C.c_void_p), ("ctrl", C.c_void_p),
    ]


class VecReplay(C.Structure):
    """struct icnn_be_vec_replay"""
    _fields_ = [
        ("steps", C.c_int), ("n_envs", C.c_int), ("dimO", C.c_int), ("dimA", C.c_int), ("observations", C.c_void_p),
        ("actions", C.c_void_p), ("rewards", C.c_void_p), ("terminals", C.c_void_p), ("ctrl", C.c_void_p),
    ]


class Dataset(C.Structure):
    """struct icnn_be_dataset"""
    _fields_ = [
        ("n_rows", C.c_int), ("n_arrays", C.c_int), ("src", C.c_void_p * DATASET_MAX_ARRAYS),
        ("row_words", C.c_int * DATASET_MAX_ARRAYS), ("ctrl", C.c_void_p),
    ]


class StepLog(C.Structure):
    """struct icnn_be_step_log"""
    _fields_ = [
        ("rows", C.c_void_p), ("ctrl", C.c_void_p), ("cap", C.c_int), ("width", C.c_int),
        ("col", C.c_void_p * LOG_MAX_COLUMNS), ("kind", C.c_int * LOG_MAX_COLUMNS),
    ]


class DdpgArgs(C.Structure):
    """struct icnn_be_ddpg_args"""
    _fields_ = [
        ("batch", C.c_int), ("dimO", C.c_int), ("dimA", C.c_int), ("l1", C.c_int), ("l2", C.c_int),
        ("obs", C.c_void_p), ("act", C.c_void_p), ("rew", C.c_void_p), ("ob2", C.c_void_p), ("term", C.c_void_p),
        ("theta_q", C.c_void_p), ("theta_p", C.c_void_p), ("target_q", C.c_void_p), ("target_p", C.c_void_p),
        ("m_q", C.c_void_p), ("v_q", C.c_void_p), ("m_p", C.c_void_p), ("v_p", C.c_void_p),
        ("grad_q", C.c_void_p), ("grad_p", C.c_void_p), ("step", C.c_void_p), ("loss", C.c_void_p), ("work", C.c_void_p),
        ("rate", C.c_double), ("prate", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_float), ("tau", C.c_float), ("discount", C.c_float), ("l2norm", C.c_float), ("pl2norm", C.c_float),
    ]


class NafArgs(C.Structure):
    """struct icnn_be_naf_args"""
    _fields_ = [
        ("batch", C.c_int), ("dimO", C.c_int), ("dimA", C.c_int), ("l1", C.c_int), ("l2", C.c_int),
        ("obs", C.c_void_p), ("act", C.c_void_p), ("rew", C.c_void_p), ("ob2", C.c_void_p), ("term", C.c_void_p),
        ("theta_l", C.c_void_p), ("theta_u", C.c_void_p), ("theta_v", C.c_void_p), ("target_v", C.c_void_p),
        ("m_l", C.c_void_p), ("v_l", C.c_void_p), ("m_u", C.c_void_p), ("v_u", C.c_void_p), ("m_v", C.c_void_p), ("v_v", C.c_void_p),
        ("grad_l", C.c_void_p), ("grad_u", C.c_void_p), ("grad_v", C.c_void_p),
        ("step", C.c_void_p), ("loss", C.c_void_p), ("work", C.c_void_p),
        ("rate", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_float), ("tau", C.c_float), ("discount", C.c_float), ("l2norm", C.c_float),
    ]


class NafBnArgs(C.Structure):
    """struct icnn_be_naf_bn_args"""
    _fields_ = [
        ("batch", C.c_int), ("dimO", C.c_int), ("dimA", C.c_int), ("l1", C.c_int), ("l2", C.c_int),
        ("obs", C.c_void_p), ("act", C.c_void_p), ("rew", C.c_void_p), ("ob2", C.c_void_p), ("term", C.c_void_p),
        ("theta_l", C.c_void_p), ("theta_u", C.c_void_p), ("theta_v", C.c_void_p), ("target_v", C.c_void_p),
        ("m_l", C.c_void_p), ("v_l", C.c_void_p), ("m_u", C.c_void_p), ("v_u", C.c_void_p), ("m_v", C.c_void_p), ("v_v", C.c_void_p),
        ("grad_l", C.c_void_p), ("grad_u", C.c_void_p), ("grad_v", C.c_void_p),
        ("mv_l", C.c_void_p), ("mv_u", C.c_void_p), ("mv_v", C.c_void_p),
        ("step", C.c_void_p), ("loss", C.c_void_p), ("work", C.c_void_p),
        ("rate", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("bn_decay", C.c_double),
        ("eps", C.c_float), ("tau", C.c_float), ("discount", C.c_float), ("l2norm", C.c_float), ("bn_eps", C.c_float),
    ]


class FfArgs(C.Structure):
    """struct icnn_be_ff_args"""
    _fields_ = [
        ("batch", C.c_int), ("n_features", C.c_int), ("n_labels", C.c_int), ("n_layers", C.c_int),
        ("width", C.c_int * FF_MAX_LAYERS),
        ("x", C.c_void_p), ("true_y", C.c_void_p),
        ("theta", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("grad", C.c_void_p),
        ("mv", BnMoving),
        ("step", C.c_void_p), ("loss", C.c_void_p), ("yhat", C.c_void_p), ("f1_tallies", C.c_void_p), ("work", C.c_void_p),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_float), ("bn_eps", C.c_float),
    ]


class FcnArgs(C.Structure):
    """struct icnn_be_fcn_args"""
    _fields_ = [
        ("batch", C.c_int), ("H", C.c_int), ("W", C.c_int), ("k", C.c_int),
        ("x", C.c_void_p), ("t", C.c_void_p),
        ("theta", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("grad", C.c_void_p),
        ("step", C.c_void_p), ("loss", C.c_void_p), ("yhat", C.c_void_p), ("work", C.c_void_p),
        ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("eps", C.c_float), ("pixel_scale", C.c_float),
    ]


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


def load():
    """Load the shared library (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: the HIP extension has not been built.  Run `python -m icnn_amd.build` "
            "(needs hipcc; there is no CPU fallback for the bundle-entropy kernels)." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.icnn_be_abi_version.restype = C.c_int
    lib.icnn_be_last_hip_error.restype = C.c_char_p
    lib.icnn_be_dual_lds_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.icnn_be_dual_lds_bytes.restype = C.c_int
    lib.icnn_be_bundle_capacity.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.icnn_be_bundle_capacity.restype = C.c_int
    lib.icnn_be_scratch_bytes.argtypes = [C.POINTER(State)]
    lib.icnn_be_scratch_bytes.restype = C.c_size_t
    lib.icnn_be_state_init.argtypes = [C.POINTER(State), C.c_void_p]
    lib.icnn_be_state_init.restype = C.c_int
    lib.icnn_be_dual_step.argtypes = [C.POINTER(State), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_dual_step.restype = C.c_int
    lib.icnn_be_fc_pack_floats.argtypes = [C.POINTER(FcModel)]
    lib.icnn_be_fc_pack_floats.restype = C.c_size_t
    lib.icnn_be_fc_pack.argtypes = [C.POINTER(FcModel), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.c_void_p]
    lib.icnn_be_fc_pack.restype = C.c_int
    lib.icnn_be_fc_fg.argtypes = [C.POINTER(FcModel), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_fc_fg.restype = C.c_int
    lib.icnn_be_solve_fc.argtypes = [C.POINTER(FcModel), C.c_void_p, C.POINTER(State), C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    lib.icnn_be_solve_fc.restype = C.c_int
    lib.icnn_be_solve_fc_reset.argtypes = (lib.icnn_be_solve_fc.argtypes[:-1] + [C.c_void_p, C.c_double, C.c_void_p])
    lib.icnn_be_solve_fc_reset.restype = C.c_int
    lib.icnn_be_rl_bundle_solve.argtypes = (lib.icnn_be_solve_fc.argtypes[:-1] + [C.c_double, C.c_void_p, C.c_void_p, C.c_void_p])
    lib.icnn_be_rl_bundle_solve.restype = C.c_int
    lib.icnn_be_conv_pack_floats.argtypes = [C.POINTER(ConvModel)]
    lib.icnn_be_conv_pack_floats.restype = C.c_size_t
    lib.icnn_be_conv_work_floats.argtypes = [C.POINTER(ConvModel), C.c_int]
    lib.icnn_be_conv_work_floats.restype = C.c_size_t
    lib.icnn_be_conv_pack.argtypes = [C.POINTER(ConvModel)] + [C.POINTER(C.c_void_p)] * 4 + [C.c_void_p] * 3
    lib.icnn_be_conv_pack.restype = C.c_int
    lib.icnn_be_conv_fg.argtypes = [C.POINTER(ConvModel), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_conv_fg.restype = C.c_int
    lib.icnn_be_solve_conv.argtypes = [C.POINTER(ConvModel), C.c_void_p, C.POINTER(State), C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    lib.icnn_be_solve_conv.restype = C.c_int
    lib.icnn_be_implicit_feed.argtypes = [C.POINTER(State), C.c_void_p, C.c_int] + [C.c_void_p] * 6
    lib.icnn_be_implicit_feed.restype = C.c_int
    lib.icnn_be_export_active.argtypes = [C.POINTER(State)] + [C.c_void_p] * 6
    lib.icnn_be_export_active.restype = C.c_int
    lib.icnn_be_debug_fast_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.icnn_be_debug_fast_math.restype = C.c_int
    lib.icnn_be_debug_solve_plan.argtypes = [C.POINTER(FcModel), C.POINTER(State), C.c_int, C.POINTER(C.c_int * 3)]
    lib.icnn_be_debug_solve_plan.restype = C.c_int
    lib.icnn_be_debug_profile_phases.restype = C.c_int
    lib.icnn_be_debug_adam_plan.argtypes = [C.POINTER(FcModel), C.POINTER(FcCtx), C.c_int, C.POINTER(C.c_int * 4)]
    lib.icnn_be_debug_adam_plan.restype = C.c_int
    lib.icnn_be_debug_dual_plan.argtypes = [C.POINTER(State), C.c_int, C.POINTER(C.c_int * 8)]
    lib.icnn_be_debug_dual_plan.restype = C.c_int
    lib.icnn_be_debug_dual_step_body.argtypes = [C.POINTER(State), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.icnn_be_debug_dual_step_body.restype = C.c_int
    lib.icnn_be_debug_shape_instance.argtypes = [C.POINTER(FcModel), C.POINTER(State)]
    lib.icnn_be_debug_shape_instance.restype = C.c_int
    lib.icnn_be_debug_fc_deal.argtypes = [C.POINTER(FcModel), C.POINTER(C.c_int), C.c_int]
    lib.icnn_be_debug_fc_deal.restype = C.c_int
    lib.icnn_be_adam_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.icnn_be_adam_workspace_bytes.restype = C.c_size_t
    lib.icnn_be_adam_fc.argtypes = [C.POINTER(FcModel), C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.icnn_be_adam_fc.restype = C.c_int
    lib.icnn_be_adam_fc_each.argtypes = [C.POINTER(FcModel), C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.icnn_be_adam_fc_each.restype = C.c_int
    lib.icnn_be_debug_adam_each_plan.argtypes = [C.POINTER(FcModel), C.c_int, C.POINTER(C.c_int * 2)]
    lib.icnn_be_debug_adam_each_plan.restype = C.c_int
    lib.icnn_be_adam_fc_obs.argtypes = [C.POINTER(FcModel), C.POINTER(FcCtx), C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.icnn_be_adam_fc_obs.restype = C.c_int
    lib.icnn_be_fc_context_work_floats.argtypes = [C.POINTER(FcCtx), C.c_int]
    lib.icnn_be_fc_context_work_floats.restype = C.c_size_t
    lib.icnn_be_fc_context.argtypes = [C.POINTER(FcCtx), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_fc_context.restype = C.c_int
    lib.icnn_be_fc_context_stage.argtypes = [C.POINTER(FcCtx), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p]
    lib.icnn_be_fc_context_stage.restype = C.c_int
    lib.icnn_be_fc_context_norm.argtypes = [C.POINTER(FcCtx), C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_fc_context_norm.restype = C.c_int
    lib.icnn_be_fc_clamp.argtypes = [C.POINTER(FcModel), C.c_int, C.c_void_p]
    lib.icnn_be_fc_clamp.restype = C.c_int
    lib.icnn_be_conv_context_work_floats.argtypes = [C.POINTER(ConvModel), C.c_int]
    lib.icnn_be_conv_context_work_floats.restype = C.c_size_t
    lib.icnn_be_conv_context.argtypes = [C.POINTER(ConvModel), C.POINTER(ConvCtx), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    lib.icnn_be_conv_context.restype = C.c_int
    lib.icnn_be_conv_clamp.argtypes = [C.POINTER(ConvModel), C.c_int, C.c_void_p]
    lib.icnn_be_conv_clamp.restype = C.c_int
    lib.icnn_be_fc_grad_floats.argtypes = [C.POINTER(FcModel), C.POINTER(FcCtx)]
    lib.icnn_be_fc_grad_floats.restype = C.c_size_t
    lib.icnn_be_fc_surrogate_grad_work_floats.argtypes = [C.POINTER(FcModel), C.POINTER(FcCtx), C.c_int, C.c_int]
    lib.icnn_be_fc_surrogate_grad_work_floats.restype = C.c_size_t
    lib.icnn_be_fc_surrogate_grad.argtypes = [C.POINTER(FcModel), C.POINTER(FcCtx), C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    lib.icnn_be_fc_surrogate_grad.restype = C.c_int
    lib.icnn_be_conv_grad_floats.argtypes = [C.POINTER(ConvModel), C.POINTER(ConvCtx)]
    lib.icnn_be_conv_grad_floats.restype = C.c_size_t
    lib.icnn_be_conv_surrogate_grad_work_floats.argtypes = [C.POINTER(ConvModel), C.POINTER(ConvCtx), C.c_int, C.c_int]
    lib.icnn_be_conv_surrogate_grad_work_floats.restype = C.c_size_t
    lib.icnn_be_conv_surrogate_grad.argtypes = [C.POINTER(ConvModel), C.POINTER(ConvCtx), C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]
    lib.icnn_be_conv_surrogate_grad.restype = C.c_int
    lib.icnn_be_fc_context_bn_work_floats.argtypes = [C.POINTER(FcCtx), C.c_int]
    lib.icnn_be_fc_context_bn_work_floats.restype = C.c_size_t
    lib.icnn_be_fc_context_bn.argtypes = [C.POINTER(FcCtx), C.POINTER(BnMoving), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_fc_context_bn.restype = C.c_int
    lib.icnn_be_conv_context_bn_work_floats.argtypes = [C.POINTER(ConvModel), C.c_int]
    lib.icnn_be_conv_context_bn_work_floats.restype = C.c_size_t
    lib.icnn_be_conv_context_bn.argtypes = [C.POINTER(ConvModel), C.POINTER(ConvCtx), C.POINTER(BnMoving), C.c_int, C.c_int,
                                            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_conv_context_bn.restype = C.c_int
    lib.icnn_be_fc_surrogate_grad_bn.argtypes = (lib.icnn_be_fc_surrogate_grad.argtypes[:-1]
                                                 + [C.POINTER(BnMoving), C.c_int, C.c_void_p])
    lib.icnn_be_fc_surrogate_grad_bn.restype = C.c_int
    lib.icnn_be_conv_surrogate_grad_bn.argtypes = (lib.icnn_be_conv_surrogate_grad.argtypes[:-1]
                                                   + [C.POINTER(BnMoving), C.c_int, C.c_void_p])
    lib.icnn_be_conv_surrogate_grad_bn.restype = C.c_int
    lib.icnn_be_fc_surrogate_grad_dev.argtypes = (lib.icnn_be_fc_surrogate_grad.argtypes[:-1]
                                                  + [C.POINTER(BnMoving), C.c_int, C.c_void_p, C.c_void_p])
    lib.icnn_be_fc_surrogate_grad_dev.restype = C.c_int
    lib.icnn_be_conv_surrogate_grad_dev.argtypes = (lib.icnn_be_conv_surrogate_grad.argtypes[:-1]
                                                    + [C.POINTER(BnMoving), C.c_int, C.c_void_p, C.c_void_p])
    lib.icnn_be_conv_surrogate_grad_dev.restype = C.c_int
    lib.icnn_be_fc_context_bn_dev.argtypes = [C.POINTER(FcCtx), C.POINTER(BnMoving), C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_fc_context_bn_dev.restype = C.c_int
    lib.icnn_be_conv_context_bn_dev.argtypes = [C.POINTER(ConvModel), C.POINTER(ConvCtx), C.POINTER(BnMoving), C.c_void_p,
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_conv_context_bn_dev.restype = C.c_int
    lib.icnn_be_feed_plan_work_bytes.argtypes = [C.c_int]
    lib.icnn_be_feed_plan_work_bytes.restype = C.c_size_t
    lib.icnn_be_fc_surrogate_grad_dev_work_floats.argtypes = lib.icnn_be_fc_surrogate_grad_work_floats.argtypes
    lib.icnn_be_fc_surrogate_grad_dev_work_floats.restype = C.c_size_t
    lib.icnn_be_conv_surrogate_grad_dev_work_floats.argtypes = lib.icnn_be_conv_surrogate_grad_work_floats.argtypes
    lib.icnn_be_conv_surrogate_grad_dev_work_floats.restype = C.c_size_t
    lib.icnn_be_feed_plan.argtypes = [C.POINTER(State), C.c_void_p, C.c_int] + [C.c_void_p] * 6
    lib.icnn_be_feed_plan.restype = C.c_int
    lib.icnn_be_feed_pad.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.icnn_be_feed_pad.restype = C.c_int
    lib.icnn_be_step_gate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_step_gate.restype = C.c_int
    lib.icnn_be_gd_feed_work_bytes.argtypes = [C.c_int]
    lib.icnn_be_gd_feed_work_bytes.restype = C.c_size_t
    lib.icnn_be_gd_feed.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float] + [C.c_void_p] * 7)
    lib.icnn_be_gd_feed.restype = C.c_int
    lib.icnn_be_gd_feed_px_work_bytes.argtypes = [C.c_int] * 3
    lib.icnn_be_gd_feed_px_work_bytes.restype = C.c_size_t
    lib.icnn_be_gd_feed_px.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_float] * 2 + [C.c_void_p] * 6)
    lib.icnn_be_gd_feed_px.restype = C.c_int
    lib.icnn_be_gd_eval_work_bytes.argtypes = [C.c_int]
    lib.icnn_be_gd_eval_work_bytes.restype = C.c_size_t
    lib.icnn_be_gd_eval.argtypes = [C.c_void_p] * 2 + [C.c_int] * 2 + [C.c_void_p] * 4
    lib.icnn_be_gd_eval.restype = C.c_int
    lib.icnn_be_macro_f1.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_macro_f1.restype = C.c_int
    lib.icnn_be_keep_best.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_keep_best.restype = C.c_int
    lib.icnn_be_param_update.argtypes = [C.POINTER(ParamUpdateArgs), C.c_void_p]
    lib.icnn_be_param_update.restype = C.c_int
    lib.icnn_be_param_update_gated.argtypes = [C.POINTER(ParamUpdateArgs), C.c_void_p, C.c_void_p]
    lib.icnn_be_param_update_gated.restype = C.c_int
    lib.icnn_be_gated_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]
    lib.icnn_be_gated_copy.restype = C.c_int
    lib.icnn_be_gd_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.icnn_be_gd_workspace_bytes.restype = C.c_size_t
    lib.icnn_be_fc_gd.argtypes = ([C.POINTER(FcModel), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
                                  + [C.c_void_p] * 5)
    lib.icnn_be_fc_gd.restype = C.c_int
    lib.icnn_be_conv_gd.argtypes = [C.POINTER(ConvModel)] + lib.icnn_be_fc_gd.argtypes[1:]
    lib.icnn_be_conv_gd.restype = C.c_int
    lib.icnn_be_pgd_workspace_bytes.argtypes = [C.c_int, C.c_int]
    lib.icnn_be_pgd_workspace_bytes.restype = C.c_size_t
    lib.icnn_be_fc_pgd.argtypes = ([C.POINTER(FcModel), C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_double] * 3
                                   + [C.c_void_p] * 5)
    lib.icnn_be_fc_pgd.restype = C.c_int
    lib.icnn_be_conv_pgd.argtypes = [C.POINTER(ConvModel)] + lib.icnn_be_fc_pgd.argtypes[1:]
    lib.icnn_be_conv_pgd.restype = C.c_int
    lib.icnn_be_entropy_objective.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_entropy_objective.restype = C.c_int
    lib.icnn_be_bundle_trace.argtypes = [C.POINTER(State), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_bundle_trace.restype = C.c_int
    lib.icnn_be_dual_bound.argtypes = [C.POINTER(State), C.c_void_p, C.c_void_p]
    lib.icnn_be_dual_bound.restype = C.c_int
    lib.icnn_be_rl_td.argtypes = ([C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_longlong, C.c_void_p,
                                                                         C.c_float, C.c_float] + [C.c_void_p] * 5)
    lib.icnn_be_rl_td.restype = C.c_int
    lib.icnn_be_rl_critic_update.argtypes = [C.POINTER(RlUpdateArgs), C.c_void_p]
    lib.icnn_be_rl_critic_update.restype = C.c_int
    lib.icnn_be_replay_enqueue.argtypes = [C.POINTER(Replay), C.c_void_p, C.c_void_p]
    lib.icnn_be_replay_enqueue.restype = C.c_int
    lib.icnn_be_replay_sample.argtypes = [C.POINTER(Replay), C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 7
    lib.icnn_be_replay_sample.restype = C.c_int
    lib.icnn_be_vec_replay_enqueue.argtypes = [C.POINTER(VecReplay)] + [C.c_void_p] * 5
    lib.icnn_be_vec_replay_enqueue.restype = C.c_int
    lib.icnn_be_vec_replay_sample.argtypes = [C.POINTER(VecReplay), C.c_int, C.c_int, C.c_ulonglong] + [C.c_void_p] * 7
    lib.icnn_be_vec_replay_sample.restype = C.c_int
    lib.icnn_be_explore.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                    C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_explore.restype = C.c_int
    lib.icnn_be_dataset_draw.argtypes = [C.POINTER(Dataset), C.c_int, C.c_ulonglong, C.POINTER(C.c_void_p), C.c_void_p,
                                         C.c_void_p]
    lib.icnn_be_dataset_draw.restype = C.c_int
    lib.icnn_be_log_row.argtypes = [C.POINTER(StepLog), C.c_void_p]
    lib.icnn_be_log_row.restype = C.c_int
    DA = C.POINTER(DdpgArgs)
    lib.icnn_be_ddpg_param_floats.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_longlong)] * 2
    lib.icnn_be_ddpg_param_floats.restype = C.c_int
    lib.icnn_be_ddpg_work_bytes.argtypes = [C.c_int] * 5
    lib.icnn_be_ddpg_work_bytes.restype = C.c_size_t
    lib.icnn_be_ddpg_work_offsets.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_longlong * len(DDPG_WORK))]
    lib.icnn_be_ddpg_work_offsets.restype = C.c_int
    for name in ("chain", "grads", "update", "step"):
        fn = getattr(lib, "icnn_be_ddpg_" + name)
        fn.argtypes, fn.restype = [DA, C.c_void_p], C.c_int
    lib.icnn_be_ddpg_act.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_ddpg_act.restype = C.c_int
    lib.icnn_be_ddpg_q.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_ddpg_q.restype = C.c_int
    NA = C.POINTER(NafArgs)
    lib.icnn_be_naf_param_floats.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_longlong)] * 3
    lib.icnn_be_naf_param_floats.restype = C.c_int
    lib.icnn_be_naf_work_bytes.argtypes = [C.c_int] * 5
    lib.icnn_be_naf_work_bytes.restype = C.c_size_t
    lib.icnn_be_naf_work_offsets.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_longlong * len(NAF_WORK))]
    lib.icnn_be_naf_work_offsets.restype = C.c_int
    for name in ("chain", "grads", "update", "step"):
        fn = getattr(lib, "icnn_be_naf_" + name)
        fn.argtypes, fn.restype = [NA, C.c_void_p], C.c_int
    lib.icnn_be_naf_act.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_naf_act.restype = C.c_int
    lib.icnn_be_naf_q.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.icnn_be_naf_q.restype = C.c_int
    NB = C.POINTER(NafBnArgs)
    lib.icnn_be_naf_bn_param_floats.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_longlong)] * 5
    lib.icnn_be_naf_bn_param_floats.restype = C.c_int
    lib.icnn_be_naf_bn_layout.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_longlong * len(NAF_BN_VARS))]
    lib.icnn_be_naf_bn_layout.restype = C.c_int
    lib.icnn_be_naf_bn_work_bytes.argtypes = [C.c_int] * 5
    lib.icnn_be_naf_bn_work_bytes.restype = C.c_size_t
    lib.icnn_be_naf_bn_work_offsets.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_longlong * len(NAF_BN_WORK))]
    lib.icnn_be_naf_bn_work_offsets.restype = C.c_int
    for name in ("chain", "grads", "update", "step"):
        fn = getattr(lib, "icnn_be_naf_bn_" + name)
        fn.argtypes, fn.restype = [NB, C.c_void_p], C.c_int
    lib.icnn_be_naf_bn_act.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_float, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
    lib.icnn_be_naf_bn_act.restype = C.c_int
    lib.icnn_be_naf_bn_q.argtypes = ([C.c_int] * 4 + [C.c_void_p] * 6 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
                                     + [C.c_void_p] * 3)
    lib.icnn_be_naf_bn_q.restype = C.c_int
    FA = C.POINTER(FfArgs)
    ff_dims = [C.c_int] * 3 + [C.POINTER(C.c_int)]
    lib.icnn_be_ff_param_floats.argtypes = ff_dims + [C.POINTER(C.c_longlong)]
    lib.icnn_be_ff_param_floats.restype = C.c_int
    lib.icnn_be_ff_work_bytes.argtypes = [C.c_int] + ff_dims
    lib.icnn_be_ff_work_bytes.restype = C.c_size_t
    lib.icnn_be_ff_work_offsets.argtypes = [C.c_int] + ff_dims + [C.POINTER(C.c_longlong * len(FF_WORK))]
    lib.icnn_be_ff_work_offsets.restype = C.c_int
    lib.icnn_be_ff_forward.argtypes, lib.icnn_be_ff_forward.restype = [FA, C.c_int, C.c_void_p], C.c_int
    for name in ("backward", "grads", "update", "step", "eval"):
        fn = getattr(lib, "icnn_be_ff_" + name)
        fn.argtypes, fn.restype = [FA, C.c_void_p], C.c_int
    CA = C.POINTER(FcnArgs)
    lib.icnn_be_fcn_param_floats.argtypes, lib.icnn_be_fcn_param_floats.restype = [C.c_int] * 3 + [C.POINTER(C.c_longlong)], C.c_int
    lib.icnn_be_fcn_work_bytes.argtypes, lib.icnn_be_fcn_work_bytes.restype = [C.c_int] * 4, C.c_size_t
    lib.icnn_be_fcn_work_offsets.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_longlong * len(FCN_WORK))]
    lib.icnn_be_fcn_work_offsets.restype = C.c_int
    for name in ("forward", "backward", "grads", "update", "step", "eval"):
        fn = getattr(lib, "icnn_be_fcn_" + name)
        fn.argtypes, fn.restype = [CA, C.c_void_p], C.c_int
    FM = C.POINTER(FicnnModel)
    lib.icnn_be_ficnn_pack_floats.argtypes = [FM]
    lib.icnn_be_ficnn_pack_floats.restype = C.c_size_t
    lib.icnn_be_ficnn_pack.argtypes = [FM] + [C.POINTER(C.c_void_p)] * 3 + [C.c_void_p]
    lib.icnn_be_ficnn_pack.restype = C.c_int
    lib.icnn_be_ficnn_context_work_floats.argtypes = [FM, C.c_int]
    lib.icnn_be_ficnn_context_work_floats.restype = C.c_size_t
    lib.icnn_be_ficnn_context.argtypes = [FM, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.icnn_be_ficnn_context.restype = C.c_int
    lib.icnn_be_ficnn_fg.argtypes = [FM] + lib.icnn_be_fc_fg.argtypes[1:]
    lib.icnn_be_ficnn_fg.restype = C.c_int
    lib.icnn_be_ficnn_gd.argtypes = [FM] + lib.icnn_be_fc_gd.argtypes[1:]
    lib.icnn_be_ficnn_gd.restype = C.c_int
    lib.icnn_be_solve_ficnn.argtypes = [FM] + lib.icnn_be_solve_fc.argtypes[1:]
    lib.icnn_be_solve_ficnn.restype = C.c_int
    lib.icnn_be_ficnn_grad_floats.argtypes = [FM]
    lib.icnn_be_ficnn_grad_floats.restype = C.c_size_t
    lib.icnn_be_ficnn_surrogate_grad_work_floats.argtypes = [FM, C.c_int, C.c_int]
    lib.icnn_be_ficnn_surrogate_grad_work_floats.restype = C.c_size_t
    lib.icnn_be_ficnn_surrogate_grad.argtypes = [FM, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    lib.icnn_be_ficnn_surrogate_grad.restype = C.c_int
    lib.icnn_be_struct_size.argtypes = [C.c_int]
    lib.icnn_be_struct_size.restype = C.c_size_t
    if tuple(lib.icnn_be_struct_size(i) for i in range(7)) != (
            C.sizeof(State), C.sizeof(FcModel), C.sizeof(FcCtx), C.sizeof(ConvModel), C.sizeof(ConvCtx), C.sizeof(BnMoving),
            C.sizeof(ParamUpdateArgs)):
        raise ImportError("ctypes struct layout differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(7) != C.sizeof(RlUpdateArgs):
        raise ImportError("ctypes struct layout of icnn_be_rl_update_args differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(8) != C.sizeof(FicnnModel):
        raise ImportError("ctypes struct layout of icnn_be_ficnn_model differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(9) != C.sizeof(Replay):
        raise ImportError("ctypes struct layout of icnn_be_replay differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(22) != C.sizeof(VecReplay):
        raise ImportError("ctypes struct layout of icnn_be_vec_replay differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(10) != C.sizeof(Dataset) or lib.icnn_be_struct_size(11) != C.sizeof(StepLog):
        raise ImportError("ctypes struct layout of icnn_be_dataset / icnn_be_step_log differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(13) != C.sizeof(DdpgArgs):
        raise ImportError("ctypes struct layout of icnn_be_ddpg_args differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(14) != C.sizeof(NafArgs):
        raise ImportError("ctypes struct layout of icnn_be_naf_args differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(16) != C.sizeof(FfArgs):
        raise ImportError("ctypes struct layout of icnn_be_ff_args differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(18) != C.sizeof(FcnArgs):
        raise ImportError("ctypes struct layout of icnn_be_fcn_args differs from libicnn_be.so's")
    if lib.icnn_be_struct_size(20) != C.sizeof(NafBnArgs):
        raise ImportError("ctypes struct layout of icnn_be_naf_bn_args differs from libicnn_be.so's")
    if lib.icnn_be_abi_version() != ABI_VERSION:
        raise ImportError("libicnn_be.so ABI %d != binding ABI %d; rebuild with python -m icnn_amd.build"
                          % (lib.icnn_be_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc == 0:
        return
    msg = ERRORS.get(rc, "error %d" % rc)
    if rc == -3:
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


UNIT_KINDS = ["fwd_y", "fwd_z", "delta", "dedy", "e"]        # ICNN_BE_UNIT_*


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
    return ("double" if out[0] == CUT_F64 else "float", out[1], out[2], variant, bool(out[4]), DUAL_KERNELS[out[5]], out[6], out[7])
