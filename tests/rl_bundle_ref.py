"""Host restatement of the RL agent's critic training step with FLAGS.icnn_opt == 'bundle_entropy' (RL/src/icnn.py:148-158,
:304-323), from existing references only (test helper; shares no code with the kernels):
    y*             oracle.solve_batch, variant 'rl', from y0 = 0.5 on the float32 PICNN chain of oracle/picnn_oracle.py with
                   action_box on: fg(y) = (negQ(obs, 2y - 1), 2 grad)
    act2, q2       2y* - 1 and the chain energy at y*
    the rest       tests/rl_train_ref.py: td with act2 given and loss (td_and_loss here), critic_update (the test calls it with
                   the gradient the device fed, as tests/test_rl_train.py does)
and the screens the tests apply to their seeds, on the oracle alone."""
import contextlib
import dataclasses

import numpy as np
import torch

from icnn_amd import picnn
from oracle import bundle_entropy_oracle as oracle
from oracle import picnn_oracle

COND_MAX = 1e10          # a Newton system beyond it is singular to the float64 solve: six digits of its solution are noise


def spec_for(n, batchnorm=False, dimO=5, szs=(24, 20)):
    """the small critic of the tests (action_box False: the solver boxes it)"""
    return dataclasses.replace(picnn.halfcheetah_spec(), n_features=dimO, n_labels=n, szs=tuple(szs), action_box=False,
                               batchnorm=batchnorm)


def params_for(spec, seed, y_scale=1.0):
    """the "spread" weights of the RL tests; y_scale shrinks the y-path weights z{i}_yu/W: at 0.1 the energy is flat enough
    that the stall rule (rl :125-126) stops some samples of a batch early while others run every round"""
    params = picnn.init_params(spec, seed, "spread", yu_bias=1.0, gate_bias=1.0)
    for i in range(len(spec.szs) + 1):
        params["z%d_yu/W" % i] = params["z%d_yu/W" % i] * np.float32(y_scale)
    return params


def problem(n, B, seed, batchnorm=False, y_scale=1.0):
    """(spec, params, obs [B, dimO] float32, ctx [B, ctx_width] float32): the context rows by picnn.context on the host
    (inference mode with fresh moving statistics when the spec normalises), fed to the device and to the oracle alike"""
    spec = spec_for(n, batchnorm)
    params = params_for(spec, seed, y_scale)
    obs = np.random.RandomState(seed + 100).randn(B, spec.n_features).astype(np.float32)
    stats = picnn.init_bn_stats(spec) if batchnorm else None
    ctx = picnn.context(spec, params, torch.from_numpy(obs), bn_stats=stats).numpy()
    return spec, params, obs, np.ascontiguousarray(ctx, np.float32)


@contextlib.contextmanager
def _watch_linear_solves(record):
    """record (raised, condition number) of every np.linalg.solve made inside the block"""
    real = np.linalg.solve

    def solve(a, b):
        try:
            out = real(a, b)
        except np.linalg.LinAlgError:
            record.append((True, np.inf))
            raise
        record.append((False, float(np.linalg.cond(a)) if np.size(a) else 1.0))
        return out

    np.linalg.solve = solve
    try:
        yield
    finally:
        np.linalg.solve = real


class Solve:
    """the oracle's solve of one problem: y [B, n], act = 2y - 1, q = the chain energy at y (float32), counts, n_iters,
    stopped_at (the round of the sample's last cut), stalled (the stall rule of rl :125-126 finished it), singular (a Newton
    system raised or was beyond COND_MAX)"""


def solve(spec, params, ctx, n_iter=5):
    B, n = ctx.shape[0], spec.n_labels
    fg = picnn_oracle.make_fg_chain(params, ctx, list(spec.szs), spec.alpha, True)
    record = []
    with np.errstate(all="ignore"), _watch_linear_solves(record):
        ora = oracle.solve_batch(fg, np.full((B, n), 0.5), n_iter, variant="rl")
    out = Solve()
    out.ora, out.y = ora, np.array(ora.y, np.float64)
    out.act = 2.0 * out.y - 1.0
    out.q = fg(out.y)[0].astype(np.float32)
    out.counts = np.array([len(a) for a in ora.active])
    out.n_iters = np.array(ora.n_iters)
    cut = (np.asarray(ora.h) != 0) | np.any(np.asarray(ora.G) != 0, axis=2)              # [B, n_iter]: a cut was taken
    out.stopped_at = np.array([int(np.nonzero(c)[0].max()) for c in cut])
    out.stalled = np.asarray(ora.finished, bool)
    out.singular = any(raised or cond > COND_MAX for raised, cond in record)
    return out


def td_and_loss(s, e_critic, batch, theta, mask, discount, l2norm, wd, q2=None):
    """(td, c, loss) of the step whose target solve is `s` (a Solve on the target's moving-mode context of ob2): q2_src is the
    chain energy at y* with act2 passed, so that the entropy of act2 is added as icnn_be_rl_td adds it; q2 given: the target's
    fresh evaluation at act2 instead (BatchNorm).  e_critic: negQ(obs, act) float32."""
    import rl_train_ref as ref
    _, act, rew, _, term = batch
    _, _, td, c = ref.td(e_critic, act, rew, term, s.q if q2 is None else q2, s.act, discount, len(rew))
    return td, c, ref.loss(td, theta, mask, l2norm, wd)
