"""Host mirror of the RL agent's second inner optimiser, `Agent.bundle_entropy(func, obs)` (RL/src/icnn.py:148-158) with
func = `_fg` / `_fg_target` (negQ WITHOUT the entropy term: the bundle method carries H(y) itself): y0 = 0.5,
`solveBatch` of RL/src/bundle_entropy.py at nIter = 5 on fg(y) = (func(obs, 2y - 1), 2 grad), result 2y* - 1.

On the device that is variant 'rl' on an action_box view of the model (picnn.FCModel.boxed()).  Up to four samples per CU
the solve, the map y -> 2y - 1 and the value negQ(obs, 2y* - 1) are ONE launch of the persistent per-sample kernel
(`icnn_be_rl_bundle_solve`, be_fused.hip); beyond, the three existing steps are composed with the same outputs bit for bit.
There is no CPU fallback.
"""
import ctypes as C

import torch

from . import _lib
from .bundle_entropy import BundleState

ELIMIT = -2


class BundleActionResult:
    """Device tensors of one call, overwritten by the next: act [B, n] float64 in [-1, 1] (what the reference returns), q [B]
    float32 = negQ at act (no entropy term), y [B, n] float64 = the solver's iterate (act = 2y - 1), state = the
    bundle_entropy.BundleState (counts, n_iters, status, lam, active, the cuts)."""

    def __init__(self, act, q, y, state):
        self.act, self.q, self.y, self.state = act, q, y, state


class BundleActionSolver:
    """Reusable buffers for repeated calls at one batch shape.  `model`: picnn.FCModel of negQ; a model built with action_box
    False is solved through its boxed() view, so the caller keeps evaluating stored actions on the model as is.
    entry: True = the one-launch entry where the plan allows it (the default), False = always the three-step composition
    [icnn_be_solve_fc_reset, 2y - 1, icnn_be_fc_fg]."""

    def __init__(self, model, batch, n_iter=5, entry=True):
        self.model = model.boxed()
        self.batch, self.n_iter, self.entry = int(batch), int(n_iter), bool(entry)
        if self.batch < 1:
            raise ValueError("batch must be positive, got %r" % (batch,))
        self.lib = _lib.load()
        dev, n, B = model.device, model.spec.n_labels, self.batch
        self.y = torch.empty(B, n, dtype=torch.float64, device=dev)
        self.state = BundleState(self.y, self.n_iter, "rl", torch.float32)
        self.act = torch.empty(B, n, dtype=torch.float64, device=dev)
        self.q = torch.empty(B, dtype=torch.float32, device=dev)
        self.f_work = torch.empty(B, dtype=torch.float32, device=dev)
        self.g_work = torch.empty(B, n, dtype=torch.float32, device=dev)
        self._g = torch.empty(B, n, dtype=torch.float32, device=dev)        # the composition's fg writes a gradient nobody reads
        self.used_entry = None               # whether the last solve() ran the one-launch entry

    def _composed(self, ctx, y0, stream):
        m, st = self.model.c_model, self.state
        rounds = self.lib.icnn_be_solve_fc_reset(C.byref(m), ctx.data_ptr(), C.byref(st.c_state), self.f_work.data_ptr(),
                                                 self.g_work.data_ptr(), None, y0, stream)
        if rounds < 0:
            _lib.check(rounds, "icnn_be_solve_fc_reset")
        torch.mul(self.y, 2.0, out=self.act)
        self.act.sub_(1.0)
        _lib.check(self.lib.icnn_be_fc_fg(C.byref(m), ctx.data_ptr(), self.y.data_ptr(), self.batch, self.q.data_ptr(),
                                          self._g.data_ptr(), None, stream), "icnn_be_fc_fg")
        return rounds

    def solve(self, ctx: torch.Tensor, y0=0.5) -> BundleActionResult:
        """The solve from the constant start y0 on the context rows ctx [B, ctx_width] (float32, contiguous); current stream,
        no host synchronisation."""
        assert ctx.is_cuda and ctx.is_contiguous() and ctx.dtype == torch.float32
        assert ctx.shape == (self.batch, self.model.spec.ctx_width)
        st, stream = self.state, self.state.stream()
        rounds = ELIMIT
        if self.entry:
            rounds = self.lib.icnn_be_rl_bundle_solve(C.byref(self.model.c_model), ctx.data_ptr(), C.byref(st.c_state),
                                                      self.f_work.data_ptr(), self.g_work.data_ptr(), float(y0),
                                                      self.act.data_ptr(), self.q.data_ptr(), stream)
            if rounds < 0 and rounds != ELIMIT:
                _lib.check(rounds, "icnn_be_rl_bundle_solve")
        self.used_entry = rounds != ELIMIT
        if not self.used_entry:              # outside the per-sample plan: the three steps, the same bits
            rounds = self._composed(ctx, float(y0), stream)
        st.rounds = rounds
        self._keep = ctx
        return BundleActionResult(self.act, self.q, self.y, st)
