"""The round class of the Bibsonomy instance of the persistent tile kernel (be_fused.hip, fused_fc_solve_kernel with CLASSES):
rounds 0 .. 7, whose bundles hold at most eight cuts, run a dual body compiled for that cap (dual_step_body, KCAP = 8 -- the
pass, the reduced Newton solve and the inertia count inlined, no MFMA sweep), later rounds the body every other kernel runs.
ICNN_BE_FLAG_NO_ROUND_CLASSES launches the instance without the class, and both must agree bit for bit: the same instances
of the same row algebra, inlined instead of called.

nIter 1, 4, 5, 6, 7, 8, 9 and 10 end inside the class, on the edges the three classes first built had (4, 6, 8 -- the classes
of up to 4 and up to 6 cuts did not pay and are not in the tree) and one past each; 9 and 10 cross into the plain body.

Inputs: Bernoulli(0.04) features from RandomState(SEED), the context of 64 rows (batch statistics), the first B of them solved
from two starts: "cold", y0 = 0.5, and "warm", the solution of the ten-round solve of the same rows plus 0.01 x standard normal
noise from RandomState(NOISE_SEED), clipped to [0.005, 0.995].  The warm start is what lets a bundle fill the cap of its round,
i.e. a sample end with count == nIter; seeds and start were looked for on the CPU with the oracle (oracle.solve_batch over
picnn_oracle.make_fg_chain on the host context picnn.context):
  * from y0 = 0.5 the first cuts are pruned in nearly every sample: over feature seeds 0 .. 999, 16 samples each, the fullest
    bundle holds 5 cuts at nIter 6 and 6 at nIter 8 (on the device with SEED = 4: 4, 4 and 6 cuts at nIter 4, 6, 8);
  * from the noisy solution most cuts stay active: over noise seeds 1000 .. 7999 (16 samples each, nIter 8) 6 samples in
    about 44 000 keep all eight cuts; 35 noise seeds have one, and each of the 35 also has a sample with count 6 at nIter 6
    and several with count 4 at nIter 4, in the oracle and -- all 35 -- on the device.  NOISE_SEED = 1375: samples 3, 7, 11,
    12, 14, 15 at nIter 4, samples 3 and 15 at nIter 6, sample 3 at nIter 8, all among the first 16 rows.
The cold start stays in the equality cases: it is the benchmark's."""
import numpy as np
import pytest
import torch

from icnn_amd import _lib, picnn

PERS, NOCLS, MFMA = _lib.FLAG_PERSISTENT, _lib.FLAG_NO_ROUND_CLASSES, _lib.FLAG_MFMA_CONTRACTION
BIB = picnn.bibtex_spec()
SEED = 4
NOISE_SEED, NOISE = 1375, 0.01
STARTS = ("cold", "warm")
BATCHES = (16, 17, 40)                 # 4-row tiles: 4, 5 (a ragged second tile row) and 10 workgroups
N_ITERS = (1, 4, 5, 6, 7, 8, 9, 10)
FIELDS = ("y", "count", "n_iters", "newton_iters", "active", "lam", "h", "G", "ys", "status")


# ---- host arithmetic: no GPU ------------------------------------------------------------------------------------------------

def fc_model(spec):
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = float(spec.alpha), int(spec.action_box), spec.ctx_width
    return m


def fc_state(spec, B, n_iter, flags):
    s = _lib.State()
    s.batch, s.n, s.slots, s.iters = B, spec.n_labels, n_iter, 0
    s.variant, s.flags, s.cut_dtype = _lib.VARIANT["dual"], flags, _lib.CUT_F32
    return s


@pytest.mark.parametrize("B,n_iter,flags,expected", [
    (4096, 10, 0, ("TILE", 16, 0, 10)), (2048, 10, 0, ("TILE", 8, 0, 10)), (4096, 5, 0, ("TILE", 16, 0, 5)),
    (40, 8, PERS, ("TILE", 4, 0, 8)), (4096, 10, _lib.FLAG_TWO_KERNELS, None), (128, 10, 0, None)])
def test_the_flag_does_not_change_the_plan(B, n_iter, flags, expected):
    """icnn_be_debug_solve_plan at 256 CUs: the table of tests/test_solve_plan.py, with and without the new flag"""
    m = fc_model(BIB)
    plain, flagged = (_lib.solve_plan(m, fc_state(BIB, B, n_iter, flags | f), 256) for f in (0, NOCLS))
    assert plain == flagged
    if expected is not None:
        assert plain == expected
    else:
        assert plain[0] != "TILE"
    assert _lib.shape_instance(m, fc_state(BIB, B, n_iter, flags)) == _lib.shape_instance(m, fc_state(BIB, B, n_iter, flags | NOCLS))


# ---- on the GPU -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def net():
    """(model, context of 64 rows, warm start of the 64 rows); built once, never written by a test"""
    from icnn_amd import bundle_entropy
    model = picnn.FCModel(BIB, picnn.init_params(BIB, 0, "spread"))
    x = (np.random.RandomState(SEED).rand(64, BIB.n_features) < 0.04).astype(np.float32)
    ctx = model.context(torch.from_numpy(x))
    ystar = bundle_entropy.FusedSolver(model, 64, 10, "dual", flags=PERS).solve(ctx, 0.5).y.clone()
    noise = torch.from_numpy(np.random.RandomState(NOISE_SEED).randn(64, BIB.n_labels)).to(ystar.device)
    return model, ctx, (ystar + NOISE * noise).clamp(0.005, 0.995)


_solved = {}


def solve(net, B, n_iter, flags, start="cold"):
    """one fused solve per (B, nIter, flags, start), shared by the tests; (instance name, plan, result tensors as clones)"""
    key = (B, n_iter, flags, start)
    if key not in _solved:
        from icnn_amd import bundle_entropy
        model, ctx_all, warm = net
        fs = bundle_entropy.FusedSolver(model, B, n_iter, "dual", flags=flags)
        res = fs.solve(ctx_all[:B].contiguous(), 0.5 if start == "cold" else warm[:B].contiguous())
        torch.cuda.synchronize()
        st = res.state
        out = {"y": res.y, "G": st.G, "ys": st.ys, "h": st.h, "lam": res.lam, "active": res.active, "count": res.count[:B],
               "n_iters": res.n_iters[:B], "newton_iters": res.newton_iters[:B], "status": res.status[:B]}
        _solved[key] = (_lib.shape_instance(model.c_model, st.c_state), _lib.solve_plan(model.c_model, st.c_state),
                        {k: v.clone() for k, v in out.items()})
    return _solved[key]


CASES = [(B, T, start) for B in BATCHES for T in N_ITERS for start in STARTS]


@pytest.mark.gpu
@pytest.mark.parametrize("B,n_iter,start", CASES, ids=["%d_%d_%s" % c for c in CASES])
def test_round_class_equals_the_one_body(net, B, n_iter, start):
    classes, plain = (solve(net, B, n_iter, PERS | f, start) for f in (0, NOCLS))
    assert classes[0] == plain[0] == "bibtex_kt16"                      # both are the instance of the shape
    assert classes[1] == plain[1] and classes[1][0] == "TILE"
    for k in FIELDS:
        assert np.array_equal(classes[2][k].cpu().numpy(), plain[2][k].cpu().numpy()), k
    assert int(classes[2]["status"].max()) == 0
    if n_iter >= 4:
        assert int(classes[2]["count"].max()) >= 2 and int(classes[2]["newton_iters"].max()) >= 1
    if start == "warm" and n_iter in (4, 6, 8):
        # not vacuous: a bundle filled the cap of the last round (count == nIter), in a solve both launches agree on
        count = classes[2]["count"].cpu().numpy()
        assert (count == n_iter).any(), "largest count %d" % int(count.max())


@pytest.mark.gpu
@pytest.mark.parametrize("n_iter", (6, 10))
def test_mfma_contraction_runs_the_one_body(net, n_iter):
    """the class is compiled for the fused VALU pass: with ICNN_BE_FLAG_MFMA_CONTRACTION the launcher must fall back"""
    sweep, plain = (solve(net, 40, n_iter, PERS | MFMA | f) for f in (0, NOCLS))
    assert sweep[0] == plain[0] == "bibtex_kt16"
    for k in FIELDS:
        assert np.array_equal(sweep[2][k].cpu().numpy(), plain[2][k].cpu().numpy()), k
    # and it is the sweep that ran: another summation order in the Newton solves than the pass
    valu = solve(net, 40, n_iter, PERS)
    assert not np.array_equal(sweep[2]["lam"].cpu().numpy(), valu[2]["lam"].cpu().numpy())
