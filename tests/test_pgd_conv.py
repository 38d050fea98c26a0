"""The conv model's side of the solver comparison (icnn_amd.pgd, be_pgd.hip): the PGD loop against the restatement around the
kernel-order oracle, the trace of a fused conv solve against the scripts' callback, and the certificate objective >= bound on
the small image."""
import numpy as np
import pytest
import torch

import pgd_ref
from icnn_amd import picnn
from pgd_ref import HI, LO, ULP
from test_pgd import LRS, check_trace, entr

SPEC = picnn.ConvSpec()                  # the reference's 64 x 32 image (tests/test_gd_conv.py)
SMALL = picnn.ConvSpec(32, 32)           # the small image of tests/test_conv_gd_trainer.py
# The certificate's margin on the small image, measured on the CPU as M_BIBTEX of test_pgd.py is: the largest |E32 - E64| of
# the kernel-order float32 oracle (picnn_conv_oracle.energy_and_grad_chain) against the same network evaluated in float64
# (picnn_conv_oracle.energy on float64 tensors) over every point that the "spread" solves (seed 1, B = 2, nIter 5, variants
# dual and pdipm) and the 3 x 10 PGD iterates visit is 3.114e-5 (|E| up to 253).  Times 4: two cut energies and the objective's
# own, with slack.
M_SMALL = 4 * 3.114e-5


def _setup(spec, B, seed):
    from oracle import picnn_conv_oracle
    params = picnn.init_conv_params(spec, seed, "spread")
    x = np.random.RandomState(seed + 50).rand(B, spec.H, spec.W, 1).astype(np.float32)
    model = picnn.ConvModel(spec, params)
    ctx = model.context(torch.from_numpy(x).cuda())
    fg = picnn_conv_oracle.make_fg_chain(params, ctx.cpu().numpy(), spec.H, spec.W)
    return model, ctx, fg


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 17])
def test_conv_solve_against_restatement(B):
    from icnn_amd import pgd
    K, lr = 3, 0.1
    n = SPEC.n_labels
    for seed in range(B, B + 20):
        model, ctx, fg = _setup(SPEC, B, seed)
        rng = np.random.RandomState(seed)
        y0 = np.repeat((0.2 + 0.6 * rng.rand(n))[None], B, axis=0)           # meanY-like start
        y0[:, ::97] = (-0.5, 0.0, 1.0, 2.0)[seed % 4]                        # some entries outside [lo, hi]
        ref, same = pgd_ref.screen_feeds(fg, y0, K, lr)
        if same:
            break
    else:
        raise AssertionError("no screened seed")
    y, obj, fin = pgd.solve(model, ctx, torch.from_numpy(y0).cuda().reshape(B, SPEC.H, SPEC.W, 1), K, lr, final=True)
    torch.cuda.synchronize()
    y, obj, fin = y.cpu().numpy(), obj.cpu().numpy(), fin.cpu().numpy()
    assert y.shape == (B, n) and obj.shape == (K, B) and fin.shape == (B,)
    dy = np.abs(y - ref["y"])
    de = np.abs(obj - ref["obj"]) / (8 * ULP * ref["scale"])
    print("  conv B=%d: max |dy| %.3e (bound %.3e), worst e_k error %.3f of its bound" % (B, dy.max(), pgd_ref.y_tolerance(K, lr),
                                                                                       de.max()))
    assert dy.max() <= pgd_ref.y_tolerance(K, lr)
    edge = (ref["y"] == LO) | (ref["y"] == HI)
    assert np.array_equal(y[edge], ref["y"][edge])
    assert de.max() <= 1.0
    assert (np.abs(fin - ref["obj_final"]) <= 8 * ULP * ref["scale_final"]).all()
    assert np.abs(ref["y"] - ref["iterates"][0]).max() > 1e-5
    # without the optional outputs: the same y_K; and a sample alone: the same bits
    y2, o2, f2 = pgd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, trace=False)
    y1, o1, f1 = pgd.solve(model, ctx[B - 1:].contiguous(), torch.from_numpy(y0[B - 1:]).cuda(), K, lr, final=True)
    torch.cuda.synchronize()
    assert o2 is None and f2 is None and np.array_equal(y2.cpu().numpy(), y)
    assert np.array_equal(y1.cpu().numpy()[0], y[B - 1]) and np.array_equal(o1.cpu().numpy()[:, 0], obj[:, B - 1])
    assert f1.cpu().numpy()[0] == fin[B - 1]


def _fused(spec, B, n_iter, variant, seed):
    from icnn_amd import bundle_entropy
    model, ctx, _ = _setup(spec, B, seed)
    seen = []
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=np.full((B, spec.n_labels), 0.5), nIter=n_iter, variant=variant,
                                    native=True, check=False,
                                    callback=lambda t, es, xs: seen.append((es - entr(xs), pgd_ref.objective_scale(es, xs))))
    return model, ctx, res, seen


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_conv_bundle_trace_against_the_scripts_callback(variant):
    model, ctx, res, seen = _fused(SPEC, 2, 5, variant, 0)
    check_trace(res, seen, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_certificate_objective_above_bound_small_conv(variant):
    from icnn_amd import pgd
    model, ctx, res, _ = _fused(SMALL, 2, 5, variant, 1)
    d = pgd.dual_bound(res)
    gap = pgd.gap(model, ctx, res)
    torch.cuda.synchronize()
    print("  small conv %s: gap %s" % (variant, gap.cpu().numpy()))
    assert bool(torch.isfinite(d).all())
    assert bool((gap >= -M_SMALL).all())
    assert float(gap.max()) > 0
    for lr in LRS:
        y, obj, fin = pgd.solve(model, ctx, 0.5, 10, lr, final=True)
        torch.cuda.synchronize()
        assert bool((obj >= d[None] - M_SMALL).all()) and bool((fin >= d - M_SMALL).all()), lr
    assert bool((fin < obj[0]).all())                 # at the smallest rate PGD descends (0.1 overshoots on this model)
