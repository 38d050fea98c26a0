"""NAF on the device (icnn_amd/naf.py, rl_agent.NAFAgent, icnn_be_naf_*, be_naf.hip) against
tests/naf_ref.py: the reference's analytic gradients against torch.autograd, the ABI and its argument checks, init_params
(CPU); the chain kernel, the weight gradients, the update, whole steps eager and captured, policy / q and the agent's cycle
with checkpoints (GPU).  Every tolerance is the reference's running bound n u M of that quantity (naf_ref's docstring); the
stage-wise test of the wide nets takes one stage's bound from the device's own operands (naf_ref.stage_step)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import naf_ref as ref
from icnn_amd import _lib, checkpoint, naf, rl_agent

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, dimO, dimA, l1, l2): one row, everything a partial tile and a 1 x 1 L that is only exp; exact column tiles and a batch
# one over a tile; K and N tails with dimA^2 = 9; dimA^2 = 25, an N tail in the second column tile of the L head; dimA^2 = 289,
# the widest head among the reference's environments, on narrow hidden layers; the shipped shape
SMALL = [(1, 3, 1, 5, 7), (17, 5, 2, 16, 16), (33, 3, 3, 20, 12), (20, 11, 5, 33, 18), (16, 4, 17, 8, 8)]
SHIPPED = (256, 17, 6, 200, 200)
# WIDE: hidden layers past 256 columns, where a wave of tile_gemm (be_tile.h) walks its column tiles more than once: 17 column
# tiles, so the second pass runs one tile with its pair predicated off, and a partial last tile; one column into tile 17 with K
# tails of 300 and 257; the largest sizes the ABI accepts, whose L head has dimA^2 = 1024 columns: four passes of every wave
WIDE = [(17, 5, 2, 272, 260), (33, 40, 3, 300, 257)]
WIDEST = (20, 600, 32, 600, 600)
SHAPES = SMALL + [SHIPPED] + WIDE + [WIDEST]
# The draw each shape is tested at.  The masks of a small shape must match exactly, so its draw must have no pre-activation
# below its own bound: MARGIN is the smallest |z| / bound of these draws on the CPU, which
# test_small_shapes_have_no_ambiguous_unit asserts (within 1 %: the figure is recorded, not chosen).  The shipped shape has
# ambiguous units at every seed (test_chain_kernel_against_the_reference prints how many), so flips there are legitimate.
# The WIDE shapes have some at every seed of 0 .. 11 too, at most 0.02 % and 0.14 % of any mask at these
# (test_wide_shapes_have_few_ambiguous_units caps them at 1 %); at WIDEST 3 % of the second layers' units are ambiguous end to
# end, and what tests that shape, and every WIDE one, layer by layer is test_stages_from_the_devices_own_operands.
SEED = {SMALL[0]: 0, SMALL[1]: 0, SMALL[2]: 0, SMALL[3]: 0, SMALL[4]: 0, SHIPPED: 0, WIDE[0]: 1, WIDE[1]: 0, WIDEST: 0}
MARGIN = {SMALL[0]: 82.09, SMALL[1]: 32.58, SMALL[2]: 16.04, SMALL[3]: 122.4, SMALL[4]: 597.6}
DISCOUNT = float(np.float32(0.99))
NEW_EXPORTS = ["icnn_be_naf_param_floats", "icnn_be_naf_work_bytes", "icnn_be_naf_work_offsets", "icnn_be_naf_chain",
               "icnn_be_naf_grads", "icnn_be_naf_update", "icnn_be_naf_step", "icnn_be_naf_act", "icnn_be_naf_q"]
W = ("l", "u", "v")


def _nets(shape, seed):
    """the four nets of a test: uniform +-1/sqrt(fan-in) everywhere, the target a draw of its own"""
    _, dimO, dimA, l1, l2 = shape
    a, b = ref.uniform_params(dimO, dimA, l1, l2, seed), ref.uniform_params(dimO, dimA, l1, l2, seed + 100)
    return a["L"], a["U"], a["V"], b["V"]


@functools.lru_cache(maxsize=None)
def _reference(shape):
    seed = SEED[shape]
    nets = _nets(shape, seed)
    mb = ref.batch(shape[0], shape[1], shape[2], seed)
    return nets + (mb,) + ref.reference_step(*nets, mb, DISCOUNT)


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("shape", [(5, 3, 2, 6, 4), (7, 4, 3, 5, 9)])
def test_reference_gradients_match_autograd(shape):
    """the analytic gradient of naf_ref against torch.autograd in float64: an independent derivation"""
    B, dimO, dimA, l1, l2 = shape
    L, Un, V, VT = _nets(shape, 3)
    mb = ref.batch(B, dimO, dimA, 3)
    l2norm = 1e-2
    fw, _, d, _, _, _ = ref.reference_step(L, Un, V, VT, mb, DISCOUNT)
    g = ref.weight_grads(mb[0].astype(np.float64), fw, d)
    mine = {w: g[w] + l2norm * ref.flat(ref.f64(N)) for w, N in zip(W, (L, Un, V))}
    # the head's own gradient: the upper triangle of d / d l is exactly 0 and the diagonal carries the exp factor
    g3 = d["d3l"].reshape(B, dimA, dimA)
    upper = np.triu(np.ones((dimA, dimA), bool), 1)
    assert np.all(g3[:, upper] == 0.0) and np.abs(g3[:, ~upper]).min() > 0
    gh = -(2.0 * fw["td"] / B)[:, None] * fw["h"]
    diag = np.arange(dimA)
    np.testing.assert_allclose(g3[:, diag, diag], fw["delta"] * gh * np.exp(fw["l"].reshape(B, dimA, dimA)[:, diag, diag]), rtol=1e-14)

    def t(net, grad):
        return {k: torch.tensor(np.asarray(v, np.float64), requires_grad=grad) for k, v in net.items()}

    def mlp(N, o):
        return torch.relu(torch.relu(o @ N["W1"] + N["b1"]) @ N["W2"] + N["b2"]) @ N["W3"] + N["b3"]

    obs, act, rew, ob2 = (torch.tensor(np.asarray(x, np.float64)) for x in mb[:4])
    term = torch.tensor(mb[4] != 0)
    tL, tU, tV, tVT = t(L, True), t(Un, True), t(V, True), t(VT, False)
    with torch.no_grad():
        y = torch.where(term, rew, rew + DISCOUNT * mlp(tVT, ob2)[:, 0])
    lm = mlp(tL, obs).reshape(B, dimA, dimA)
    Lm = torch.tril(lm, -1) + torch.diag_embed(torch.exp(torch.diagonal(lm, dim1=1, dim2=2)))
    delta = act - torch.tanh(mlp(tU, obs))
    h = torch.bmm(delta[:, None, :], Lm)[:, 0]
    q = mlp(tV, obs)[:, 0] - 0.5 * (h * h).sum(1)
    sq = sum((v ** 2).sum() for N in (tL, tU, tV) for v in N.values())
    loss = ((q - y) ** 2).mean() + l2norm * 0.5 * sq
    for w, N in zip(W, (tL, tU, tV)):
        auto = torch.autograd.grad(loss, [N[k] for k in ref.NAMES], retain_graph=True)
        want = np.concatenate([x.numpy().reshape(-1) for x in auto])
        assert np.abs(want).max() > 1e-3
        np.testing.assert_allclose(mine[w], want, rtol=1e-11, atol=1e-14)
    assert abs(ref.loss_q([ref.f64(N) for N in (L, Un, V)], fw, l2norm) - loss.item()) < 1e-13


def test_new_exports_declared_and_abi():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"ICNN_BE_API\s+(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.icnn_be_abi_version() == 12 and "#define ICNN_BE_ABI_VERSION 12" in header
    assert lib.icnn_be_struct_size(14) == C.sizeof(_lib.NafArgs) and lib.icnn_be_struct_size(15) == 0
    for name, value in (("MAX_OBS", _lib.NAF_MAX_OBS), ("MAX_ACT", _lib.NAF_MAX_ACT), ("MAX_HIDDEN", _lib.NAF_MAX_HIDDEN),
                        ("STEP_INTS", _lib.NAF_STEP_INTS), ("WORK_PIECES", len(_lib.NAF_WORK))):
        assert "#define ICNN_BE_NAF_%s %d" % (name, value) in header
    for i, piece in enumerate(_lib.NAF_WORK):
        assert re.search(r"#define ICNN_BE_NAF_W_%s %d\b" % (piece.upper(), i), header), piece
    assert _lib.NAF_MAX_OBS >= 376 and _lib.NAF_MAX_ACT >= 17 and _lib.NAF_MAX_HIDDEN >= 600


def test_sizes_and_workspace_layout():
    lib = _lib.load()
    for dims in ((376, 17, 600, 600), (1, 1, 1, 1), (17, 6, 200, 200), (600, 32, 600, 600)):
        n = [C.c_longlong() for _ in W]
        assert lib.icnn_be_naf_param_floats(*dims, *[C.byref(x) for x in n]) == 0
        spec = naf.NAFSpec(*dims)
        assert [x.value for x in n] == [naf.n_floats(spec, w) for w in W]
        off = (C.c_longlong * len(_lib.NAF_WORK))()
        assert lib.icnn_be_naf_work_offsets(256, *dims, C.byref(off)) == 0
        off = list(off)
        assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:])) and all(o % 4 == 0 for o in off)
        assert lib.icnn_be_naf_work_bytes(256, *dims) >= 4 * off[-1] + 8
    for bad in ((0, 1, 1, 1), (601, 1, 1, 1), (1, 0, 1, 1), (1, 33, 1, 1), (1, 1, 0, 1), (1, 1, 601, 1), (1, 1, 1, 0), (1, 1, 1, 601)):
        assert lib.icnn_be_naf_work_bytes(4, *bad) == 0
        assert lib.icnn_be_naf_param_floats(*bad, *[C.byref(C.c_longlong()) for _ in W]) == -1
        assert lib.icnn_be_naf_work_offsets(4, *bad, C.byref((C.c_longlong * len(_lib.NAF_WORK))())) == -1
    assert lib.icnn_be_naf_work_bytes(0, 3, 1, 5, 7) == 0


def _fake_args(**kw):
    """a descriptor of pointers that are never followed: every entry must refuse it before a launch"""
    a = _lib.NafArgs()
    a.batch, a.dimO, a.dimA, a.l1, a.l2 = 4, 3, 1, 5, 7
    for i, (name, _) in enumerate(f for f in _lib.NafArgs._fields_ if f[1] is C.c_void_p):
        setattr(a, name, 4096 * (i + 1))
    a.rate, a.beta1, a.beta2 = 1e-3, 0.9, 0.999
    a.eps, a.tau, a.discount, a.l2norm = 1e-4, 0.01, 0.99, 1e-4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_refused_before_a_launch():
    lib = _lib.load()
    entries = [lib.icnn_be_naf_chain, lib.icnn_be_naf_grads, lib.icnn_be_naf_update, lib.icnn_be_naf_step]
    bad = [dict(batch=0), dict(batch=-3), dict(dimO=0), dict(dimO=_lib.NAF_MAX_OBS + 1), dict(dimA=0),
           dict(dimA=_lib.NAF_MAX_ACT + 1), dict(l1=0), dict(l1=_lib.NAF_MAX_HIDDEN + 1), dict(l2=-1),
           dict(l2=_lib.NAF_MAX_HIDDEN + 1), dict(tau=-0.01), dict(tau=1.5), dict(tau=float("nan")),
           dict(discount=float("inf")), dict(discount=float("nan")), dict(l2norm=-1.0), dict(l2norm=float("nan")),
           dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0), dict(rate=float("nan")), dict(rate=float("inf"))]
    pointers = [name for name, kind in _lib.NafArgs._fields_ if kind is C.c_void_p]
    bad += [{name: None} for name in pointers if name != "loss"]
    bad += [{name: 4096 + 4} for name in ("theta_l", "theta_u", "theta_v", "target_v", "m_l", "v_l", "m_u", "v_u", "m_v", "v_v",
                                          "grad_l", "grad_u", "grad_v", "work")]
    bad += [{name: 4096 + 2} for name in ("obs", "rew", "ob2", "step", "loss")] + [dict(act=4096 + 4)]
    for kw in bad:
        for fn in entries:
            assert fn(C.byref(_fake_args(**kw)), None) == -1, kw
    for fn in entries:
        assert fn(None, None) == -1
        assert fn(C.byref(_fake_args()), C.c_void_p(4)) == -1           # a misaligned stream
    assert lib.icnn_be_naf_step(C.byref(_fake_args(loss=None)), None) == -1
    for fn, n_ptr, n16 in ((lib.icnn_be_naf_act, 2, 1), (lib.icnn_be_naf_q, 5, 3)):
        good = [4096 * (i + 1) for i in range(n_ptr)]
        for dims in ((0, 1, 5, 7), (3, 0, 5, 7), (3, 1, 0, 7), (3, 1, 5, 0), (601, 1, 5, 7), (3, 33, 5, 7), (3, 1, 601, 7),
                     (3, 1, 5, 601)):
            assert fn(*dims, *good, 4, 8192 * 4, None) == -1, dims
        assert fn(3, 1, 5, 7, *good, 0, 8192 * 4, None) == -1
        assert fn(3, 1, 5, 7, *good, 4, None, None) == -1
        assert fn(3, 1, 5, 7, *good, 4, 8192 * 4 + 2, None) == -1
        assert fn(3, 1, 5, 7, *good, 4, 8192 * 4, C.c_void_p(4)) == -1
        for i in range(n_ptr):
            assert fn(3, 1, 5, 7, *[None if j == i else p for j, p in enumerate(good)], 4, 8192 * 4, None) == -1
            assert fn(3, 1, 5, 7, *[p + 2 if j == i else p for j, p in enumerate(good)], 4, 8192 * 4, None) == -1
        for i in range(n16):                                            # a net that is 4- but not 16-byte aligned
            assert fn(3, 1, 5, 7, *[p + 4 if j == i else p for j, p in enumerate(good)], 4, 8192 * 4, None) == -1


def test_init_params_ranges_and_shapes():
    dimO, dimA, l1, l2 = 17, 6, 200, 150
    params = naf.init_params(dimO, dimA, l1, l2, 5)
    spec = naf.NAFSpec(dimO, dimA, l1, l2)
    assert set(params) == {"l", "u", "v", "target_v"}
    for which, width in (("l", dimA * dimA), ("u", dimA), ("v", 1)):
        net = params[which]
        assert [(k, v.shape) for k, v in net.items()] == naf.layout(spec, which)
        assert net["W3"].shape == (l2, width)
        for name, a in net.items():
            assert a.dtype == np.float32
            if name.startswith("b"):
                assert not a.any()
            else:
                assert np.abs(a).max() <= 2 * 0.01
                if a.size >= 1000:                                  # a cut normal of that std: not a narrower draw
                    assert np.abs(a).max() > 1.8 * 0.01 and 0.8 * 0.01 < a.std() < 0.01 and abs(a.mean()) < 1e-3
        flat = naf.flatten(spec, which, net)
        assert flat.shape == (naf.n_floats(spec, which),)
        back = naf.unflatten(spec, which, flat)
        assert all(np.array_equal(back[k], net[k]) for k in net)
    assert all(np.array_equal(params["target_v"][k], params["v"][k]) for k in params["v"])
    assert params["target_v"]["W1"] is not params["v"]["W1"]
    again = naf.init_params(dimO, dimA, l1, l2, 5)
    assert all(np.array_equal(again[w][k], params[w][k]) for w in params for k in params[w])
    other = naf.init_params(dimO, dimA, l1, l2, 6)
    assert not np.array_equal(other["l"]["W1"], params["l"]["W1"])
    wide = naf.init_params(dimO, dimA, l1, l2, 5, initstd=0.5)
    assert 0.5 < np.abs(wide["u"]["W2"]).max() <= 1.0


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes_have_no_ambiguous_unit(shape):
    """the precondition of the exact mask comparison: no pre-activation of the small shapes lies below its own bound"""
    fw, bound_fw, ambiguous = _reference(shape)[5], _reference(shape)[6], _reference(shape)[10]
    assert not any(a.any() for a in ambiguous.values())
    margin = min((np.abs(fw[z]) / bound_fw[z]).min() for z in ref.MASKS.values())
    print("smallest |z| / bound %.4g" % margin)
    assert margin > 8 and abs(margin / MARGIN[shape] - 1) < 0.01


@pytest.mark.parametrize("shape", WIDE)
def test_wide_shapes_have_few_ambiguous_units(shape):
    """at most 1 % of the units of any mask lie below their own end-to-end bound"""
    ambiguous = _reference(shape)[10]
    for k, a in ambiguous.items():
        print("ambiguous %s: %d of %d" % (k, a.sum(), a.size))
        assert a.mean() <= 0.01, k


STAGE_INPUTS = ("l", "y") + tuple(k + w for k in ("h1", "h2", "d3", "d2") for w in W)


@pytest.mark.parametrize("shape", WIDE + [WIDEST])
def test_stage_bounds_leave_few_units_ambiguous(shape):
    """the precondition of the stage-wise mask comparison, from the reference's own activations: under one layer's rounding
    at most 1 % of a layer's units lie below their bound"""
    L, Un, V, _, mb, fw, _, d = _reference(shape)[:8]
    dev = {k: fw[k] if k in fw else d[k] for k in STAGE_INPUTS}
    s = ref.stage_step(L, Un, V, mb[0], mb[1], dev, shape[0])
    assert set(s.pre) == set(ref.MASKS)
    for k, a in s.ambiguous().items():
        print("ambiguous %s: %d of %d" % (k, a.sum(), a.size))
        assert a.mean() <= 0.01, k
    # the stages, chained through the reference's own values, restate the reference's step
    for k, want in s.want.items():
        np.testing.assert_allclose(want, d[k] if k in d else fw[k], rtol=1e-12, atol=1e-14, err_msg=k)


def test_the_widest_nets_are_accepted_and_one_more_unit_is_refused():
    """WIDEST is the largest every dimension goes, its LDS fits (naf_fits), and one more hidden unit or action dimension is
    refused by the size entries, before any launch"""
    lib = _lib.load()
    B, dimO, dimA, l1, l2 = WIDEST
    assert (dimO, dimA, l1, l2) == (_lib.NAF_MAX_OBS, _lib.NAF_MAX_ACT, _lib.NAF_MAX_HIDDEN, _lib.NAF_MAX_HIDDEN)
    for shape in WIDE + [WIDEST]:
        assert lib.icnn_be_naf_work_bytes(*shape) > 0
    for bad in ((dimO, dimA, l1 + 1, l2), (dimO, dimA, l1, l2 + 1), (dimO, dimA + 1, l1, l2), (dimO + 1, dimA, l1, l2)):
        assert lib.icnn_be_naf_work_bytes(B, *bad) == 0, bad
        assert lib.icnn_be_naf_work_offsets(B, *bad, C.byref((C.c_longlong * len(_lib.NAF_WORK))())) == -1, bad
        assert lib.icnn_be_naf_param_floats(*bad, *[C.byref(C.c_longlong()) for _ in W]) == -1, bad


# ------------------------------------------------------------------------------------------------ GPU


def _trainer(shape, **kw):
    """a NAFTrainer at `shape` holding the test's nets and minibatch"""
    B, dimO, dimA, l1, l2 = shape
    seed = SEED.get(shape, 0)
    L, Un, V, VT = _nets(shape, seed)
    tr = naf.NAFTrainer(dimO, dimA, l1, l2, batch=B, discount=DISCOUNT, **kw)
    tr.load(l=L, u=Un, v=V, target_v=VT)
    obs, act, rew, ob2, term = ref.batch(B, dimO, dimA, seed)
    for dst, src in ((tr.obs, obs), (tr.act, act), (tr.rew, rew), (tr.ob2, ob2), (tr.term, term)):
        dst.copy_(torch.from_numpy(src))
    return tr


def _host(t):
    return t.cpu().numpy().astype(np.float64)


def _within(name, got, want, bound):
    err = np.abs(got - want)
    assert got.shape == want.shape == bound.shape and err.size
    worst = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
    print("%s: largest error / bound %.3g (error %.3e, bound %.3e)" % (name, err[worst] / max(bound[worst], 1e-300), err[worst],
                                                                      bound[worst]))
    assert np.all(err <= bound), "%s: error %.3e beyond its bound %.3e at %s" % (name, err[worst], bound[worst], worst)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_chain_kernel_against_the_reference(shape):
    B, dimO, dimA, l1, l2 = shape
    L, Un, V, VT, mb, fw, bound_fw, _, _, own, ambiguous = _reference(shape)
    tr = _trainer(shape)
    tr.work.view(torch.int32).fill_(0x7fc0beef)
    tr.chain()
    torch.cuda.synchronize()
    work = tr.work.cpu().numpy().view(np.uint32)
    # nothing outside the B rows of each piece is written
    written = np.zeros(work.size, bool)
    for name in _lib.NAF_WORK[:_lib.NAF_WORK.index("upd")]:
        v = tr.work_view(name)
        at = tr.work_offsets[name]
        written[at:at + v.numel() * (2 if name == "sq" else 1)] = True
    assert np.all(work[~written] == 0x7fc0beef) and (~written).sum() > 0
    assert not np.any(work[written] == 0x7fc0beef)
    # the forward quantities
    for name in ("y", "u", "l", "ld", "h", "adv", "q", "td"):
        got = _host(tr.work_view(name))
        _within(name, got if fw[name].ndim == 2 else got[:, 0], fw[name], bound_fw[name])
    dev_h = {k: _host(tr.work_view(k)) for k in ref.MASKS}
    for k, h in dev_h.items():
        _within(k, h, fw[k], bound_fw[k])
    sq = tr.work_view("sq").cpu().numpy()
    td32 = tr.work_view("td").cpu().numpy()[:, 0].astype(np.float64)
    np.testing.assert_allclose(sq, [np.sum(td32[i:i + 16] ** 2) for i in range(0, B, 16)], rtol=17 * 2.0 ** -53, atol=0)
    # the masks: the reference's everywhere except at ambiguous units (the small shapes have none)
    dev_masks = {k: (h > 0).astype(np.float64) for k, h in dev_h.items()}
    n_ambiguous = sum(int(a.sum()) for a in ambiguous.values())
    print("ambiguous units: %d of %d" % (n_ambiguous, sum(a.size for a in ambiguous.values())))
    if shape in SMALL:
        assert n_ambiguous == 0
    for k in dev_masks:
        assert np.array_equal(dev_masks[k][~ambiguous[k]], own[k][~ambiguous[k]]), k
    # the deltas against the reference backward at the device's masks
    _, _, d, bound_d, _, _ = ref.reference_step(L, Un, V, VT, mb, DISCOUNT, masks=dev_masks)
    for name in ("d3l", "d2l", "d1l", "d3u", "d2u", "d1u", "d3v", "d2v", "d1v"):
        _within(name, _host(tr.work_view(name)), d[name], bound_d[name])
    g3 = tr.work_view("d3l").cpu().numpy().reshape(B, dimA, dimA)
    assert not g3[:, np.triu(np.ones((dimA, dimA), bool), 1)].any()      # the upper triangle: exactly zero


@pytest.mark.gpu
@pytest.mark.parametrize("shape", WIDE + [WIDEST])
def test_stages_from_the_devices_own_operands(shape):
    """Every stored layer output and delta of the chain once more, from the stored quantities it was formed from and the
    device's own parameters (naf_ref.stage_step): each bound holds one stage's roundings and stays sharp at the widest nets,
    where the end-to-end bounds say little.  A mask has the sign of its pre-activation wherever that exceeds its bound."""
    B, dimO, dimA, l1, l2 = shape
    tr = _trainer(shape)
    tr.chain()
    torch.cuda.synchronize()
    names = STAGE_INPUTS + ("u", "ld", "h", "adv", "q", "td") + tuple("d1" + w for w in W)
    dev = {k: _host(tr.work_view(k)) for k in names}
    for k in ("y", "adv", "q", "td"):
        dev[k] = dev[k][:, 0]
    s = ref.stage_step(*[tr.host_params(w) for w in W], _host(tr.obs), _host(tr.act), dev, B)
    for name, (z, e) in s.pre.items():
        sure = np.abs(z) > e
        print("%s: %d of %d units below their bound" % (name, (~sure).sum(), sure.size))
        assert (~sure).mean() <= 0.01, name
        assert np.array_equal((dev[name] > 0)[sure], (z > 0)[sure]), name
    for name in s.want:
        assert np.abs(s.want[name]).max() > 1e-7, name
        _within("stage " + name, dev[name], s.want[name], s.bound[name])
        ratio = float(np.median(s.bound[name][s.want[name] != 0] / np.abs(s.want[name][s.want[name] != 0])))
        print("stage %s: median bound / |value| %.3g" % (name, ratio))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradients_from_the_devices_own_operands(shape):
    B = shape[0]
    tr = _trainer(shape)
    tr.chain()
    tr.grads()
    torch.cuda.synchronize()
    got = {w: tr.grad[w].cpu().numpy() for w in W}
    obs = _host(tr.obs)
    d = {k + w: _host(tr.work_view(k + w)) for k in ("d3", "d2", "d1") for w in W}
    h = {k + w: _host(tr.work_view(k + w)) for k in ("h1", "h2") for w in W}
    want = ref.weight_grads(obs, h, d)
    mag = ref.weight_grads(np.abs(obs), {k: np.abs(v) for k, v in h.items()}, {k: np.abs(v) for k, v in d.items()})
    for w in W:                                      # one chain of B fma per element
        assert np.abs(want[w]).max() > 1e-5
        _within("g_" + w, got[w].astype(np.float64), want[w], B * ref.U * mag[w])
    # a second run gives the same bits
    for w in W:
        tr.grad[w].fill_(7.0)
    tr.chain()
    tr.grads()
    torch.cuda.synchronize()
    for w in W:
        assert np.array_equal(tr.grad[w].cpu().numpy().view(np.uint32), got[w].view(np.uint32)), w


def _state(tr):
    out = {w: tr.theta[w] for w in naf.NETS}
    for w in W:
        out["m_" + w], out["v_" + w] = tr.m[w], tr.v[w]
    return out


def _snapshot(tr):
    return {k: t.cpu().numpy().copy() for k, t in _state(tr).items()}


def _expected_update(tr, before, g, t):
    """update32 of the three nets from the state `before`, the device's gradients and the ONE step count after the update;
    only v has a target (l and u get a dummy one that is dropped)"""
    out = {}
    for w in W:
        target = before["target_v"] if w == "v" else np.zeros_like(before[w])
        th, m, v, tt = ref.update32(before[w], before["m_" + w], before["v_" + w], target, g[w], t, tr.rate, tr.l2norm, tr.tau)
        out.update({w: th, "m_" + w: m, "v_" + w: v})
        if w == "v":
            out["target_v"] = tt
    return out


def _same_bits(got, want):
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# the parameter counts of each of the three nets take every residue mod 4 over these (asserted below); the last has several
# workgroups per net
UPDATE_DIMS = [(3, 1, 5, 7), (3, 2, 5, 6), (4, 3, 5, 7), (2, 2, 3, 5), (3, 3, 5, 6), (2, 1, 3, 6), (17, 6, 200, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("tau, l2norm", [(0.01, 1e-2), (0.0, 0.0), (1.0, 1e-2), (0.3, 0.0)])
def test_update_bit_for_bit(tau, l2norm):
    residues = {w: set() for w in W}
    for dims in UPDATE_DIMS:
        B = 20
        tr = naf.NAFTrainer(*dims, batch=B, tau=tau, l2norm=l2norm, rate=1e-3, seed=4, initstd=0.3)
        rng = np.random.RandomState(7)
        g = {}
        for w in W:
            residues[w].add(tr.n[w] % 4)
            tr.m[w].copy_(torch.from_numpy(rng.uniform(-1e-2, 1e-2, tr.n[w]).astype(np.float32)))
            tr.v[w].copy_(torch.from_numpy(rng.uniform(0, 1e-3, tr.n[w]).astype(np.float32)))
            g[w] = rng.uniform(-1, 1, tr.n[w]).astype(np.float32)
            g[w][::5] = 0.0
            tr.grad[w].copy_(torch.from_numpy(g[w]))
        tr.theta["target_v"].copy_(torch.from_numpy(rng.uniform(-1, 1, tr.n["v"]).astype(np.float32)))
        sq = rng.uniform(0, 3, 2)                                   # the tile sums the chain would have left
        tr.work_view("sq").copy_(torch.from_numpy(sq))
        tr.step_count.copy_(torch.tensor([3, 0, 0, 0], dtype=torch.int32))
        for t in (4, 5):                                            # two updates: the count advances, the ticket is re-armed
            before = _snapshot(tr)
            tr.update()
            torch.cuda.synchronize()
            _same_bits(_snapshot(tr), _expected_update(tr, before, g, t))
            assert tr.step_count.cpu().tolist() == [t, 0, 0, 0] and tr.t == t     # exactly one count, by one
            # loss_q: float64 sums of float32 values, rounded to float32 once (the float64 sums err below 2^-30 of it)
            want = (sq[0] + sq[1]) / B + float(np.float32(l2norm)) * 0.5 * sum(np.sum(before[w].astype(np.float64) ** 2) for w in W)
            assert abs(tr.loss.item() - want) <= 2 * ref.U * abs(want), (tr.loss.item(), want)
        if l2norm == 0.0:                                           # a zero coefficient leaves g: m is b1 m + c1 g exactly
            f = np.float32
            assert np.array_equal(_snapshot(tr)["m_l"], f(0.9) * before["m_l"] + f(1.0 - 0.9) * g["l"])
        if tau == 0.0:                                              # (tau 1 is t - (t - v), which need not round to v)
            assert np.array_equal(_snapshot(tr)["target_v"], before["target_v"])
    assert residues == {w: {0, 1, 2, 3} for w in W}, residues


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(33, 3, 3, 20, 12), SHIPPED])
def test_three_whole_steps_eager_and_captured(shape):
    B, dimO, dimA, l1, l2 = shape
    kw = dict(l2norm=1e-2, rate=1e-3, tau=0.05)
    tr = _trainer(shape, **kw)
    mb = ref.batch(B, dimO, dimA, SEED[shape])
    eager = []
    for t in (1, 2, 3):
        before = _snapshot(tr)
        nets = [tr.host_params(w) for w in naf.NETS]
        loss = tr.step_buffers()
        torch.cuda.synchronize()
        g = {w: tr.grad[w].cpu().numpy() for w in W}
        after = _snapshot(tr)
        _same_bits(after, _expected_update(tr, before, g, t))
        assert tr.t == t
        fw, bound_fw, _, _, _, _ = ref.reference_step(*nets, mb, DISCOUNT)
        want = ref.loss_q([ref.f64(n) for n in nets[:3]], fw, kw["l2norm"])
        bound = bound_fw["loss_td"] + 2 * ref.U * want          # td's own error, then float64 sums rounded to float32 once
        print("loss_q %.9g, reference %.9g, bound %.3e" % (loss.item(), want, bound))
        assert abs(loss.item() - want) <= bound
        eager.append((after, loss.item()))
    assert all(not np.array_equal(eager[0][0][k], eager[2][0][k]) for k in naf.NETS)
    # a captured step replayed three times: a warm-up step outside the graph, undone, then the capture
    cap, fresh = _trainer(shape, **kw), _trainer(shape, **kw)
    cap.step_buffers()
    torch.cuda.synchronize()
    for dst, src in zip(_state(cap).values(), _state(fresh).values()):
        dst.copy_(src)
    cap.step_count.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = cap.step_buffers().clone()
    for after, loss in eager:
        g.replay()
        torch.cuda.synchronize()
        _same_bits(_snapshot(cap), after)
        assert np.float32(out.item()).view(np.uint32) == np.float32(loss).view(np.uint32)
    assert cap.t == 3


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 17])
def test_policy_and_q_equal_the_chain_bit_for_bit(B):
    """at the trainer's batch, and at B' != batch: the first rows of a larger batch through a forward launch of their own"""
    for dims in [(5, 2, 16, 16), (11, 5, 33, 18), (4, 17, 8, 8), (17, 6, 200, 200)] + [s[1:] for s in WIDE + [WIDEST]]:
        tr = _trainer((B,) + dims)
        tr.chain()
        u, q = tr.policy(tr.obs), tr.q(tr.obs, tr.act)
        big = _trainer((B + 20,) + dims)
        for w in naf.NETS:                                          # the same nets, whatever seed either shape is drawn at
            big.theta[w].copy_(tr.theta[w])
        big.obs[:B].copy_(tr.obs)
        big.act[:B].copy_(tr.act)
        u2, q2 = big.policy(big.obs[:B].contiguous()), big.q(big.obs[:B].contiguous(), big.act[:B].contiguous())
        torch.cuda.synchronize()
        want_u = tr.work_view("u").cpu().numpy().view(np.uint32)
        want_q = tr.work_view("q").cpu().numpy()[:, 0].view(np.uint32)
        assert np.abs(u.cpu().numpy()).max() > 0 and np.abs(q.cpu().numpy()).max() > 0
        for got_u, got_q in ((u, q), (u2, q2)):
            assert np.array_equal(got_u.cpu().numpy().view(np.uint32), want_u)
            assert np.array_equal(got_q.cpu().numpy().view(np.uint32), want_q)


# ---- the agent ----

EPISODE_STEPS, EPISODE_ENDS, WARMUP = 40, (13, 27), 8


def _script(dimO):
    """the scripted environment: observation t + 1 and the reward depend on the step and on the action taken"""
    rng = np.random.RandomState(11)
    base = rng.uniform(-1, 1, (EPISODE_STEPS + 1, dimO)).astype(np.float32)

    def next_obs(t, action):
        return (0.8 * base[t + 1] + 0.2 * np.float32(np.tanh(action.sum()))).astype(np.float32)

    return base, next_obs


def _agent(capture, seed=3):
    return rl_agent.NAFAgent(5, 3, l1=16, l2=12, bsize=16, warmup=WARMUP, iters=2, rmsize=64, seed=seed, capture=capture, tau=0.05,
                             l2norm=1e-3, initstd=0.3)


def _run(agent, first, last):
    """steps first .. last - 1 of the scripted episode; an episode ends after the steps of EPISODE_ENDS"""
    base, next_obs = _script(agent.dimO)
    actions = []
    if first == 0:
        agent.reset(base[0])
    for t in range(first, last):
        action = agent.act()
        actions.append(action.copy())
        term = t in EPISODE_ENDS
        agent.observe(float(np.cos(t) - np.abs(action).sum()), term, next_obs(t, action))
        if term:
            agent.reset(base[t + 1])
    return np.array(actions)


def _agent_state(agent):
    torch.cuda.synchronize()
    out = _snapshot(agent.trainer)
    out["step"] = agent.trainer.step_count.cpu().numpy()
    out["loss"] = np.atleast_1d(agent.trainer.loss.cpu().numpy())
    return out


@pytest.mark.gpu
def test_agent_is_silent_until_warmup():
    agent = _agent(False)
    start = _agent_state(agent)
    _run(agent, 0, WARMUP)
    quiet = _agent_state(agent)
    for k in start:
        assert np.array_equal(quiet[k].view(np.uint8), start[k].view(np.uint8)), k
    assert agent.t == WARMUP and agent.trainer.t == 0 and agent.memory.n == WARMUP
    _run(agent, WARMUP, WARMUP + 1)
    assert agent.trainer.t == 2                                 # iters steps on the first observation past the warm-up
    after = _agent_state(agent)
    assert all(not np.array_equal(after[k], start[k]) for k in naf.NETS)


@pytest.mark.gpu
def test_agent_capture_on_and_off_agree():
    runs = []
    for capture in (False, True):
        agent = _agent(capture)
        actions = _run(agent, 0, EPISODE_STEPS)
        agent.memory.raise_on_error()
        assert agent.t == EPISODE_STEPS and agent.trainer.t == 2 * (EPISODE_STEPS - WARMUP)
        assert (agent._graph is not None) == capture
        assert np.abs(actions).max() <= 1.0 and actions.dtype == np.float64 and actions.shape == (EPISODE_STEPS, 3)
        runs.append((actions, _agent_state(agent)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k].view(np.uint8), runs[1][1][k].view(np.uint8)), k
    # act(test=True) is u itself, without noise
    agent = _agent(False)
    agent.reset(_script(5)[0][0])
    want = agent.trainer.policy(torch.from_numpy(_script(5)[0][:1]).cuda()).cpu().numpy()[0]
    assert np.array_equal(agent.act(test=True), np.clip(want.astype(np.float64), -1, 1)) and not agent.noise.any()
    assert np.abs(want).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [False, True])
def test_agent_checkpoint_resumes_bit_for_bit(capture, tmp_path):
    whole = _agent(capture)
    want_actions = _run(whole, 0, EPISODE_STEPS)
    want = _agent_state(whole)
    cut = 25
    first = _agent(capture)
    got_head = _run(first, 0, cut)
    path = tmp_path / "naf.npz"
    checkpoint.save(path, first)
    if capture:                                                 # a graph captured before the load replays on the loaded state
        second = _agent(capture)
        _run(second, 0, 12)
        graph = second._graph
        assert graph is not None
    else:
        second = _agent(capture, seed=9)                        # other weights, another noise stream, another sampler seed
    pointers = {k: t.data_ptr() for k, t in _state(second.trainer).items()}
    checkpoint.load(path, second)
    assert pointers == {k: t.data_ptr() for k, t in _state(second.trainer).items()}     # into the existing tensors
    if capture:
        assert second._graph is graph
    got_tail = _run(second, cut, EPISODE_STEPS)
    second.memory.raise_on_error()
    assert np.array_equal(np.concatenate([got_head, got_tail]), want_actions)
    got = _agent_state(second)
    for k in want:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert second.t == EPISODE_STEPS
    # the trainer alone
    tr = naf.NAFTrainer(5, 3, 16, 12, batch=16, seed=1)
    checkpoint.save(tmp_path / "trainer.npz", second.trainer)
    checkpoint.load(tmp_path / "trainer.npz", tr)
    _same_bits(_snapshot(tr), _snapshot(second.trainer))
    with pytest.raises(ValueError):
        checkpoint.load(tmp_path / "trainer.npz", naf.NAFTrainer(5, 3, 16, 13, batch=16))
