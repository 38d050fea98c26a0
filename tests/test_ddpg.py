"""DDPG on the device (icnn_amd/ddpg.py, rl_agent.DDPGAgent, icnn_be_ddpg_*, be_ddpg.hip) against
tests/ddpg_ref.py: the reference's analytic gradients against torch.autograd, the ABI and its argument checks, init_params
(CPU); the chain kernel, the weight gradients, the update, whole steps eager and captured, act and the agent's cycle with
checkpoints (GPU).  Every tolerance is the reference's running bound n u M of that quantity (ddpg_ref's docstring); the
stage-wise test of the wide nets takes one layer's bound from the device's own operands (ddpg_ref.stage_step)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import ddpg_ref as ref
from icnn_amd import _lib, checkpoint, ddpg, rl_agent

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, dimO, dimA, l1, l2): everything a partial tile; exact column tiles and a batch one over a tile; K and N tails twice;
# the shipped shape (l1 + dimA = 206, a K tail)
SMALL = [(1, 3, 1, 5, 7), (17, 5, 2, 16, 16), (33, 3, 1, 20, 12), (48, 11, 3, 33, 18)]
SHIPPED = (256, 17, 6, 200, 200)
# WIDE: hidden layers past 256 columns, where a wave of tile_gemm (be_tile.h) walks its column tiles more than once: 17 column
# tiles, so the second pass runs one tile with its pair predicated off, and a partial last tile; one column into tile 17 with K
# tails of 300 + 3 and 257; the largest sizes the ABI accepts, whose launch needs 163 456 of a workgroup's 163 840 LDS bytes
WIDE = [(17, 5, 2, 272, 260), (33, 40, 3, 300, 257)]
WIDEST = (20, 600, 32, 600, 600)
SHAPES = SMALL + [SHIPPED] + WIDE + [WIDEST]
# The draw each shape is tested at.  The masks of a small shape must match exactly, so its draw must have no pre-activation
# below its own bound: on the CPU the smallest |z| / bound of these draws is 8007, 24.6, 111 and 26.5 (seed 0 of the last
# shape has 0.80 and seed 2 has 1.24: avoided); test_small_shapes_have_no_ambiguous_unit asserts it.  The shipped shape
# has about 290 ambiguous units of 256 x 600 at every seed, so flips there are legitimate.  The WIDE shapes have ambiguous
# units at every seed of 0 .. 11, at most 0.14 % and 0.54 % of any mask at these (test_wide_shapes_have_few_ambiguous_units
# caps them at 1 %).  At WIDEST the end-to-end bounds say little (53 % of ch2 lies below its own): what tests that shape, and
# every WIDE one, layer by layer is test_stages_from_the_devices_own_operands.
SEED = {SMALL[0]: 0, SMALL[1]: 0, SMALL[2]: 2, SMALL[3]: 3, SHIPPED: 0, WIDE[0]: 7, WIDE[1]: 4, WIDEST: 0}
DISCOUNT = float(np.float32(0.99))
NEW_EXPORTS = ["icnn_be_ddpg_param_floats", "icnn_be_ddpg_work_bytes", "icnn_be_ddpg_work_offsets", "icnn_be_ddpg_chain",
               "icnn_be_ddpg_grads", "icnn_be_ddpg_update", "icnn_be_ddpg_step", "icnn_be_ddpg_act", "icnn_be_ddpg_q"]


def _nets(shape, seed):
    """the four nets of a test: uniform +-1/sqrt(fan-in) everywhere, the targets a draw of their own"""
    _, dimO, dimA, l1, l2 = shape
    a, b = ref.uniform_params(dimO, dimA, l1, l2, seed), ref.uniform_params(dimO, dimA, l1, l2, seed + 100)
    return a["p"], a["q"], b["p"], b["q"]


@functools.lru_cache(maxsize=None)
def _reference(shape):
    seed = SEED[shape]
    P, Q, PT, QT = _nets(shape, seed)
    mb = ref.batch(shape[0], shape[1], shape[2], seed)
    return (P, Q, PT, QT, mb) + ref.reference_step(P, Q, PT, QT, mb, DISCOUNT)


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("shape", [(5, 3, 2, 6, 4), (7, 4, 1, 5, 9)])
def test_reference_gradients_match_autograd(shape):
    """the analytic g_q and g_p of ddpg_ref against torch.autograd in float64: an independent derivation"""
    B, dimO, dimA, l1, l2 = shape
    P, Q, PT, QT = _nets(shape, 3)
    mb = ref.batch(B, dimO, dimA, 3)
    l2norm, pl2norm = 1e-2, 3e-3
    fw, _, d, _, masks, _ = ref.reference_step(P, Q, PT, QT, mb, DISCOUNT)
    xa = np.concatenate([fw["qh1"], mb[1]], axis=1)
    gq, gp = ref.weight_grads(mb[0].astype(np.float64), xa, fw["qh2"], fw["ph1"], fw["ph2"], d)
    gq, gp = gq + l2norm * ref.flat(ref.f64(Q)), gp + pl2norm * ref.flat(ref.f64(P))

    def t(net, grad):
        return {k: torch.tensor(np.asarray(v, np.float64), requires_grad=grad) for k, v in net.items()}

    def pol(N, o):
        return torch.tanh(torch.relu(torch.relu(o @ N["W1"] + N["b1"]) @ N["W2"] + N["b2"]) @ N["W3"] + N["b3"])

    def cri(N, o, a):
        h1 = torch.relu(o @ N["W1"] + N["b1"])
        return (torch.relu(torch.cat([h1, a], 1) @ N["W2"] + N["b2"]) @ N["W3"] + N["b3"])[:, 0]

    obs, act, rew, ob2 = (torch.tensor(np.asarray(x, np.float64)) for x in mb[:4])
    term = torch.tensor(mb[4] != 0)
    tP, tQ, tPT, tQT = t(P, True), t(Q, True), t(PT, False), t(QT, False)
    with torch.no_grad():
        y = torch.where(term, rew, rew + DISCOUNT * cri(tQT, ob2, pol(tPT, ob2)))
    sq = lambda N: sum((v ** 2).sum() for v in N.values())
    loss_q = ((cri(tQ, obs, act) - y) ** 2).mean() + l2norm * 0.5 * sq(tQ)
    auto_q = torch.autograd.grad(loss_q, [tQ[k] for k in ref.NAMES])
    frozen = {k: v.detach() for k, v in tQ.items()}
    loss_p = -cri(frozen, obs, pol(tP, obs)).mean() + pl2norm * 0.5 * sq(tP)
    auto_p = torch.autograd.grad(loss_p, [tP[k] for k in ref.NAMES])
    for mine, auto in ((gq, auto_q), (gp, auto_p)):
        want = np.concatenate([g.numpy().reshape(-1) for g in auto])
        assert np.abs(want).max() > 1e-3
        np.testing.assert_allclose(mine, want, rtol=1e-11, atol=1e-14)
    want_q, _ = ref.losses(ref.f64(P), ref.f64(Q), fw, l2norm, pl2norm)
    assert abs(want_q - loss_q.item()) < 1e-13


def test_new_exports_declared_and_abi():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"ICNN_BE_API\s+(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.icnn_be_abi_version() == 12 and "#define ICNN_BE_ABI_VERSION 12" in header
    assert lib.icnn_be_struct_size(12) == 0
    assert lib.icnn_be_struct_size(13) == C.sizeof(_lib.DdpgArgs)
    for name, value in (("MAX_OBS", _lib.DDPG_MAX_OBS), ("MAX_ACT", _lib.DDPG_MAX_ACT), ("MAX_HIDDEN", _lib.DDPG_MAX_HIDDEN),
                        ("STEP_INTS", _lib.DDPG_STEP_INTS), ("WORK_PIECES", len(_lib.DDPG_WORK))):
        assert "#define ICNN_BE_DDPG_%s %d" % (name, value) in header
    for i, piece in enumerate(_lib.DDPG_WORK):
        assert re.search(r"#define ICNN_BE_DDPG_W_%s %d\b" % (piece.upper(), i), header), piece
    assert _lib.DDPG_MAX_OBS >= 376 and _lib.DDPG_MAX_ACT >= 17 and _lib.DDPG_MAX_HIDDEN >= 600


def test_sizes_and_workspace_layout():
    lib = _lib.load()
    for dims in ((376, 17, 600, 600), (1, 1, 1, 1), (17, 6, 200, 200), (600, 32, 600, 600)):
        np_, nq = C.c_longlong(), C.c_longlong()
        assert lib.icnn_be_ddpg_param_floats(*dims, C.byref(np_), C.byref(nq)) == 0
        spec = ddpg.DDPGSpec(*dims)
        assert (np_.value, nq.value) == (ddpg.n_floats(spec, "p"), ddpg.n_floats(spec, "q"))
        off = (C.c_longlong * len(_lib.DDPG_WORK))()
        assert lib.icnn_be_ddpg_work_offsets(256, *dims, C.byref(off)) == 0
        off = list(off)
        assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:])) and all(o % 64 == 0 for o in off)
        assert lib.icnn_be_ddpg_work_bytes(256, *dims) >= 4 * off[-1]
    for bad in ((0, 1, 1, 1), (601, 1, 1, 1), (1, 0, 1, 1), (1, 33, 1, 1), (1, 1, 0, 1), (1, 1, 601, 1), (1, 1, 1, 0), (1, 1, 1, 601)):
        assert lib.icnn_be_ddpg_work_bytes(4, *bad) == 0
        assert lib.icnn_be_ddpg_param_floats(*bad, C.byref(C.c_longlong()), C.byref(C.c_longlong())) == -1
        assert lib.icnn_be_ddpg_work_offsets(4, *bad, C.byref((C.c_longlong * len(_lib.DDPG_WORK))())) == -1
    assert lib.icnn_be_ddpg_work_bytes(0, 3, 1, 5, 7) == 0


def _fake_args(**kw):
    """a descriptor of pointers that are never followed: every entry must refuse it before a launch"""
    a = _lib.DdpgArgs()
    a.batch, a.dimO, a.dimA, a.l1, a.l2 = 4, 3, 1, 5, 7
    for i, (name, _) in enumerate(f for f in _lib.DdpgArgs._fields_ if f[1] is C.c_void_p):
        setattr(a, name, 4096 * (i + 1))
    a.rate, a.prate, a.beta1, a.beta2 = 1e-3, 1e-4, 0.9, 0.999
    a.eps, a.tau, a.discount, a.l2norm, a.pl2norm = 1e-4, 0.01, 0.99, 1e-4, 0.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_invalid_arguments_are_refused_before_a_launch():
    lib = _lib.load()
    entries = [lib.icnn_be_ddpg_chain, lib.icnn_be_ddpg_grads, lib.icnn_be_ddpg_update, lib.icnn_be_ddpg_step]
    bad = [dict(batch=0), dict(batch=-3), dict(dimO=0), dict(dimO=_lib.DDPG_MAX_OBS + 1), dict(dimA=0),
           dict(dimA=_lib.DDPG_MAX_ACT + 1), dict(l1=0), dict(l1=_lib.DDPG_MAX_HIDDEN + 1), dict(l2=-1),
           dict(l2=_lib.DDPG_MAX_HIDDEN + 1), dict(tau=-0.01), dict(tau=1.5), dict(tau=float("nan")),
           dict(discount=float("inf")), dict(discount=float("nan")), dict(l2norm=-1.0), dict(pl2norm=float("nan")),
           dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0), dict(rate=float("nan")), dict(prate=float("inf"))]
    pointers = [name for name, kind in _lib.DdpgArgs._fields_ if kind is C.c_void_p]
    bad += [{name: None} for name in pointers if name != "loss"]
    bad += [{name: 4096 + 4} for name in ("theta_q", "theta_p", "target_q", "target_p", "m_q", "v_q", "m_p", "v_p", "grad_q",
                                          "grad_p", "work")]
    bad += [{name: 4096 + 2} for name in ("obs", "rew", "ob2", "step", "loss")] + [dict(act=4096 + 4)]
    for kw in bad:
        for fn in entries:
            assert fn(C.byref(_fake_args(**kw)), None) == -1, kw
    for fn in entries:
        assert fn(None, None) == -1
        assert fn(C.byref(_fake_args()), C.c_void_p(4)) == -1           # a misaligned stream
    assert lib.icnn_be_ddpg_step(C.byref(_fake_args(loss=None)), None) == -1
    for fn, n_ptr in ((lib.icnn_be_ddpg_act, 2), (lib.icnn_be_ddpg_q, 3)):
        good = [4096 * (i + 1) for i in range(n_ptr)]
        for dims in ((0, 1, 5, 7), (3, 0, 5, 7), (3, 1, 0, 7), (3, 1, 5, 0), (601, 1, 5, 7), (3, 33, 5, 7), (3, 1, 601, 7),
                     (3, 1, 5, 601)):
            assert fn(*dims, *good, 4, 8192 * 4, None) == -1, dims
        assert fn(3, 1, 5, 7, *good, 0, 8192 * 4, None) == -1
        assert fn(3, 1, 5, 7, *good, 4, None, None) == -1
        assert fn(3, 1, 5, 7, *good, 4, 8192 * 4 + 2, None) == -1
        for i in range(n_ptr):
            assert fn(3, 1, 5, 7, *[None if j == i else p for j, p in enumerate(good)], 4, 8192 * 4, None) == -1
            assert fn(3, 1, 5, 7, *[p + 2 if j == i else p for j, p in enumerate(good)], 4, 8192 * 4, None) == -1


def test_init_params_ranges_and_shapes():
    dimO, dimA, l1, l2 = 17, 6, 200, 150
    params = ddpg.init_params(dimO, dimA, l1, l2, 5)
    spec = ddpg.DDPGSpec(dimO, dimA, l1, l2)
    fan = {"p": (dimO, l1, l2), "q": (dimO, l1 + dimA, l2)}
    for which, final in (("p", 3e-3), ("q", 3e-4)):
        net = params[which]
        assert [(k, v.shape) for k, v in net.items()] == ddpg.layout(spec, which)
        for i, fan_in in enumerate(fan[which], 1):
            bound = final if i == 3 else 1.0 / np.sqrt(fan_in)
            for name in ("W%d" % i, "b%d" % i):
                a = net[name]
                assert a.dtype == np.float32 and np.abs(a).max() <= bound
                if a.size >= 100:                                   # the draws fill the range: not a narrower one
                    assert np.abs(a).max() > 0.9 * bound and a.min() < 0 < a.max()
        flat = ddpg.flatten(spec, which, net)
        assert flat.shape == (ddpg.n_floats(spec, which),)
        back = ddpg.unflatten(spec, which, flat)
        assert all(np.array_equal(back[k], net[k]) for k in net)
    again = ddpg.init_params(dimO, dimA, l1, l2, 5)
    assert all(np.array_equal(again[w][k], params[w][k]) for w in "pq" for k in params[w])
    other = ddpg.init_params(dimO, dimA, l1, l2, 6)
    assert not np.array_equal(other["p"]["W1"], params["p"]["W1"])
    wide = ddpg.init_params(dimO, dimA, l1, l2, 5, final_p=None, final_q=None)
    assert np.abs(wide["q"]["W3"]).max() > 0.5 / np.sqrt(l2)


@pytest.mark.parametrize("shape", SMALL)
def test_small_shapes_have_no_ambiguous_unit(shape):
    """the precondition of the exact mask comparison: no pre-activation of the small shapes lies below its own bound"""
    fw, bound_fw, ambiguous = _reference(shape)[5], _reference(shape)[6], _reference(shape)[10]
    assert not any(a.any() for a in ambiguous.values())
    assert min((np.abs(fw[z]) / bound_fw[z]).min() for z in ("qz1", "qz2", "pz1", "pz2", "cz2")) > 8


@pytest.mark.parametrize("shape", WIDE)
def test_wide_shapes_have_few_ambiguous_units(shape):
    """at most 1 % of the units of any mask lie below their own end-to-end bound"""
    ambiguous = _reference(shape)[10]
    for k, a in ambiguous.items():
        print("ambiguous %s: %d of %d" % (k, a.sum(), a.size))
        assert a.mean() <= 0.01, k


STAGE_INPUTS = ("xa", "h2q", "q", "y", "td", "d3q", "d2q", "h1p", "h2p", "a", "h2c", "d3p", "d2p")


@pytest.mark.parametrize("shape", WIDE + [WIDEST])
def test_stage_bounds_leave_few_units_ambiguous(shape):
    """the precondition of the stage-wise mask comparison, from the reference's own activations: under one layer's rounding
    at most 1 % of a layer's units lie below their bound"""
    P, Q, _, _, mb, fw, _, d = _reference(shape)[:8]
    B = shape[0]
    dev = {"xa": np.concatenate([fw["qh1"], mb[1]], axis=1), "h2q": fw["qh2"], "h1p": fw["ph1"], "h2p": fw["ph2"], "h2c": fw["ch2"]}
    dev.update({k: fw[k] for k in ("q", "y", "td", "a")})
    dev.update({k: d[k] for k in ("d3q", "d2q", "d3p", "d2p")})
    assert set(dev) == set(STAGE_INPUTS)
    s = ref.stage_step(P, Q, mb[0], dev, B)
    assert set(s.pre) == {"qh1", "h2q", "h1p", "h2p", "h2c"}
    for k, a in s.ambiguous().items():
        print("ambiguous %s: %d of %d" % (k, a.sum(), a.size))
        assert a.mean() <= 0.01, k
    # the stages, chained through the reference's own values, restate the reference's step
    names = {"qh1": "qh1", "h2q": "qh2", "h1p": "ph1", "h2p": "ph2", "h2c": "ch2"}
    for k, want in s.want.items():
        np.testing.assert_allclose(want, d[k] if k in d else fw[names.get(k, k)], rtol=1e-12, atol=1e-14, err_msg=k)


def test_the_widest_nets_are_accepted_and_one_more_unit_is_refused():
    """WIDEST is the largest every dimension goes, its LDS fits (ddpg_fits), and one more hidden unit or action dimension is
    refused by the size entries, before any launch"""
    lib = _lib.load()
    B, dimO, dimA, l1, l2 = WIDEST
    assert (dimO, dimA, l1, l2) == (_lib.DDPG_MAX_OBS, _lib.DDPG_MAX_ACT, _lib.DDPG_MAX_HIDDEN, _lib.DDPG_MAX_HIDDEN)
    for shape in WIDE + [WIDEST]:
        assert lib.icnn_be_ddpg_work_bytes(*shape) > 0
    for bad in ((dimO, dimA, l1 + 1, l2), (dimO, dimA, l1, l2 + 1), (dimO, dimA + 1, l1, l2), (dimO + 1, dimA, l1, l2)):
        assert lib.icnn_be_ddpg_work_bytes(B, *bad) == 0, bad
        assert lib.icnn_be_ddpg_work_offsets(B, *bad, C.byref((C.c_longlong * len(_lib.DDPG_WORK))())) == -1, bad
        assert lib.icnn_be_ddpg_param_floats(*bad, C.byref(C.c_longlong()), C.byref(C.c_longlong())) == -1, bad


# ------------------------------------------------------------------------------------------------ GPU


def _trainer(shape, **kw):
    """a DDPGTrainer at `shape` holding the test's nets and minibatch"""
    B, dimO, dimA, l1, l2 = shape
    seed = SEED.get(shape, 0)
    P, Q, PT, QT = _nets(shape, seed)
    tr = ddpg.DDPGTrainer(dimO, dimA, l1, l2, batch=B, discount=DISCOUNT, **kw)
    tr.load(p=P, q=Q, target_p=PT, target_q=QT)
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


POISON = np.float32(np.frombuffer(np.uint32(0x7fc0beef).tobytes(), np.float32)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_chain_kernel_against_the_reference(shape):
    B, dimO, dimA, l1, l2 = shape
    P, Q, PT, QT, mb, fw, bound_fw, _, _, own, ambiguous = _reference(shape)
    tr = _trainer(shape)
    tr.work.view(torch.int32).fill_(0x7fc0beef)
    tr.chain()
    torch.cuda.synchronize()
    work = tr.work.cpu().numpy().view(np.uint32)
    # nothing outside the B rows of each piece is written
    written = np.zeros(work.size, bool)
    for name in _lib.DDPG_WORK[:_lib.DDPG_WORK.index("upd")]:
        v = tr.work_view(name)
        at = tr.work_offsets[name]
        written[at:at + v.numel() * (2 if name == "sq" else 1)] = True
    assert np.all(work[~written] == 0x7fc0beef) and (~written).sum() > 0
    assert not np.any(work[written] == 0x7fc0beef)
    # the forward quantities
    for name in ("a2", "y", "q", "td", "a", "qpi"):
        got = _host(tr.work_view(name))
        _within(name, got if got.shape[1] > 1 or fw[name].ndim == 2 else got[:, 0], fw[name], bound_fw[name])
    xa = _host(tr.work_view("xa"))
    assert np.array_equal(xa[:, l1:], mb[1])                       # the float64 action, rounded to float32 once
    dev_h = {"qh1": xa[:, :l1], "qh2": _host(tr.work_view("h2q")), "ph1": _host(tr.work_view("h1p")),
             "ph2": _host(tr.work_view("h2p")), "ch2": _host(tr.work_view("h2c"))}
    for k, h in dev_h.items():
        _within(k, h, fw[k], bound_fw[k])
    sq = tr.work_view("sq").cpu().numpy()
    td32 = tr.work_view("td").cpu().numpy()[:, 0].astype(np.float64)
    np.testing.assert_allclose(sq, [np.sum(td32[i:i + 16] ** 2) for i in range(0, B, 16)], rtol=17 * 2.0 ** -53, atol=0)
    # the masks: the reference's everywhere except at ambiguous units (the small shapes have none)
    dev_masks = {k: (h > 0).astype(np.float64) for k, h in dev_h.items()}
    n_ambiguous = sum(int(a.sum()) for a in ambiguous.values())
    if shape in SMALL:
        assert n_ambiguous == 0
    for k in dev_masks:
        assert np.array_equal(dev_masks[k][~ambiguous[k]], own[k][~ambiguous[k]]), k
    # the deltas against the reference backward at the device's masks
    _, _, d, bound_d, _, _ = ref.reference_step(P, Q, PT, QT, mb, DISCOUNT, masks=dev_masks)
    for name in ("d3q", "d2q", "d1q", "d3p", "d2p", "d1p"):
        _within(name, _host(tr.work_view(name)), d[name], bound_d[name])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", WIDE + [WIDEST])
def test_stages_from_the_devices_own_operands(shape):
    """Every stored layer output and delta of the chain once more, from the stored quantities it was formed from and the
    device's own parameters (ddpg_ref.stage_step): each bound holds one layer's roundings, some 1e-5 of the quantity, and stays
    sharp at the widest nets, where the end-to-end bounds say nothing.  A mask has the sign of its pre-activation wherever that
    exceeds its bound."""
    B, dimO, dimA, l1, l2 = shape
    tr = _trainer(shape)
    tr.chain()
    torch.cuda.synchronize()
    dev = {k: _host(tr.work_view(k)) for k in STAGE_INPUTS + ("d1q", "d1p", "qpi")}
    for k in ("q", "y", "td", "qpi"):
        dev[k] = dev[k][:, 0]
    s = ref.stage_step(tr.host_params("p"), tr.host_params("q"), _host(tr.obs), dev, B)
    dev["qh1"] = dev["xa"][:, :l1]
    assert np.array_equal(dev["xa"][:, l1:], _host(tr.act))
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
    B, dimO, dimA, l1, l2 = shape
    tr = _trainer(shape)
    tr.chain()
    tr.grads()
    torch.cuda.synchronize()
    gq, gp = tr.grad_q.cpu().numpy(), tr.grad_p.cpu().numpy()
    obs = _host(tr.obs)
    d = {k: _host(tr.work_view(k)) for k in ("d3q", "d2q", "d1q", "d3p", "d2p", "d1p")}
    X = (obs, _host(tr.work_view("xa")), _host(tr.work_view("h2q")), _host(tr.work_view("h1p")), _host(tr.work_view("h2p")))
    want_q, want_p = ref.weight_grads(*X, d)
    mag_q, mag_p = ref.weight_grads(*[np.abs(x) for x in X], {k: np.abs(v) for k, v in d.items()})
    n = B                                            # one chain of B fma per element
    assert np.abs(want_q).max() > 1e-4 and np.abs(want_p).max() > 1e-5
    _within("g_q", gq.astype(np.float64), want_q, n * ref.U * mag_q)
    _within("g_p", gp.astype(np.float64), want_p, n * ref.U * mag_p)
    # a second run gives the same bits
    tr.grad_q.fill_(7.0)
    tr.grad_p.fill_(7.0)
    tr.chain()
    tr.grads()
    torch.cuda.synchronize()
    assert np.array_equal(tr.grad_q.cpu().numpy().view(np.uint32), gq.view(np.uint32))
    assert np.array_equal(tr.grad_p.cpu().numpy().view(np.uint32), gp.view(np.uint32))


def _state(tr):
    return {"q": tr.theta["q"], "p": tr.theta["p"], "target_q": tr.theta["target_q"], "target_p": tr.theta["target_p"],
            "m_q": tr.m["q"], "v_q": tr.v["q"], "m_p": tr.m["p"], "v_p": tr.v["p"]}


def _snapshot(tr):
    return {k: t.cpu().numpy().copy() for k, t in _state(tr).items()}


def _expected_update(tr, before, gq, gp, t_q, t_p):
    """update32 of both nets from the state `before`, the device's gradients and the step counts after the update"""
    out = {}
    for w, g, t, lr, k in (("q", gq, t_q, tr.rate, tr.l2norm), ("p", gp, t_p, tr.prate, tr.pl2norm)):
        th, m, v, tt = ref.update32(before[w], before["m_" + w], before["v_" + w], before["target_" + w], g, t, lr, k, tr.tau)
        out.update({w: th, "m_" + w: m, "v_" + w: v, "target_" + w: tt})
    return out


def _same_bits(got, want):
    for k in want:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


# the parameter counts of these nets have every residue mod 4 (asserted below); the last has several workgroups per net
UPDATE_DIMS = [(3, 1, 5, 7), (3, 2, 5, 7), (4, 1, 5, 6), (2, 2, 3, 5), (3, 3, 5, 7), (3, 1, 5, 6), (17, 6, 200, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("tau, pl2norm", [(0.01, 0.0), (0.0, 1e-3), (1.0, 0.0), (0.3, 2e-2)])
def test_update_bit_for_bit(tau, pl2norm):
    residues = {"p": set(), "q": set()}
    for dims in UPDATE_DIMS:
        tr = ddpg.DDPGTrainer(*dims, batch=2, tau=tau, l2norm=1e-2, pl2norm=pl2norm, rate=1e-3, prate=1e-4, seed=4)
        rng = np.random.RandomState(7)
        for w in "pq":
            residues[w].add(tr.n[w] % 4)
            tr.m[w].copy_(torch.from_numpy(rng.uniform(-1e-2, 1e-2, tr.n[w]).astype(np.float32)))
            tr.v[w].copy_(torch.from_numpy(rng.uniform(0, 1e-3, tr.n[w]).astype(np.float32)))
            tr.theta["target_" + w].copy_(torch.from_numpy(rng.uniform(-1, 1, tr.n[w]).astype(np.float32)))
        gq, gp = (rng.uniform(-1, 1, tr.n[w]).astype(np.float32) for w in "qp")
        gq[::5] = 0.0
        tr.grad_q.copy_(torch.from_numpy(gq))
        tr.grad_p.copy_(torch.from_numpy(gp))
        tr.step_count.copy_(torch.tensor([3, 11, 0, 0], dtype=torch.int32))
        for t_q, t_p in ((4, 12), (5, 13)):                         # two updates: the counts advance, the ticket is re-armed
            before = _snapshot(tr)
            tr.update()
            torch.cuda.synchronize()
            _same_bits(_snapshot(tr), _expected_update(tr, before, gq, gp, t_q, t_p))
            assert tr.step_count.cpu().tolist() == [t_q, t_p, 0, 0] and tr.t == (t_q, t_p)
        if pl2norm == 0.0:                                          # a zero coefficient leaves g: m is b1 m + c1 g exactly
            f = np.float32
            assert np.array_equal(_snapshot(tr)["m_p"], f(0.9) * before["m_p"] + f(1.0 - 0.9) * gp)
    assert residues == {"p": {0, 1, 2, 3}, "q": {0, 1, 2, 3}}, residues


def _loss_bound(shape, fw_mag_td, Q, l2norm):
    """loss_q = mean td^2 + l2norm sum theta^2 / 2 in float64 from float32 td and theta, rounded once: td carries its n u M"""
    B, dimO, dimA, l1, l2 = shape
    n_td = ref.forward_counts(dimO, dimA, l1, l2)["td"]
    return (2 * n_td + 2) * ref.U * np.mean(fw_mag_td ** 2) + 2 * ref.U * l2norm * 0.5 * np.sum(ref.flat(ref.f64(Q)) ** 2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(33, 3, 1, 20, 12), SHIPPED])
def test_three_whole_steps_eager_and_captured(shape):
    B, dimO, dimA, l1, l2 = shape
    kw = dict(l2norm=1e-2, pl2norm=1e-3, rate=1e-3, prate=1e-4, tau=0.05)
    tr = _trainer(shape, **kw)
    mb = ref.batch(B, dimO, dimA, SEED[shape])
    eager = []
    for t in (1, 2, 3):
        before = _snapshot(tr)
        nets = [tr.host_params(w) for w in ("p", "q", "target_p", "target_q")]
        loss = tr.step_buffers()
        torch.cuda.synchronize()
        gq, gp = tr.grad_q.cpu().numpy(), tr.grad_p.cpu().numpy()
        after = _snapshot(tr)
        _same_bits(after, _expected_update(tr, before, gq, gp, t, t))
        assert tr.t == (t, t)
        fw = ref.step_forward(ref.Exact, *[ref.f64(n) for n in nets], *[np.asarray(x, np.float64) for x in mb[:4]], mb[4], DISCOUNT)
        mg = ref.step_forward(ref.Mag, *[ref.absnet(n) for n in nets], *[np.abs(np.asarray(x, np.float64)) for x in mb[:4]], mb[4],
                              DISCOUNT)
        want, _ = ref.losses(nets[0], ref.f64(nets[1]), fw, kw["l2norm"], 0.0)
        bound = _loss_bound(shape, mg["td"], nets[1], kw["l2norm"])
        print("loss_q %.9g, reference %.9g, bound %.3e" % (loss.item(), want, bound))
        assert abs(loss.item() - want) <= bound
        # and at its own scale: from the device's own td and theta in float64, then one rounding to float32
        td = tr.work_view("td").cpu().numpy()[:, 0].astype(np.float64)
        own = np.mean(td ** 2) + float(np.float32(kw["l2norm"])) * 0.5 * np.sum(before["q"].astype(np.float64) ** 2)
        assert abs(loss.item() - own) <= 2 * ref.U * abs(own)
        eager.append((after, loss.item()))
    assert not np.array_equal(eager[0][0]["p"], eager[2][0]["p"]) and not np.array_equal(eager[0][0]["target_q"], eager[2][0]["target_q"])
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
    assert cap.t == (3, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 17])
def test_act_and_q_equal_the_chain_bit_for_bit(B):
    for dims in [(5, 2, 16, 16), (11, 3, 33, 18), (17, 6, 200, 200)] + [s[1:] for s in WIDE + [WIDEST]]:
        tr = _trainer((B,) + dims)
        tr.chain()
        a = tr.policy(tr.obs)
        q = tr.q(tr.obs, tr.act)
        a2 = tr.policy(tr.ob2, which="target_p")
        torch.cuda.synchronize()
        assert np.abs(a.cpu().numpy()).max() > 0
        assert np.array_equal(a.cpu().numpy().view(np.uint32), tr.work_view("a").cpu().numpy().view(np.uint32))
        assert np.array_equal(a2.cpu().numpy().view(np.uint32), tr.work_view("a2").cpu().numpy().view(np.uint32))
        assert np.array_equal(q.cpu().numpy().view(np.uint32), tr.work_view("q").cpu().numpy()[:, 0].view(np.uint32))


# ---- the agent ----

EPISODE_STEPS, EPISODE_ENDS = 40, (13, 27)


def _script(dimO):
    """the scripted environment: observation t + 1 and the reward depend on the step and on the action taken"""
    rng = np.random.RandomState(11)
    base = rng.uniform(-1, 1, (EPISODE_STEPS + 1, dimO)).astype(np.float32)

    def next_obs(t, action):
        return (0.8 * base[t + 1] + 0.2 * np.float32(np.tanh(action.sum()))).astype(np.float32)

    return base, next_obs


def _agent(capture, seed=3):
    return rl_agent.DDPGAgent(5, 2, l1=16, l2=12, bsize=16, warmup=8, iters=2, rmsize=64, seed=seed, capture=capture, tau=0.05,
                              pl2norm=1e-3)


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
def test_agent_capture_on_and_off_agree():
    runs = []
    for capture in (False, True):
        agent = _agent(capture)
        actions = _run(agent, 0, EPISODE_STEPS)
        agent.memory.raise_on_error()
        assert agent.t == EPISODE_STEPS and agent.trainer.t == (2 * (EPISODE_STEPS - 8),) * 2
        assert (agent._graph is not None) == capture
        assert np.abs(actions).max() <= 1.0 and actions.dtype == np.float64 and actions.shape == (EPISODE_STEPS, 2)
        runs.append((actions, _agent_state(agent)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k].view(np.uint8), runs[1][1][k].view(np.uint8)), k
    start = _snapshot(_agent(False).trainer)
    assert not np.array_equal(start["p"], runs[0][1]["p"]) and not np.array_equal(start["target_q"], runs[0][1]["target_q"])
    # act(test=True) is the policy itself, without noise
    agent = _agent(False)
    agent.reset(_script(5)[0][0])
    want = agent.trainer.policy(torch.from_numpy(_script(5)[0][:1]).cuda()).cpu().numpy()[0]
    assert np.array_equal(agent.act(test=True), np.clip(want.astype(np.float64), -1, 1)) and not agent.noise.any()


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [False, True])
def test_agent_checkpoint_resumes_bit_for_bit(capture, tmp_path):
    whole = _agent(capture)
    want_actions = _run(whole, 0, EPISODE_STEPS)
    want = _agent_state(whole)
    cut = 25
    first = _agent(capture)
    got_head = _run(first, 0, cut)
    path = tmp_path / "ddpg.npz"
    checkpoint.save(path, first)
    if capture:                                                 # a graph captured before the load replays on the loaded state
        second = _agent(capture)
        _run(second, 0, 12)
        graph = second._graph
        assert graph is not None
    else:
        second = _agent(capture, seed=9)                        # other weights, another noise stream, another sampler seed
    checkpoint.load(path, second)
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
    tr = ddpg.DDPGTrainer(5, 2, 16, 12, batch=16, seed=1)
    checkpoint.save(tmp_path / "trainer.npz", second.trainer)
    checkpoint.load(tmp_path / "trainer.npz", tr)
    _same_bits(_snapshot(tr), _snapshot(second.trainer))
    with pytest.raises(ValueError):
        checkpoint.load(tmp_path / "trainer.npz", ddpg.DDPGTrainer(5, 2, 16, 13, batch=16))
