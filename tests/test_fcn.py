"""The FCN baseline of the completion experiment (icnn_amd/fcn.py, be_fcn.hip) against
  - tests/golden/fcn_baseline__k16_16x24.npz: outputs of the reference's own FCN class and loop (tools/gen_golden_fcn.py), and
  - tests/fcn_ref.py: the float64 restatement with derived float32 bounds (u = 2^-24), never measured from the device.
The end-to-end bounds grow through seven layers, so every launch is also checked from the device's OWN inputs, where the bound
holds one layer's roundings."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import fcn_ref as ref
from icnn_amd import _lib, checkpoint, fcn, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "fcn_baseline__k16_16x24.npz")
U = ref.U
# (k, B, H, W)
SMALL = [(16, 1, 8, 8), (16, 3, 8, 16), (32, 2, 16, 8), (48, 2, 8, 8), (16, 3, 16, 24)]
SHIPPED = (32, 70, 32, 64)
SHAPES = SMALL + [SHIPPED]
# The draws' seeds, chosen from the float64 reference alone (test_few_units_are_ambiguous prints the figures): with 7 no unit of
# the first two shapes is ambiguous (smallest |z| / bound 40.4 and 19.3) and at most 0.27 % of the other small shapes' are; at
# the shipped shape seed 7 gives 1.01 % and seed 4 gives 0.55 %.
SEED = {shape: 7 for shape in SMALL}
SEED[SHIPPED] = 4
# k = 64 takes the paths no shape above takes (four column tiles, more than 48 KB of LDS): checked per launch only
WIDEST = (64, 2, 8, 16)
SEED[WIDEST] = 7
NEW_EXPORTS = ["icnn_be_fcn_" + n for n in ("param_floats", "work_bytes", "work_offsets", "forward", "backward", "grads", "update",
                                           "step", "eval")]


@functools.lru_cache(maxsize=None)
def _draw(shape):
    k, B, H, W = shape
    return ref.draw(k, B, H, W, SEED[shape])


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """the float64 reference with end-to-end bounds, computed once and shared; nobody writes to it"""
    P, x, t = _draw(shape)
    return ref.reference(P, x, t)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    return {"theta0": {k[len("theta0/"):]: g[k] for k in g.files if k.startswith("theta0/")}, **{k: g[k] for k in g.files if "/" not in k}}


def _within(what, got, want, bound):
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: max err %.3e, %.3f of its bound (bound up to %.3e)" % (what, err.max(), ratio, bound.max()))
    assert (err <= bound).all(), "%s: %.3f of its bound" % (what, ratio)
    return ratio


# ----------------------------------------------------------------------------------------------------------------- CPU tests
def test_reference_against_the_fixture():
    """yhat, loss and the flat gradient of the REFERENCE ITSELF (float32, CPU) lie within the derived end-to-end bounds of the
    float64 restatement; the restatement's gradient equals torch.autograd's"""
    g = _golden()
    assert os.path.getsize(GOLDEN) <= 250 * 1024
    assert g["x"].shape == g["t"].shape == g["yhat"].shape == (3, 16, 24) and g["losses"].shape == (3,)
    assert g["grad1"].shape == g["grad2"].shape == g["grad3"].shape == g["theta3"].shape == (11777,)
    r = ref.reference(g["theta0"], g["x"], g["t"])
    _within("yhat", g["yhat"], r["yhat"], r["e_yhat"])
    assert 1.7e-3 < r["e_yhat"].max() < 1.9e-3              # the bound's own size at this shape: 1.8e-3
    assert abs(float(g["losses"][0]) - r["loss"]) <= r["e_loss"]
    _within("grad", g["grad1"], r["grad"], r["e_grad"])
    want = ref.autograd_grad(g["theta0"], g["x"], g["t"])
    np.testing.assert_allclose(r["grad"], want, rtol=1e-9, atol=1e-300)
    assert fcn.flatten(fcn.FCNSpec(16, 24, 16), g["theta0"]).shape == (11777,)


def test_conv1_reads_only_even_rows_and_columns():
    """the reference's behaviour, kept: d yhat / d x is exactly 0 at every odd row or column"""
    P, x, t = _draw(SMALL[4])
    gx = ref.grad_x(P, x, t)
    assert np.abs(gx[:, ::2, ::2]).max() > 0
    assert (gx[:, 1::2, :] == 0).all() and (gx[:, :, 1::2] == 0).all()


def test_adam64_against_the_fixture_and_torch():
    g = _golden()
    # (a) the fixture's loop: adam64 from theta_0 on the reference's OWN three gradients against its theta after three steps,
    # within the sum of the per-step tolerances
    spec = fcn.FCNSpec(16, 24, 16)
    theta, m, v = fcn.flatten(spec, g["theta0"]).astype(np.float64), 0.0, 0.0
    tol = np.zeros_like(theta)
    for t in (1, 2, 3):
        new, m, v = ref.adam64(theta, m, v, g["grad%d" % t], t)
        tol += ref.adam_tol(theta, new)
        theta = new
    ratio = (np.abs(g["theta3"] - theta) / tol).max()
    print("fixture, theta after 3 steps from the reference's gradients: %.3f of the summed per-step tolerance" % ratio)
    assert ratio <= 1.0
    # (b) torch.optim.Adam on CPU float32, five steps on gradients whose magnitudes span 1e-8 ... 1, step by step from torch's
    # own state; TF's form (eps inside the correction) must leave the same tolerance by more than 10x somewhere
    rng = np.random.RandomState(3)
    n = 4096
    p = torch.nn.Parameter(torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32)))
    opt = torch.optim.Adam([p], lr=1e-4)
    mag = 10.0 ** rng.uniform(-8, 0, n)
    worst_tf = 0.0
    for t in range(1, 6):
        grad = (mag * rng.uniform(-1, 1, n)).astype(np.float32)
        before = p.detach().numpy().copy()
        st = opt.state[p]
        m0 = st["exp_avg"].numpy().copy() if st else np.zeros(n, np.float32)
        v0 = st["exp_avg_sq"].numpy().copy() if st else np.zeros(n, np.float32)
        p.grad = torch.from_numpy(grad)
        opt.step()
        after = p.detach().numpy()
        want, m1, v1 = ref.adam64(before, m0, v0, grad, t)
        tol = ref.adam_tol(before, want)
        assert (np.abs(after - want) <= tol).all(), "step %d: %.3f" % (t, (np.abs(after - want) / tol).max())
        tf = before - train.adam_lr_t(1e-4, 0.9, 0.999, t) * m1 / (np.sqrt(v1) + 1e-8)
        worst_tf = max(worst_tf, float((np.abs(tf - want) / tol).max()))
    print("TF's form leaves the tolerance by %.1fx" % worst_tf)
    assert worst_tf > 10.0


def test_new_exports_declared_and_abi():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"ICNN_BE_API\s+(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.icnn_be_abi_version() == 12 and "#define ICNN_BE_ABI_VERSION 12" in header
    assert lib.icnn_be_struct_size(18) == C.sizeof(_lib.FcnArgs) > 0
    assert lib.icnn_be_struct_size(17) == 0 and lib.icnn_be_struct_size(19) == 0
    for name, value in (("MAX_K", _lib.FCN_MAX_K), ("MAX_HW", _lib.FCN_MAX_HW), ("MAX_BATCH", _lib.FCN_MAX_BATCH),
                        ("MAX_EVAL_BATCH", _lib.FCN_MAX_EVAL_BATCH), ("STEP_INTS", _lib.FCN_STEP_INTS),
                        ("WORK_PIECES", len(_lib.FCN_WORK))):
        assert "#define ICNN_BE_FCN_%s %d" % (name, value) in header
    for piece, first in (("H", 0), ("DY", 6), ("DZ", 7), ("WPART", 13), ("LPART", 14), ("CTL", 15)):
        assert re.search(r"#define ICNN_BE_FCN_W_%s %d\b" % (piece, first), header), piece
        assert _lib.FCN_WORK[first].rstrip("0") == piece.lower()
    assert (_lib.FCN_MAX_K, _lib.FCN_MAX_HW, _lib.FCN_MAX_BATCH) == (64, 128, 128)


def test_param_floats_and_layout():
    lib = _lib.load()
    for k, want in ((16, 11777), (32, 46593), (48, 45 * 48 * 48 + 16 * 48 + 1), (64, 45 * 64 * 64 + 16 * 64 + 1)):
        n = C.c_longlong()
        assert lib.icnn_be_fcn_param_floats(64, 32, k, C.byref(n)) == 0
        assert n.value == want == fcn.n_floats(fcn.FCNSpec(64, 32, k))
    spec = fcn.FCNSpec(8, 16, 16)
    assert fcn.layout(spec) == [
        ("conv1.weight", (16, 1, 3, 3)), ("conv1.bias", (16,)), ("conv2.weight", (16, 16, 3, 3)), ("conv2.bias", (16,)),
        ("conv3.weight", (16, 16, 3, 3)), ("conv3.bias", (16,)), ("up1.weight", (16, 16, 3, 3)), ("up1.bias", (16,)),
        ("up2.weight", (16, 16, 3, 3)), ("up2.bias", (16,)), ("up3.weight", (16, 16, 3, 3)), ("up3.bias", (16,)),
        ("up4.weight", (16, 1, 1, 1)), ("up4.bias", (1,))]
    assert [n for n, _ in fcn.layout(spec)] == list(_golden()["theta0"])        # torch's own order of named_parameters()
    assert fcn.olivetti_fcn_spec() == fcn.FCNSpec(64, 32, 32)
    for k, B, H, W in SHAPES + [(64, 128, 128, 128), (16, 1000, 8, 8)]:
        off = (C.c_longlong * len(_lib.FCN_WORK))()
        assert lib.icnn_be_fcn_work_offsets(B, H, W, k, C.byref(off)) == 0
        off = list(off)
        assert off[0] == 0 and all(b > a for a, b in zip(off, off[1:])) and all(o % 4 == 0 for o in off)
        for i, div in enumerate((2, 4, 8, 4, 2, 1)):
            for base in (0, 7):
                assert off[base + i + 1] - off[base + i] >= B * (H // div) * (W // div) * k
        assert off[7] - off[6] >= B * H * W
        assert lib.icnn_be_fcn_work_bytes(B, H, W, k) >= 4 * off[-1] + 16


BAD_SIZES = [(0, 8, 16), (4, 8, 16), (12, 8, 16), (136, 8, 16), (8, 0, 16), (8, 20, 16), (8, 136, 16), (8, 8, 0), (8, 8, 8), (8, 8, 24),
             (8, 8, 80), (-8, 8, 16)]


def test_sizes_out_of_range_are_refused():
    lib = _lib.load()
    for H, W, k in BAD_SIZES:
        assert lib.icnn_be_fcn_work_bytes(4, H, W, k) == 0, (H, W, k)
        assert lib.icnn_be_fcn_param_floats(H, W, k, C.byref(C.c_longlong())) == -1
        assert lib.icnn_be_fcn_work_offsets(4, H, W, k, C.byref((C.c_longlong * len(_lib.FCN_WORK))())) == -1
    assert lib.icnn_be_fcn_work_bytes(0, 8, 8, 16) == 0 and lib.icnn_be_fcn_work_bytes(-2, 8, 8, 16) == 0
    assert lib.icnn_be_fcn_work_bytes(_lib.FCN_MAX_EVAL_BATCH + 1, 8, 8, 16) == 0
    assert lib.icnn_be_fcn_work_bytes(1, 8, 8, 16) > 0 and lib.icnn_be_fcn_work_bytes(1000, 8, 8, 16) > 0       # evaluation
    assert lib.icnn_be_fcn_param_floats(8, 8, 16, None) == -1
    assert lib.icnn_be_fcn_work_offsets(4, 8, 8, 16, None) == -1
    with pytest.raises(ValueError):
        fcn.FCNModel(fcn.FCNSpec(8, 8, 24), device="cpu")


POINTERS = ["x", "t", "theta", "m", "v", "grad", "step", "loss", "yhat", "work"]


def _fake_args(**kw):
    """a descriptor of pointers that are never followed: every entry must refuse it before a launch"""
    a = _lib.FcnArgs()
    a.batch, a.H, a.W, a.k = 4, 8, 16, 16
    for i, name in enumerate(POINTERS):
        setattr(a, name, 4096 * (i + 1))
    a.lr, a.beta1, a.beta2, a.eps, a.pixel_scale = 1e-4, 0.9, 0.999, 1e-8, 255.0
    for k, val in kw.items():
        setattr(a, k, val)
    return a


def test_invalid_arguments_are_refused_before_a_launch():
    lib = _lib.load()
    entries = {n: getattr(lib, "icnn_be_fcn_" + n) for n in ("forward", "backward", "grads", "update", "step", "eval")}
    entries["predict"] = lambda a, s: lib.icnn_be_fcn_forward(C.byref(_with_t_none(a)), s)
    everywhere = [dict(batch=0), dict(batch=-3), dict(batch=_lib.FCN_MAX_EVAL_BATCH + 1)]
    everywhere += [dict(H=H, W=W, k=k) for H, W, k in BAD_SIZES]
    for kw in everywhere:
        for name, fn in entries.items():
            assert fn(C.byref(_fake_args(**kw)), None) == -1, (name, kw)
    for name, fn in entries.items():
        if name != "predict":
            assert fn(None, None) == -1
        assert fn(C.byref(_fake_args()), C.c_void_p(4)) == -1, name              # a misaligned stream
    for name in ("forward", "backward", "grads", "step"):                       # the entries that train: batch <= 128
        assert entries[name](C.byref(_fake_args(batch=_lib.FCN_MAX_BATCH + 1)), None) == -1, name
    # what each entry needs (the descriptor is never followed: a refusal is all that can be observed)
    needs = {"x": ("forward", "predict", "grads", "step", "eval"), "t": ("step", "eval"),
             "theta": ("forward", "predict", "backward", "update", "step", "eval"),
             "yhat": ("forward", "predict", "step", "eval"), "loss": ("forward", "step", "eval"),
             "work": ("forward", "predict", "backward", "grads", "step", "eval"), "grad": ("grads", "update", "step"),
             "m": ("update", "step"), "v": ("update", "step"), "step": ("update", "step")}
    for ptr, who in needs.items():
        for name in who:
            assert entries[name](C.byref(_fake_args(**{ptr: None})), None) == -1, (name, ptr)
            assert entries[name](C.byref(_fake_args(**{ptr: 4096 * 40 + 2})), None) == -1, (name, ptr)
    for ptr in ("theta", "m", "v", "grad", "work"):                             # 4- but not 16-byte aligned
        for name in needs[ptr]:
            assert entries[name](C.byref(_fake_args(**{ptr: 4096 * 40 + 4})), None) == -1, (name, ptr)
    for kw in (dict(beta1=1.0), dict(beta2=-0.1), dict(eps=0.0), dict(lr=float("nan")), dict(lr=float("inf"))):
        for name in ("update", "step"):
            assert entries[name](C.byref(_fake_args(**kw)), None) == -1, (name, kw)
    for kw in (dict(pixel_scale=0.0), dict(pixel_scale=float("nan"))):
        for name in ("forward", "step", "eval"):
            assert entries[name](C.byref(_fake_args(**kw)), None) == -1, (name, kw)


def _with_t_none(ref_to_args):
    a = ref_to_args._obj
    a.t = None
    return a


def test_init_params_ranges_and_determinism():
    spec = fcn.FCNSpec(16, 24, 32)
    P, Q, R = fcn.init_params(spec, 4), fcn.init_params(spec, 4), fcn.init_params(spec, 5)
    assert list(P) == [n for n, _ in fcn.layout(spec)]
    # torch's fan-in: weight.size(1) kh kw -- the transposed convolutions count their output channels, up4 (to one channel) 1
    fan = {"conv1": 9, "conv2": 288, "conv3": 288, "up1": 288, "up2": 288, "up3": 288, "up4": 1}
    for name, shape in fcn.layout(spec):
        a, r = P[name], 1.0 / np.sqrt(fan[name.split(".")[0]])
        assert a.dtype == np.float32 and a.shape == shape
        assert np.array_equal(a, Q[name]) and not np.array_equal(a, R[name])
        assert np.abs(a).max() <= r
        if a.size >= 16:
            assert np.abs(a).max() > 0.8 * r and a.min() < 0 < a.max()
    assert fcn.fan_in("up1.weight", (16, 32, 3, 3)) == 288 and fcn.fan_in("conv2.weight", (16, 32, 3, 3)) == 288


def test_flatten_round_trip_with_torch_names():
    g = _golden()
    spec = fcn.FCNSpec(16, 24, 16)
    flat = fcn.flatten(spec, g["theta0"])
    assert np.array_equal(flat, np.concatenate([g["theta0"][n].reshape(-1) for n in g["theta0"]]))
    back = fcn.unflatten(spec, flat)
    assert all(np.array_equal(back[n], g["theta0"][n]) for n in g["theta0"])
    bad = dict(g["theta0"])
    bad["up1.weight"] = bad["up1.weight"][:, :8]
    with pytest.raises(ValueError):
        fcn.flatten(spec, bad)


@pytest.mark.parametrize("shape", SHAPES)
def test_few_units_are_ambiguous(shape):
    """from the reference alone: a ReLU unit is end-to-end ambiguous where |z| < its end-to-end bound.  None at the first two
    shapes; at most 1 % at the others (up4 has no ReLU and is not counted)"""
    P, x, _ = _draw(shape)
    r = ref.reference(P, x)
    amb = sum(int((np.abs(z) < e).sum()) for z, e in zip(r["z"], r["e_z"]))
    units = sum(z.size for z in r["z"])
    nz = [np.abs(z)[z != 0] / e[z != 0] for z, e in zip(r["z"], r["e_z"])]
    print("%s: %d of %d units ambiguous (%.3f %%); smallest |z| / bound %.3g; bound of yhat %.3g"
          % (shape, amb, units, 100.0 * amb / units, min(a.min() for a in nz), r["e_yhat"].max()))
    if shape in SMALL[:2]:
        assert amb == 0
    assert amb <= 0.01 * units


# ----------------------------------------------------------------------------------------------------------------- GPU tests
def _trainer(shape, P=None, lr=1e-4, eval_batch=None, data=True):
    k, B, H, W = shape
    params, x, t = _draw(shape)
    model = fcn.FCNModel(fcn.FCNSpec(H, W, k), params=params if P is None else P)
    tr = fcn.FCNTrainer(model, B, lr=lr, eval_batch=eval_batch)
    if data:
        tr.x.copy_(torch.from_numpy(x).view(B, H, W, 1))
        tr.t.copy_(torch.from_numpy(t).view(B, H * W))
    return tr


def _host(t):
    return t.detach().cpu().numpy().copy()


def _snapshot(tr):
    return {"theta": _host(tr.model.theta), "m": _host(tr.m["fcn"]), "v": _host(tr.v["fcn"]), "step": _host(tr.step_count)}


def _same_bits(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


IMAGES = ["h%d" % i for i in range(6)] + ["dy"] + ["dz%d" % i for i in range(6)]
SENTINEL = np.float32(-1234.5)


def _fill_gaps(tr):
    """a sentinel in everything of the workspace behind the logical end of a piece that holds images, up to the next piece,
    and in the unused control words; returns the mask of those floats"""
    gaps = torch.zeros(tr.work.numel(), dtype=torch.bool)
    order = sorted(tr.work_offsets.values()) + [tr.work.numel()]
    for name in IMAGES:
        at = tr.work_offsets[name]
        gaps[at + int(np.prod(tr.piece_shape(name, tr.batch))):order[order.index(at) + 1]] = True
    gaps[tr.work_offsets["ctl"] + 2:] = True
    tr.work[gaps.to(tr.device)] = float(SENTINEL)
    return gaps.numpy()


@functools.lru_cache(maxsize=None)
def _device_run(shape):
    """forward, backward, grads once on the shape's draw: host copies of every piece, shared by the tests below"""
    tr = _trainer(shape)
    gaps = _fill_gaps(tr)
    tr.forward()
    tr.backward()
    tr.grads()
    torch.cuda.synchronize()
    out = {name: _host(tr.work_view(name)) for name in IMAGES}
    out.update(yhat=_host(tr.yhat).reshape(shape[1], shape[2], shape[3]), loss=float(tr.loss.item()), grad=_host(tr.grad),
               work=_host(tr.work), gaps=gaps, ctl=_host(tr.work_view("ctl")).view(np.int32))
    tr.grads()
    torch.cuda.synchronize()
    out["grad_again"] = _host(tr.grad)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + [WIDEST])
def test_every_launch_from_the_devices_own_inputs(shape):
    """each layer's forward from the device's stored previous activation, each data gradient from the device's own incoming
    delta and stored mask, each weight gradient against the float64 X^T Delta of the device's own X and Delta: one launch's
    roundings.  A ReLU mask equals the reference's wherever the reference's pre-activation is at least its bound."""
    k, B, H, W = shape
    P, x, t = _draw(shape)
    d = _device_run(shape)
    P64 = ref.params64(P)
    t64 = ref.t64
    assert (d["work"][d["gaps"]] == SENTINEL).all()                   # nothing outside the pieces' rows is written
    assert d["ctl"][0] == 0                                         # the ticket re-armed
    hs = [t64(x).reshape(B, 1, H, W)] + [t64(ref.nchw(d["h%d" % i])) for i in range(6)]
    deltas = [t64(ref.nchw(d["dz%d" % i])) for i in range(6)] + [t64(d["dy"]).reshape(B, 1, H, W)]
    for i, name in enumerate(ref.LAYERS):
        Wt, b = P64[name + ".weight"], P64[name + ".bias"].view(1, -1, 1, 1)
        K = ref.terms(name, hs[i].shape[1])
        z = (ref.op(name, hs[i], Wt) + b).numpy()
        bound = ((K + 1) * U * (ref.op(name, hs[i].abs(), Wt.abs()) + b.abs())).numpy()
        if name == "up4":
            _within("yhat from the device's h5", d["yhat"], z[:, 0], bound[:, 0])
            break
        got = hs[i + 1].numpy()
        _within("h%d from the device's input" % i, got, np.maximum(z, 0), bound)
        sure = np.abs(z) >= bound
        assert ((got > 0) == (z > 0))[sure].all(), "mask of h%d" % i
    N = B * H * W
    diff = d["yhat"].astype(np.float64) - t
    loss = (255.0 ** 2 * diff ** 2).mean()
    print("loss %.9g against the float64 sum over the device's yhat %.9g" % (d["loss"], loss))
    assert abs(d["loss"] - loss) <= 7 * U * loss
    dy = 2 * 255.0 ** 2 * diff / N
    _within("dy from the device's yhat", d["dy"], dy, 5 * U * np.abs(dy) + 1e-40)
    for i in range(5, -1, -1):
        name = ref.LAYERS[i + 1]
        Wt = P64[name + ".weight"]
        Kt = ref.terms_T(name, deltas[i + 1].shape[1])
        dh = ref.op_T(name, deltas[i + 1], Wt, hs[i + 1]).numpy()
        bound = ((Kt + 1) * U * ref.op_T(name, deltas[i + 1].abs(), Wt.abs(), hs[i + 1])).numpy()
        _within("dz%d from the device's delta and mask" % i, deltas[i].numpy(), dh * (hs[i + 1].numpy() > 0), bound + 1e-40)
    want, bound = {}, {}
    for i, name in enumerate(ref.LAYERS):
        Wt, hin, dl = P64[name + ".weight"], hs[i], deltas[i]
        T, Tb = ref.contraction(name, hin, dl), dl[:, 0].numel()
        want[name + ".weight"] = ref.op_W(name, hin, dl, Wt).numpy()
        bound[name + ".weight"] = ((T + 1) * U * ref.op_W(name, hin.abs(), dl.abs(), Wt)).numpy()
        want[name + ".bias"] = dl.sum((0, 2, 3)).numpy()
        bound[name + ".bias"] = ((Tb + 1) * U * dl.abs().sum((0, 2, 3))).numpy()
    spec = fcn.FCNSpec(H, W, k)
    got = fcn.unflatten(spec, d["grad"])
    for name in want:
        _within("grad of %s from the device's X and Delta" % name, got[name], want[name], bound[name] + 1e-40)
    # same bits on a second run
    assert np.array_equal(d["grad"].view(np.uint32), d["grad_again"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL)
def test_every_piece_end_to_end(shape):
    d, r = _device_run(shape), _reference(shape)
    for i in range(6):
        _within("h%d" % i, ref.nchw(d["h%d" % i]), r["h"][i], r["e_h"][i])
    _within("yhat", d["yhat"], r["yhat"], r["e_yhat"])
    assert abs(d["loss"] - r["loss"]) <= r["e_loss"]
    _within("dy", d["dy"], r["dy"], r["e_dy"])
    for i in range(6):
        _within("dz%d" % i, ref.nchw(d["dz%d" % i]), r["dz"][i], r["e_dz"][i] + 1e-40)
    _within("grad", d["grad"], r["grad"], r["e_grad"] + 1e-40)


@pytest.mark.gpu
def test_shipped_shape_yhat_against_the_cpu_float32_error():
    """at the shipped shape the end-to-end bound is vacuous, so the yardstick is the max-norm error of a float32 CPU evaluation
    (torch's own kernels, the arithmetic the reference runs on) against the same float64: the device may err 4 x that at most --
    both are float32 sums of the same terms in different orders, the maximum taken over 143 360 elements"""
    import torch.nn.functional as F
    P, x, _ = _draw(SHIPPED)
    r = ref.reference(P, x)
    h = torch.from_numpy(x).unsqueeze(1)
    for name in ref.LAYERS:
        W, b = torch.from_numpy(P[name + ".weight"]), torch.from_numpy(P[name + ".bias"])
        h = ref.op(name, h, W) + b.view(1, -1, 1, 1)
        h = h if name == "up4" else F.relu(h)
    cpu_err = np.abs(h.numpy()[:, 0].astype(np.float64) - r["yhat"]).max()
    dev_err = np.abs(_device_run(SHIPPED)["yhat"].astype(np.float64) - r["yhat"]).max()
    print("yhat at %s: device %.3e, float32 CPU %.3e, ratio %.3f; end-to-end bound %.3e" % (SHIPPED, dev_err, cpu_err, dev_err / cpu_err,
                                                                                        r["e_yhat"].max()))
    assert dev_err <= 4 * cpu_err


def _check_update(before, after, grad, t, lr):
    want, m, v = ref.adam64(before["theta"], before["m"], before["v"], grad, t, lr=lr)
    tol = ref.adam_tol(before["theta"], want)
    ratio = (np.abs(after["theta"] - want) / tol).max()
    print("update %d: theta %.3f of its tolerance" % (t, ratio))
    assert ratio <= 1.0
    # m: a difference, a product and a sum of float32 over |m| + |g|; v: positive terms alone
    assert (np.abs(after["m"] - m) <= 4 * U * (np.abs(before["m"]) + np.abs(grad)) + 1e-40).all()
    assert (np.abs(after["v"] - v) <= 4 * U * v + 1e-40).all()
    assert after["step"].tolist() == [t, 0, 0, 0]


@pytest.mark.gpu
def test_the_fixture_on_the_device():
    """from the fixture's theta_0, x, t: yhat, loss and gradient within the bounds the CPU test applies to the reference itself.
    The update is held to what the CPU test holds the reference to: every step against adam64 on the DEVICE'S OWN gradient of
    that step within 2 u |theta| + 16 u |delta theta|, and theta after the three steps against adam64 driven from theta_0 by the
    device's three gradients within the sum of the per-step tolerances."""
    g = _golden()
    shape = (16, 3, 16, 24)
    tr = _trainer(shape, P=g["theta0"], data=False)
    r = ref.reference(g["theta0"], g["x"], g["t"])
    theta, m, v = fcn.flatten(tr.spec, g["theta0"]).astype(np.float64), 0.0, 0.0
    tol = np.zeros_like(theta)
    for t in (1, 2, 3):
        before = _snapshot(tr)
        loss = tr.step(g["x"], g["t"].reshape(3, -1)).item()
        torch.cuda.synchronize()
        grad = _host(tr.grad)
        if t == 1:
            _within("yhat", _host(tr.yhat).reshape(3, 16, 24), r["yhat"], r["e_yhat"])
            assert abs(loss - r["loss"]) <= r["e_loss"]
            _within("grad", grad, r["grad"], r["e_grad"])
        _check_update(before, _snapshot(tr), grad, t, tr.lr)
        new, m, v = ref.adam64(theta, m, v, grad, t)
        tol += ref.adam_tol(theta, new)
        theta = new
    got = _host(tr.model.theta)
    ratio = (np.abs(got - theta) / tol).max()
    print("theta after 3 steps from the device's gradients: %.3f of the summed per-step tolerance" % ratio)
    assert ratio <= 1.0
    assert not np.array_equal(got, fcn.flatten(tr.spec, g["theta0"])) and tr.t_steps == 3


@pytest.mark.gpu
def test_update_against_adam64():
    """the update alone on gradients whose magnitudes span 1e-8 ... 1: within 2 u |theta| + 16 u |delta theta| per step, and
    exactly one step count that advances by one.  The entry takes the parameter count from k, 45 k^2 + 16 k + 1, which is 1 mod
    4 for every k, and the kernel has no vector path: other residues cannot be asked for."""
    tr = _trainer(SMALL[0])
    rng = np.random.RandomState(8)
    for t in range(1, 6):
        grad = (10.0 ** rng.uniform(-8, 0, tr.model.n) * rng.uniform(-1, 1, tr.model.n)).astype(np.float32)
        tr.grad.copy_(torch.from_numpy(grad))
        before = _snapshot(tr)
        tr.update()
        torch.cuda.synchronize()
        _check_update(before, _snapshot(tr), grad, t, tr.lr)


@pytest.mark.gpu
@pytest.mark.parametrize("E", [1, 33, 50])
def test_evaluate_and_predict(E):
    shape = SMALL[1]
    k, B, H, W = shape
    rng = np.random.RandomState(40 + E)
    xe, te = rng.uniform(0, 1, (E, H, W)).astype(np.float32), rng.uniform(0, 1, (E, H * W)).astype(np.float32)
    tr = _trainer(shape, eval_batch=E)
    tr.step()
    torch.cuda.synchronize()
    before, held = _snapshot(tr), (_host(tr.yhat), _host(tr.loss), _host(tr.grad), _host(tr.work))
    loss = tr.evaluate(xe, te)
    torch.cuda.synchronize()
    _same_bits(_snapshot(tr), before)                              # theta, m, v and the step count unwritten
    for a, b in zip(held, (_host(tr.yhat), _host(tr.loss), _host(tr.grad), _host(tr.work))):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    y = _host(tr.y_eval)
    want = (255.0 ** 2 * (y.astype(np.float64) - te) ** 2).mean()
    assert abs(loss.item() - want) <= 7 * U * want
    r = ref.reference(tr.host_params(), xe)
    _within("y_eval", y.reshape(E, H, W), r["yhat"], r["e_yhat"])
    # row j is bit-equal to the batch of one, and predict() (no targets) gives the same bits
    one = fcn.FCNTrainer(tr.model, 1, eval_batch=1)
    for j in sorted({0, E // 2, E - 1}):
        one.evaluate(xe[j:j + 1], te[j:j + 1])
        assert np.array_equal(_host(one.y_eval)[0].view(np.uint32), y[j].view(np.uint32)), j
    pred = tr.model.predict(torch.from_numpy(xe).to(tr.device))
    assert np.array_equal(_host(pred).view(np.uint32), y.view(np.uint32))
    _same_bits(_snapshot(tr), before)
    with pytest.raises(ValueError):
        _trainer(shape).evaluate()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SMALL[1], SMALL[3]])
def test_three_whole_steps_eager_and_captured(shape):
    k, B, H, W = shape
    _, x, t = _draw(shape)
    tr = _trainer(shape)
    eager = []
    for step in (1, 2, 3):
        before = _snapshot(tr)
        loss = tr.step().item()
        torch.cuda.synchronize()
        after = _snapshot(tr)
        # the reference at the weights the step began with, stepped with the device's masks
        masks = [ref.nchw(_host(tr.work_view("h%d" % i))) > 0 for i in range(6)]
        r = ref.reference(fcn.unflatten(tr.spec, before["theta"]), x, t, masks=masks)
        assert abs(loss - r["loss"]) <= r["e_loss"]
        _within("step %d: yhat" % step, _host(tr.yhat).reshape(B, H, W), r["yhat"], r["e_yhat"])
        grad = _host(tr.grad)
        _within("step %d: grad" % step, grad, r["grad"], r["e_grad"] + 1e-40)
        _check_update(before, after, grad, step, tr.lr)
        eager.append((after, loss, _host(tr.yhat)))
    assert not np.array_equal(eager[0][0]["theta"], eager[2][0]["theta"])
    # a captured step replayed three times: a warm-up step outside the graph, undone, then the capture
    cap = _trainer(shape)
    cap.step()
    cap.load(_draw(shape)[0], reset=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cap.step().clone()
    for after, loss, yhat in eager:
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(_snapshot(cap), after)
        assert np.float32(out.item()).view(np.uint32) == np.float32(loss).view(np.uint32)
        assert np.array_equal(_host(cap.yhat).view(np.uint32), yhat.view(np.uint32))
    assert cap.t_steps == 3


@pytest.mark.gpu
def test_epoch_runner_equals_eager_steps():
    """eager + capture + replay runs of an EpochRunner against the same count of hand-made eager iterations"""
    shape, steps = SMALL[1], 3
    k, B, H, W = shape
    rng = np.random.RandomState(5)
    X, Y = rng.uniform(0, 1, (40, H, W, 1)).astype(np.float32), rng.uniform(0, 1, (40, H * W)).astype(np.float32)
    a, b = _trainer(shape, data=False), _trainer(shape, data=False)
    da, db = train.DeviceDataset((X, Y), seed=9), train.DeviceDataset((X, Y), seed=9)
    log = train.StepLog([("loss", a.loss)], 64)
    runner = train.EpochRunner(a, da, steps, log=log)
    for _ in range(3):                                             # eager, capture + replay, replay
        runner.run()
    losses = []
    for _ in range(3 * steps):
        db.draw_into(b.x, b.t)
        losses.append(b.step().item())
    torch.cuda.synchronize()
    _same_bits(_snapshot(a), _snapshot(b))
    assert a.t_steps == b.t_steps == 3 * steps and da.draws == db.draws == 3 * steps
    got = log.read()["loss"]
    assert np.array_equal(got.astype(np.float32).view(np.uint32), np.asarray(losses, np.float32).view(np.uint32))


@pytest.mark.gpu
def test_checkpoint_resumes_bit_for_bit(tmp_path):
    shape = SMALL[1]
    path = str(tmp_path / "fcn.npz")
    whole, first = _trainer(shape), _trainer(shape)
    for _ in range(4):
        whole.step()
    for _ in range(2):
        first.step()
    checkpoint.save(path, first)
    second = _trainer(shape, P=fcn.init_params(first.spec, 77))    # other weights and moments: all overwritten
    second.step()
    ptr = second.model.theta.data_ptr()
    checkpoint.load(path, second)
    assert second.model.theta.data_ptr() == ptr and second.t_steps == 2
    for _ in range(2):
        second.step()
    torch.cuda.synchronize()
    _same_bits(_snapshot(second), _snapshot(whole))
    assert np.array_equal(_host(second.loss).view(np.uint32), _host(whole.loss).view(np.uint32))
    with pytest.raises(ValueError):
        checkpoint.load(path, _trainer(SMALL[0]))


LR_FALLS = 1e-3


@functools.lru_cache(maxsize=None)
def _losses64(steps):
    shape = SMALL[1]
    P, x, t = _draw(shape)
    spec = fcn.FCNSpec(shape[2], shape[3], shape[0])
    theta, m, v, out = fcn.flatten(spec, P).astype(np.float64), 0.0, 0.0, []
    for s in range(1, steps + 2):
        r = ref.reference(fcn.unflatten(spec, theta), x, t)
        out.append(r["loss"])
        theta, m, v = ref.adam64(theta, m, v, r["grad"], s, lr=LR_FALLS)
    return out


def test_the_references_loss_falls_strictly():
    losses = _losses64(30)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


@pytest.mark.gpu
def test_the_loss_falls():
    """30 device steps on one fixed batch at (16, 3, 8, 16) with lr 1e-3 end below the float64 reference's loss after 15; the
    reference's own losses fall strictly over those 30 steps (asserted first)"""
    losses = _losses64(30)
    assert all(b < a for a, b in zip(losses, losses[1:]))
    tr = _trainer(SMALL[1], lr=LR_FALLS)
    first = tr.step().item()
    for _ in range(29):
        tr.step()
    tr.forward()                                                   # the loss at the weights 30 steps left
    torch.cuda.synchronize()
    print("device: %.6g -> %.6g after 30 steps; float64 reference after 15: %.6g, after 30: %.6g" % (first, tr.loss.item(), losses[15],
                                                                                                  losses[30]))
    assert tr.loss.item() < losses[15]
