"""The flat-vector layout (icnn_amd/flat.py) that ddpg.py, naf.py, ff.py and fcn.py share: the round trip, the views, the two
errors with their texts, and that every module's flatten is still the concatenation in its layout's order.  CPU only."""
import numpy as np
import pytest
import torch

from icnn_amd import ddpg, fcn, ff, flat, naf

# a one-element variable between two matrices; a 4-d shape next to vectors; a single variable
LAYOUTS = {
    "scalar": [("W", (3, 2)), ("s", (1,)), ("V", (2, 5))],
    "conv": [("k.weight", (2, 3, 3, 3)), ("k.bias", (2,)), ("u.weight", (2, 1, 1, 1)), ("u.bias", (1,))],
    "single": [("b", (7,))],
}


def _params(layout, seed=0):
    rng = np.random.RandomState(seed)
    return {name: rng.standard_normal(shape).astype(np.float32) for name, shape in layout}


def _concatenated(layout, params):
    return np.concatenate([np.asarray(params[name], np.float32).reshape(-1) for name, _ in layout])


@pytest.mark.parametrize("which", sorted(LAYOUTS))
def test_round_trip(which):
    layout = LAYOUTS[which]
    p = _params(layout)
    vec = flat.flatten(layout, p)
    assert vec.dtype == np.float32 and vec.shape == (flat.n_floats(layout),)
    assert flat.n_floats(layout) == sum(int(np.prod(shape)) for _, shape in layout)
    np.testing.assert_array_equal(vec, _concatenated(layout, p))
    back = flat.unflatten(layout, vec)
    assert list(back) == [name for name, _ in layout]
    for name, shape in layout:
        assert back[name].shape == shape and back[name].dtype == np.float32
        np.testing.assert_array_equal(back[name], p[name])
    back[layout[0][0]][...] = 7.0                                # copies: the vector stays
    np.testing.assert_array_equal(vec, _concatenated(layout, p))


@pytest.mark.parametrize("which", sorted(LAYOUTS))
def test_views_alias_the_tensor(which):
    layout = LAYOUTS[which]
    p = _params(layout, 1)
    t = torch.from_numpy(flat.flatten(layout, p).copy())
    v = flat.views(layout, t)
    at = 0
    for name, shape in layout:
        assert tuple(v[name].shape) == shape
        assert v[name].data_ptr() == t.data_ptr() + 4 * at
        np.testing.assert_array_equal(v[name].numpy(), p[name])
        at += int(np.prod(shape))
    assert at == t.numel()
    last = layout[-1][0]
    v[last].fill_(3.0)                                           # through the view into the tensor, and back
    assert (t[-v[last].numel():] == 3.0).all()
    t[0] = -5.0
    assert v[layout[0][0]].reshape(-1)[0].item() == -5.0


def test_wrong_shape_error():
    layout = LAYOUTS["scalar"]
    p = _params(layout)
    p["s"] = np.zeros((1, 1), np.float32)
    with pytest.raises(ValueError) as e:
        flat.flatten(layout, p)
    assert str(e.value) == "s: shape (1, 1), expected (1,)"
    with pytest.raises(ValueError) as e:
        flat.flatten(layout, p, "q/")
    assert str(e.value) == "q/s: shape (1, 1), expected (1,)"
    t = torch.zeros(flat.n_floats(layout))
    with pytest.raises(ValueError) as e:
        flat.copy_into(t, layout, p, "target_q", "q/")
    assert str(e.value) == "q/s: shape (1, 1), expected (1,)"
    assert (t == 0).all()


def test_copy_into_and_wrong_length_error():
    layout = LAYOUTS["conv"]
    p = _params(layout, 2)
    n = flat.n_floats(layout)
    t = torch.zeros(n)
    flat.copy_into(t, layout, p, "theta")                        # a dict
    np.testing.assert_array_equal(t.numpy(), _concatenated(layout, p))
    vec = np.arange(n, dtype=np.float64)
    flat.copy_into(t, layout, vec, "theta")                      # a flat vector of another dtype
    np.testing.assert_array_equal(t.numpy(), vec.astype(np.float32))
    for bad in (np.zeros(n + 1, np.float32), np.zeros(n - 1, np.float32), np.zeros((n, 1), np.float32)):
        with pytest.raises(ValueError) as e:
            flat.copy_into(t, layout, bad, "target_v")
        assert str(e.value) == "target_v: %s values, expected %d" % (bad.shape, n)
    np.testing.assert_array_equal(t.numpy(), vec.astype(np.float32))


def _module_cases():
    d = ddpg.DDPGSpec(3, 2, 5, 4)
    a = naf.NAFSpec(3, 2, 5, 4)
    yield "ddpg/p", ddpg.layout(d, "p"), lambda p: ddpg.flatten(d, "p", p), lambda v: ddpg.unflatten(d, "p", v), ddpg.n_floats(d, "p")
    yield "ddpg/q", ddpg.layout(d, "q"), lambda p: ddpg.flatten(d, "q", p), lambda v: ddpg.unflatten(d, "q", v), ddpg.n_floats(d, "q")
    for w in naf.TRAINED:
        yield ("naf/" + w, naf.layout(a, w), lambda p, w=w: naf.flatten(a, w, p), lambda v, w=w: naf.unflatten(a, w, v),
               naf.n_floats(a, w))
    f = ff.FFSpec(5, 3, (4, 6))
    yield "ff", ff.layout(f), lambda p: ff.flatten(f, p), lambda v: ff.unflatten(f, v), ff.n_floats(f)
    c = fcn.FCNSpec(8, 8, 16)
    yield "fcn", fcn.layout(c), lambda p: fcn.flatten(c, p), lambda v: fcn.unflatten(c, v), fcn.n_floats(c)


@pytest.mark.parametrize("case", list(_module_cases()), ids=lambda c: c[0])
def test_modules_flatten_is_the_concatenation(case):
    _, layout, flatten, unflatten, n = case
    p = _params(layout, 4)
    want = _concatenated(layout, p)
    got = flatten(p)
    assert got.dtype == np.float32 and n == want.size
    np.testing.assert_array_equal(got, want)
    back = unflatten(got)
    for name, _ in layout:
        np.testing.assert_array_equal(back[name], p[name])


def test_modules_keep_their_error_texts():
    d = ddpg.DDPGSpec(3, 2, 5, 4)
    p = _params(ddpg.layout(d, "q"))
    p["b3"] = np.zeros((2,), np.float32)
    with pytest.raises(ValueError) as e:
        ddpg.flatten(d, "q", p)
    assert str(e.value) == "q/b3: shape (2,), expected (1,)"
    a = naf.NAFSpec(3, 2, 5, 4)
    p = _params(naf.layout(a, "l"))
    p["W3"] = np.zeros((4, 2), np.float32)
    with pytest.raises(ValueError) as e:
        naf.flatten(a, "l", p)
    assert str(e.value) == "l/W3: shape (4, 2), expected (4, 4)"
    f = ff.FFSpec(5, 3, (4,))
    p = _params(ff.layout(f))
    p["gamma1"] = np.zeros((5,), np.float32)
    with pytest.raises(ValueError) as e:
        ff.flatten(f, p)
    assert str(e.value) == "gamma1: shape (5,), expected (4,)"
    c = fcn.FCNSpec(8, 8, 16)
    p = _params(fcn.layout(c))
    p["up4.weight"] = np.zeros((16, 1), np.float32)
    with pytest.raises(ValueError) as e:
        fcn.flatten(c, p)
    assert str(e.value) == "up4.weight: shape (16, 1), expected (16, 1, 1, 1)"
