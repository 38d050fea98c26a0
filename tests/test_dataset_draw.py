"""The minibatch draw and the step log on the device (icnn_be_dataset_draw, icnn_be_log_row, be_train_data.hip;
train.DeviceDataset, train.StepLog) against tests/dataset_ref.py: indices with array_equal, gathered rows with
torch.equal against X[idx], at every row width, batch size and set size at which the kernel takes another path or a grid
tail, with the draw counter through eager launches, a replayed graph and reset()."""
import numpy as np
import pytest
import torch

import dataset_ref as ref

pytestmark = pytest.mark.gpu

SEEDS = (0, (0x9e3779b9 << 32) | 12345)      # the second has bits above 2^32: the key's high word
FILL = -7.0
SPARE = 3                                    # rows of every destination behind the batch: they must stay FILL


def _array(rng, n_rows, width, dtype):
    """distinct values in every element, so that a row copied from the wrong place or in the wrong order shows"""
    a = rng.permutation(n_rows * width).reshape(n_rows, width).astype(np.float64) + 0.25
    return torch.from_numpy(a.astype(dtype))


def _check_draws(shapes, n_rows, batch, seed, draws=1):
    """a dataset of `shapes` = ((width, dtype), ...): `draws` launches from a fresh counter, each against the reference"""
    from icnn_amd import train
    rng = np.random.RandomState(n_rows + batch)
    arrays = [_array(rng, n_rows, w, dt) for w, dt in shapes]
    data = train.DeviceDataset(arrays, seed=seed)
    dev = [a.cuda() for a in arrays]
    big = [torch.full((batch + SPARE, a.shape[1]), FILL, dtype=a.dtype, device="cuda") for a in arrays]
    for d in range(draws):
        idx = data.draw_into(*[b[:batch] for b in big])
        want = ref.indices(seed, d, batch, n_rows)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want), (d, seed)
        pick = torch.from_numpy(want.astype(np.int64)).cuda()
        for a, b in zip(dev, big):
            assert torch.equal(b[:batch], a[pick]), (d, tuple(a.shape), a.dtype)
            assert bool((b[batch:] == FILL).all())
    ctrl = data.ctrl.cpu().numpy()
    assert ctrl.tolist() == [draws, 0, 0, 0, 0, 0, 0, 0] and data.draws == draws and data.status == 0
    data.raise_on_error()


@pytest.mark.parametrize("width", [1, 3, 4, 5, 64, 257, 1836])
def test_float32_row_widths(width):
    """both copy paths (width % 4 == 0 or not), tails, and rows longer than one pass of the workgroup"""
    for seed in SEEDS:
        _check_draws(((width, np.float32),), 1000, 5, seed)


@pytest.mark.parametrize("width, dtype", [(1, np.float64), (3, np.float64), (159, np.float64), (159, np.float32)])
def test_label_rows(width, dtype):
    """float64 rows are 2 n words: 2 and 6 words go word by word, 318 too; float32 159 is the dword path"""
    for seed in SEEDS:
        _check_draws(((8, np.float32), (width, dtype)), 1000, 5, seed)


@pytest.mark.parametrize("shapes", [
    ((1836, np.float32), (159, np.float64)),
    ((5, np.float32), (4, np.float64), (1, np.int32)),
    ((64, np.float32), (3, np.float32), (2, np.float64), (257, np.float32)),
], ids=["two", "three", "four"])
def test_several_arrays(shapes):
    for seed in SEEDS:
        _check_draws(shapes, 1000, 5, seed)


@pytest.mark.parametrize("n_rows", [1, 2, 3, 1000, (1 << 20) + 7])
def test_set_sizes(n_rows):
    width = 1 if n_rows > 1000 else 4
    for seed in SEEDS:
        _check_draws(((width, np.float32),), n_rows, 64, seed)


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 64, 257])
def test_batch_sizes(batch):
    """the grid tails, whichever number of samples a workgroup takes"""
    for seed in SEEDS:
        _check_draws(((5, np.float32), (3, np.float64)), 1000, batch, seed)


def test_counter_through_eager_launches_a_replayed_graph_and_reset():
    """three eager launches use draws 0, 1, 2; a graph holding two draws, replayed twice, continues at 3 .. 6 -- the ticket
    re-arms between consecutive launches and across replays; reset() returns to draw 0"""
    from icnn_amd import train
    n_rows, batch, seed = 1000, 5, SEEDS[1]
    rng = np.random.RandomState(1)
    X, Y = _array(rng, n_rows, 12, np.float32), _array(rng, n_rows, 3, np.float64)
    data = train.DeviceDataset((X, Y), seed=seed)
    Xd, Yd = X.cuda(), Y.cuda()
    x = torch.full((batch, 12), FILL, dtype=torch.float32, device="cuda")
    y = torch.full((batch, 3), FILL, dtype=torch.float64, device="cuda")

    def expect(d, idx, xs, ys):
        want = ref.indices(seed, d, batch, n_rows)
        pick = torch.from_numpy(want.astype(np.int64)).cuda()
        assert np.array_equal(idx.cpu().numpy(), want), d
        assert torch.equal(xs, Xd[pick]) and torch.equal(ys, Yd[pick]), d

    first = data.draw_into(x, y)
    expect(0, first, x, y)
    for d in (1, 2):
        idx = data.draw_into(x, y)
        assert idx.data_ptr() == first.data_ptr()          # one index buffer per batch size
        expect(d, idx, x, y)
    assert data.draws == 3
    torch.cuda.synchronize()
    g, kept = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(g):
        for _ in range(2):
            idx = data.draw_into(x, y)
            kept.append((idx.clone(), x.clone(), y.clone()))
    d = 3
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for idx, xs, ys in kept:
            expect(d, idx, xs, ys)
            d += 1
    assert data.ctrl.cpu().numpy().tolist() == [7, 0, 0, 0, 0, 0, 0, 0]
    data.reset()
    assert data.draws == 0
    expect(0, data.draw_into(x, y), x, y)
    g.replay()                                             # the captured launches read the counter, not a captured value
    torch.cuda.synchronize()
    expect(1, *kept[0])
    expect(2, *kept[1])


def test_draw_into_refuses_wrong_buffers():
    from icnn_amd import train
    X, Y = torch.zeros(10, 6), torch.zeros(10, 3, dtype=torch.float64)
    data = train.DeviceDataset((X, Y))
    x, y = torch.zeros(4, 6, device="cuda"), torch.zeros(4, 3, dtype=torch.float64, device="cuda")
    for bad in [(x,), (x, y, y), (x, y.float()), (x.double(), y), (x[:, :5], y), (torch.zeros(4, 5, device="cuda"), y),
                (x, torch.zeros(3, 3, dtype=torch.float64, device="cuda")), (x.cpu(), y), (x, y.cpu()),
                (torch.zeros(4, 7, device="cuda")[:, 1:], y),
                (torch.zeros(32, device="cuda")[1:25].view(4, 6), y)]:          # the last: 4 bytes off the alignment
        with pytest.raises(ValueError):
            data.draw_into(*bad)
    assert data.draws == 0 and int(data.ctrl.abs().sum().item()) == 0
    for arrays in [(), (X,) * 5, (X, Y[:9]), (torch.zeros(10, 3, dtype=torch.float16),), (torch.zeros(0, 4),)]:
        with pytest.raises(ValueError):
            train.DeviceDataset(arrays)
    assert np.array_equal(data.draw_into(x.view(4, 2, 3), y).cpu().numpy(), ref.indices(0, 0, 4, 10))   # the row size counts


def test_step_log_through_a_graph():
    """columns of the three kinds, capacity 4, appends through a captured graph: read() returns the rows since the last
    read() in order across the ring's wrap, and raises when more than capacity rows were appended"""
    from icnn_amd import train
    f32 = torch.zeros((), dtype=torch.float32, device="cuda")
    f64 = torch.zeros(1, dtype=torch.float64, device="cuda")
    i32 = torch.zeros((), dtype=torch.int32, device="cuda")
    log = train.StepLog([("loss", f32), ("fine", f64), ("rows", i32)], 4)
    third = 1.0 / 3.0

    def advance():
        f32.add_(0.1)
        f64.add_(third)
        i32.sub_(16777217)                               # not a float32: the int32 column is widened, not rounded

    def want(first, count):
        a = np.float32(0.0)
        b, c = np.float64(0.0), 0
        rows = []
        for i in range(first + count):
            a, b, c = np.float32(a + np.float32(0.1)), b + np.float64(third), c - 16777217
            rows.append((float(a), float(b), float(np.int32(c))))
        return np.array(rows[first:], np.float64).reshape(count, 3)

    advance()
    log.append()                                           # eager
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        advance()
        log.append()
    for _ in range(2):
        g.replay()
    got = log.read()
    assert list(got) == ["loss", "fine", "rows"] and all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(np.stack([got[k] for k in got], 1), want(0, 3))
    assert all(v.shape == (0,) for v in log.read().values())
    for _ in range(4):                                     # seven appends so far: rows 3, 0, 1, 2 of the ring
        g.replay()
    got = log.read()
    assert np.array_equal(np.stack([got[k] for k in got], 1), want(3, 4))
    for _ in range(5):
        g.replay()
    with pytest.raises(RuntimeError, match="5 rows"):
        log.read()
    g.replay()
    got = log.read()                                       # reading goes on behind the lost rows
    assert np.array_equal(np.stack([got[k] for k in got], 1), want(12, 1))
    assert int(log.ctrl[0].item()) == 13


def test_step_log_refuses_wrong_columns():
    from icnn_amd import train
    ok = torch.zeros((), device="cuda")
    for cols in [[], [("a", ok)] * 2, [("c%d" % i, ok) for i in range(9)], [("a", torch.zeros(2, device="cuda"))],
                 [("a", torch.zeros(()))], [("a", torch.zeros((), dtype=torch.int64, device="cuda"))], [("a", 1.0)]]:
        with pytest.raises(ValueError):
            train.StepLog(cols, 4)
    with pytest.raises(ValueError):
        train.StepLog([("a", ok)], 0)
