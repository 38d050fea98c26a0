"""The training set on the device, host side: icnn_be_dataset_draw and icnn_be_log_row are declared, exported
and refuse bad arguments before anything is launched; the index rule of tests/dataset_ref.py gives its known answers and a
flat histogram.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import dataset_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_dataset_draw", "icnn_be_log_row"]
EINVAL = -1
P = 64              # a fake non-NULL, 16-byte aligned pointer: every case below is refused before a launch could read it


def test_new_exports_in_header_and_library():
    from icnn_amd import _lib
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()
    assert "be_train_data.hip" in __import__("icnn_amd.build", fromlist=["SOURCES"]).SOURCES
    assert re.search(r"#define ICNN_BE_DATASET_MAX_ARRAYS %d\b" % _lib.DATASET_MAX_ARRAYS, header)
    assert re.search(r"#define ICNN_BE_DATASET_CTRL_INTS %d\b" % _lib.DATASET_CTRL_INTS, header)
    assert re.search(r"#define ICNN_BE_LOG_MAX_COLUMNS %d\b" % _lib.LOG_MAX_COLUMNS, header)
    assert (_lib.DATASET_MAX_ARRAYS, _lib.DATASET_CTRL_INTS, _lib.LOG_MAX_COLUMNS) == (4, 8, 8)
    assert _lib.LOG_KIND == {"float32": 0, "float64": 1, "int32": 2}


def test_struct_sizes():
    from icnn_amd import _lib
    lib = _lib.load()
    assert lib.icnn_be_struct_size(10) == C.sizeof(_lib.Dataset) > 0
    assert lib.icnn_be_struct_size(11) == C.sizeof(_lib.StepLog) > 0
    assert lib.icnn_be_struct_size(9) == C.sizeof(_lib.Replay) and lib.icnn_be_struct_size(12) == 0


def _dataset(n_rows=10, n_arrays=2, src=(P, P, P, P), row_words=(3, 4, 1, 1), ctrl=P):
    from icnn_amd import _lib
    d = _lib.Dataset()
    d.n_rows, d.n_arrays, d.ctrl = n_rows, n_arrays, ctrl
    for i in range(4):
        d.src[i], d.row_words[i] = src[i], row_words[i]
    return d


def _draw(d, batch=5, dst=(P, P, P, P), idx=P, stream=None):
    from icnn_amd import _lib
    arr = None if dst is None else (C.c_void_p * 4)(*dst)
    return _lib.load().icnn_be_dataset_draw(None if d is None else C.byref(d), batch, 7, arr, idx, stream)


DRAW_REFUSALS = {
    "NULL d": lambda: _draw(None),
    "NULL ctrl": lambda: _draw(_dataset(ctrl=None)),
    "NULL idx": lambda: _draw(_dataset(), idx=None),
    "NULL dst": lambda: _draw(_dataset(), dst=None),
    "NULL src[0]": lambda: _draw(_dataset(src=(None, P, P, P))),
    "NULL src[1]": lambda: _draw(_dataset(src=(P, None, P, P))),
    "NULL src[3]": lambda: _draw(_dataset(n_arrays=4, src=(P, P, P, None))),
    "NULL dst[0]": lambda: _draw(_dataset(), dst=(None, P, P, P)),
    "NULL dst[1]": lambda: _draw(_dataset(), dst=(P, None, P, P)),
    "N = 0": lambda: _draw(_dataset(n_rows=0)),
    "N < 0": lambda: _draw(_dataset(n_rows=-4)),
    "batch = 0": lambda: _draw(_dataset(), batch=0),
    "batch < 0": lambda: _draw(_dataset(), batch=-1),
    "no arrays": lambda: _draw(_dataset(n_arrays=0)),
    "negative arrays": lambda: _draw(_dataset(n_arrays=-1)),
    "five arrays": lambda: _draw(_dataset(n_arrays=5)),
    "row_words = 0": lambda: _draw(_dataset(row_words=(3, 0, 1, 1))),
    "row_words < 0": lambda: _draw(_dataset(row_words=(-2, 4, 1, 1))),
    "src 4-byte aligned": lambda: _draw(_dataset(src=(P + 4, P, P, P))),
    "src 8-byte aligned": lambda: _draw(_dataset(src=(P, P + 8, P, P))),
    "dst 4-byte aligned": lambda: _draw(_dataset(), dst=(P, P + 4, P, P)),
    "dst 8-byte aligned": lambda: _draw(_dataset(), dst=(P + 8, P, P, P)),
    "idx 4-byte aligned": lambda: _draw(_dataset(), idx=P + 4),
    "idx 8-byte aligned": lambda: _draw(_dataset(), idx=P + 8),
    "ctrl 2-byte aligned": lambda: _draw(_dataset(ctrl=P + 2)),
    "stream misaligned": lambda: _draw(_dataset(), stream=P + 4),
}


@pytest.mark.parametrize("case", sorted(DRAW_REFUSALS))
def test_dataset_draw_refuses(case):
    assert DRAW_REFUSALS[case]() == EINVAL


def _log(rows=P, ctrl=P, cap=4, width=3, col=(P,) * 8, kind=(0, 1, 2, 0, 0, 0, 0, 0)):
    from icnn_amd import _lib
    L = _lib.StepLog()
    L.rows, L.ctrl, L.cap, L.width = rows, ctrl, cap, width
    for j in range(8):
        L.col[j], L.kind[j] = col[j], kind[j]
    return L


def _log_row(L, stream=None):
    from icnn_amd import _lib
    return _lib.load().icnn_be_log_row(None if L is None else C.byref(L), stream)


LOG_REFUSALS = {
    "NULL L": lambda: _log_row(None),
    "NULL rows": lambda: _log_row(_log(rows=None)),
    "NULL ctrl": lambda: _log_row(_log(ctrl=None)),
    "NULL col[0]": lambda: _log_row(_log(col=(None,) + (P,) * 7)),
    "NULL col[2]": lambda: _log_row(_log(col=(P, P, None) + (P,) * 5)),
    "cap = 0": lambda: _log_row(_log(cap=0)),
    "cap < 0": lambda: _log_row(_log(cap=-1)),
    "width = 0": lambda: _log_row(_log(width=0)),
    "width = 9": lambda: _log_row(_log(width=9)),
    "kind 3": lambda: _log_row(_log(kind=(0, 3, 2, 0, 0, 0, 0, 0))),
    "kind -1": lambda: _log_row(_log(kind=(-1, 1, 2, 0, 0, 0, 0, 0))),
    "rows 4-byte aligned": lambda: _log_row(_log(rows=P + 4)),
    "float64 column 4-byte aligned": lambda: _log_row(_log(col=(P, P + 4) + (P,) * 6)),
    "float32 column 2-byte aligned": lambda: _log_row(_log(col=(P + 2,) + (P,) * 7)),
    "stream misaligned": lambda: _log_row(_log(), stream=P + 4),
}


@pytest.mark.parametrize("case", sorted(LOG_REFUSALS))
def test_log_row_refuses(case):
    assert LOG_REFUSALS[case]() == EINVAL


@pytest.mark.parametrize("seed, n_rows, draw, want", [
    (0, 1000, 0, [178, 308, 56, 486, 86, 915, 146, 356]),
    (0, 1000, 1, [911, 462, 622, 709]),
    (0, (1 << 20) + 7, 0, [187624, 323716, 59628, 509683]),
])
def test_index_rule_known_answers(seed, n_rows, draw, want):
    assert ref.indices(seed, draw, len(want), n_rows).tolist() == want


def test_index_rule_keeps_its_range_and_its_own_stream():
    import replay_ref
    for n_rows in (1, 2, 3, 63):
        idx = [ref.index(7, d, k, n_rows) for d in range(4) for k in range(300)]
        assert min(idx) == 0 and max(idx) == n_rows - 1
    for n_rows in (1000, (1 << 20) + 7, (1 << 31) - 1):
        idx = [ref.index(7, d, k, n_rows) for d in range(2) for k in range(100)]
        assert 0 <= min(idx) and max(idx) < n_rows and len(set(idx)) > 100
    # domain tag 1: not the replay memory's candidates (tag 0) at the same seed, draw and range
    mine = [ref.index(0, 0, k, 1000) for k in range(8)]
    theirs = [replay_ref.candidate(0, 0, k, 0, 1001) for k in range(8)]
    assert mine != theirs
    assert ref.index((5 << 32) | 3, 2, 1, 1 << 20) != ref.index(3, 2, 1, 1 << 20)      # the high key word counts


@pytest.mark.parametrize("n_rows, bound", [(16, 37.70), (3, 13.82)])       # chi-square at p = 0.001, N - 1 degrees of freedom
@pytest.mark.parametrize("seed", [0, 7])
def test_index_rule_histogram_is_flat(seed, n_rows, bound):
    """a guard against a mis-stated rule, not a measurement: the rule gives 5.65 / 14.38 at N = 16 and 1.52 / 0.52 at N = 3
    for seeds 0 / 7"""
    assert ref.chi_square(seed, n_rows) < bound
