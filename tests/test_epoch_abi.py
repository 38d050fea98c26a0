"""The epoch level of the training scripts, host side: the new entries are declared, exported and refuse bad
arguments before anything is launched, and the checkpoint file layer round-trips arrays without pickles and never damages an
existing file.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_gd_eval_work_bytes", "icnn_be_gd_eval", "icnn_be_macro_f1", "icnn_be_keep_best"]
EINVAL = -1
P = 64              # a fake non-NULL pointer: every case below is refused before a launch could read it


def test_new_exports_in_header_and_library():
    from icnn_amd import _lib
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()
    assert "be_train_epoch.hip" in __import__("icnn_amd.build", fromlist=["SOURCES"]).SOURCES
    assert lib.icnn_be_gd_eval_work_bytes(128) >= 128 * 8 + 4
    assert lib.icnn_be_gd_eval_work_bytes(128) == lib.icnn_be_gd_feed_work_bytes(128)
    assert lib.icnn_be_gd_eval_work_bytes(0) == 0 and lib.icnn_be_gd_eval_work_bytes(-3) == 0


def test_einval_is_minus_one():
    from icnn_amd import _lib
    assert "invalid" in _lib.ERRORS[EINVAL].lower() or "EINVAL" in _lib.ERRORS[EINVAL]


@pytest.mark.parametrize("B,n", [(0, 4), (-1, 4), (4, 0), (4, -2)])
def test_gd_eval_rejects_sizes(B, n):
    from icnn_amd import _lib
    lib = _lib.load()
    assert lib.icnn_be_gd_eval(P, P, B, n, P, P, P, None) == EINVAL


@pytest.mark.parametrize("null", ["yK", "t", "loss", "work"])
def test_gd_eval_rejects_null(null):
    from icnn_amd import _lib
    lib = _lib.load()
    a = dict(yK=P, t=P, loss=P, tallies=P, work=P)
    a[null] = None
    assert lib.icnn_be_gd_eval(a["yK"], a["t"], 4, 3, a["loss"], a["tallies"], a["work"], None) == EINVAL


def test_macro_f1_rejects_bad_arguments():
    from icnn_amd import _lib
    lib = _lib.load()
    assert lib.icnn_be_macro_f1(P, 0, P, None) == EINVAL
    assert lib.icnn_be_macro_f1(P, -5, P, None) == EINVAL
    assert lib.icnn_be_macro_f1(None, 4, P, None) == EINVAL
    assert lib.icnn_be_macro_f1(P, 4, None, None) == EINVAL


def test_keep_best_rejects_bad_arguments():
    from icnn_amd import _lib
    lib = _lib.load()
    for mode in (-1, 2, 7):
        assert lib.icnn_be_keep_best(P, 0, mode, P, P, None) == EINVAL
        assert lib.icnn_be_keep_best(P, 1, mode, P, P, None) == EINVAL
    for mode in (0, 1):
        assert lib.icnn_be_keep_best(None, 0, mode, P, P, None) == EINVAL
        assert lib.icnn_be_keep_best(P, 0, mode, None, P, None) == EINVAL
        assert lib.icnn_be_keep_best(P, 1, mode, P, None, None) == EINVAL
    assert _lib.KEEP_MODE == {"min": 0, "max": 1}


# ---- the file layer -------------------------------------------------------------------------
def _mixed():
    rng = np.random.RandomState(3)
    return {"theta": rng.randn(37).astype(np.float32), "best": np.asarray([-np.inf]), "gate": np.array([1, 6, 2], np.int32),
            "keys": rng.randint(0, 2 ** 32, 624, dtype=np.uint64).astype(np.uint32), "terminals": np.array([0, 1, 1], np.uint8),
            "kind": np.asarray("GDTrainer"), "spec": np.asarray('{"n_features": 40}'), "empty": np.zeros((0, 5), np.float64),
            "scalar": np.asarray(7, np.int64), "nan": np.asarray([np.nan, 1.5], np.float64)}


def test_file_round_trip_without_pickle(tmp_path):
    from icnn_amd import checkpoint
    path = str(tmp_path / "ck.npz")
    arrays = _mixed()
    checkpoint.write_arrays(path, arrays)
    assert not os.path.exists(path + ".tmp")
    back = checkpoint.read_arrays(path)
    assert set(back) == set(arrays) | {"format"}
    assert int(back["format"]) == checkpoint.FORMAT
    for k, a in arrays.items():
        assert back[k].dtype == a.dtype and back[k].shape == a.shape, k
        assert np.array_equal(back[k], a, equal_nan=a.dtype.kind == "f"), k
    assert str(back["kind"]) == "GDTrainer"
    with np.load(path, allow_pickle=False) as z:                # a plain .npz: no pickles inside
        assert set(z.files) == set(back)
        for k in z.files:
            z[k]
    with pytest.raises(ValueError):                             # an object array would need a pickle
        checkpoint.write_arrays(path, {"x": np.array([{"a": 1}], dtype=object)})
    assert set(checkpoint.read_arrays(path)) == set(back)


def test_unknown_format_raises(tmp_path):
    from icnn_amd import checkpoint
    path = str(tmp_path / "ck.npz")
    checkpoint.write_arrays(path, {"format": np.asarray(checkpoint.FORMAT + 98, np.int64), "x": np.zeros(3)})
    with pytest.raises(ValueError, match="format"):
        checkpoint.read_arrays(path)
    np.savez(path, x=np.zeros(3))                               # no format key at all
    with pytest.raises(ValueError, match="format"):
        checkpoint.read_arrays(path)


def test_failed_replace_leaves_the_old_file(tmp_path, monkeypatch):
    from icnn_amd import checkpoint
    path = str(tmp_path / "ck.npz")
    checkpoint.write_arrays(path, {"x": np.arange(5)})
    before = open(path, "rb").read()

    def refuse(src, dst):
        raise OSError("cannot replace")
    monkeypatch.setattr(checkpoint.os, "replace", refuse)
    with pytest.raises(OSError):
        checkpoint.write_arrays(path, {"x": np.arange(50)})
    monkeypatch.undo()
    assert open(path, "rb").read() == before
    assert np.array_equal(checkpoint.read_arrays(path)["x"], np.arange(5))


def test_spec_json_tells_specs_apart():
    from icnn_amd import checkpoint, ficnn, picnn
    a = checkpoint.spec_json(picnn.FCSpec(40, 16, (64, 32), batchnorm=True))
    assert a == checkpoint.spec_json(picnn.FCSpec(40, 16, (64, 32), batchnorm=True))
    assert a != checkpoint.spec_json(picnn.FCSpec(40, 16, (64, 48), batchnorm=True))
    assert a != checkpoint.spec_json(picnn.FCSpec(40, 16, (64, 32), batchnorm=False))
    assert checkpoint.spec_json(ficnn.synthetic_spec()) != checkpoint.spec_json(picnn.synthetic_spec())
