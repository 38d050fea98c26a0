"""The surface and the bits of every supervised trainer, pinned in tests/golden/trainer_surface.json (written by
tools/gen_golden_trainers.py on the MI355X): BundleTrainer on an FCModel ("xent") and on a ConvModel ("mse"), GDTrainer with
f1=True, ConvGDTrainer, ficnn.GDTrainer, ff.FFTrainer and fcn.FCNTrainer, each without a test phase and with an eval_batch that
differs from the batch (ficnn.GDTrainer has no test phase: one run).  Per run:

    surface    the public attributes after construction (name -> type; a tensor's dtype, shape and device type; a plain
               number's or string's value) and the sorted public method names equal the fixture's;
    bits       three step() calls on fixed data, then one evaluate(): the SHA-256 of the bytes of every parameter vector, Adam
               moment, step count, arena, moving statistic and public tensor of the trainer (loss, grad, eval_loss, y_eval ...)
               equals the fixture's -- the kernels are deterministic on one architecture;
    isolation  evaluate() leaves every training-phase tensor, the parameters, the optimiser state and the moving statistics
               bit-identical, step() leaves every eval-phase tensor bit-identical, and evaluate() without eval_batch raises
               ValueError.

The shapes are the smallest the kernels accept (FF: batch 2, one hidden layer; FCN: 8 x 8, k = 16, batch 1) and the smallest
specs of tests/test_epoch_trainers.py, tests/test_conv_gd_trainer.py and tests/test_ficnn_train.py, with n_iter 2 or 3."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_surface.json")
KINDS = ("bundle_fc", "bundle_conv", "gd", "conv_gd", "ficnn", "ff", "fcn")
CASES = [(kind, with_eval) for kind in KINDS for with_eval in (False, True) if not (kind == "ficnn" and with_eval)]
STEPS = 3


def case_id(kind, with_eval):
    return "%s-%s" % (kind, "eval" if with_eval else "plain")


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def build(kind, with_eval):
    """(trainer, the batch size E of its test phase or None, batch(rows, seed) -> the arguments of step / evaluate)"""
    from icnn_amd import fcn, ff, ficnn, picnn, train
    if kind in ("bundle_fc", "gd"):
        spec = picnn.FCSpec(20, 12, (24, 12), alpha=0.0, batchnorm=True, action_box=False)
        model = picnn.FCModel(spec, picnn.init_params(spec, 5, "spread"), "cuda")
        B, E = 4, 3
        if kind == "bundle_fc":
            tr = train.BundleTrainer(model, B, n_iter=3, loss="xent", variant="pdipm", lr=1e-3, eval_batch=E if with_eval else None)
            dtype = np.float64
        else:
            tr = train.GDTrainer(model, B, n_iter=3, lr=0.1, momentum=0.3, adam_lr=1e-2, bn_updates=1, f1=True,
                                 eval_batch=E if with_eval else None)
            dtype = np.float32

        def batch(rows, seed):
            rng = np.random.RandomState(seed)
            return _cuda(rng.rand(rows, spec.n_features).astype(np.float32), (rng.rand(rows, spec.n_labels) < 0.3).astype(dtype))
    elif kind in ("bundle_conv", "conv_gd"):
        spec = picnn.ConvSpec(32, 32)
        model = picnn.ConvModel(spec, picnn.init_conv_params(spec, 8, "spread"), "cuda")
        B, E = 2, 3
        if kind == "bundle_conv":
            tr = train.BundleTrainer(model, B, n_iter=2, loss="mse", variant="pdipm", lr=1e-3, eval_batch=E if with_eval else None)
            dtype = np.float64
        else:
            tr = train.ConvGDTrainer(model, B, n_iter=2, lr=0.01, momentum=0.9, y0=0.5, bn_updates=1,
                                     eval_batch=E if with_eval else None)
            dtype = np.float32

        def batch(rows, seed):
            rng = np.random.RandomState(seed)
            return _cuda(rng.rand(rows, spec.H, spec.W, 1).astype(np.float32), rng.rand(rows, spec.n_labels).astype(dtype))
    elif kind == "ficnn":
        spec = ficnn.synthetic_spec()
        B, E = 4, None
        tr = ficnn.GDTrainer(ficnn.FICNNModel(spec, ficnn.make_convex(ficnn.init_params(spec, 0))), B, n_iter=3, adam_lr=1e-2)

        def batch(rows, seed):
            rng = np.random.RandomState(seed)
            return _cuda(rng.uniform(-1, 1, (rows, 2)).astype(np.float32), (rng.rand(rows, 1) < 0.5).astype(np.float32))
    elif kind == "ff":
        spec = ff.FFSpec(5, 3, (4,))
        B, E = 2, 1
        tr = ff.FFTrainer(ff.FFModel(spec, seed=0), B, eval_batch=E if with_eval else None)

        def batch(rows, seed):
            rng = np.random.RandomState(seed)
            return _cuda(rng.rand(rows, spec.n_features).astype(np.float32), (rng.rand(rows, spec.n_labels) < 0.4).astype(np.float32))
    else:
        assert kind == "fcn"
        spec = fcn.FCNSpec(8, 8, 16)
        B, E = 1, 2
        tr = fcn.FCNTrainer(fcn.FCNModel(spec, seed=0), B, eval_batch=E if with_eval else None)

        def batch(rows, seed):
            rng = np.random.RandomState(seed)
            return _cuda(rng.rand(rows, spec.H, spec.W, 1).astype(np.float32), rng.rand(rows, spec.H * spec.W).astype(np.float32))
    return tr, (E if with_eval else None), batch


# ------------------------------------------------------------------------------------------------ what is recorded


def _describe(value):
    if torch.is_tensor(value):
        return "Tensor %s %s %s" % (value.dtype, list(value.shape), value.device.type)
    if isinstance(value, dict) and value and all(torch.is_tensor(t) for t in value.values()):
        return {k: _describe(t) for k, t in sorted(value.items())}
    if value is None or isinstance(value, (bool, int, float, str)):
        return "%s %r" % (type(value).__name__, value)
    return type(value).__name__


def surface(tr):
    """the public attributes of the instance and the public methods (properties too) of its class"""
    attributes = {name: _describe(value) for name, value in sorted(vars(tr).items()) if not name.startswith("_")}
    methods = sorted(name for name in dir(type(tr)) if not name.startswith("_")
                     and (callable(getattr(type(tr), name)) or isinstance(getattr(type(tr), name), property)))
    return {"attributes": attributes, "methods": methods}


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _state(tr):
    """{name: tensor} of the parameters, the optimiser state and the moving statistics"""
    out = {}
    opt = getattr(tr, "opt", None)
    if opt is not None:
        out.update({"opt." + k: getattr(opt, k) for k in ("theta", "m", "v", "step_count", "arena")})
    else:
        for group in ("theta", "m", "v"):
            out.update({"%s[%s]" % (group, k): t for k, t in getattr(tr, group).items()})
        out["step_count"] = tr.step_count
    for k, t in (getattr(tr.model, "bn_stats", None) or {}).items():
        out["bn_stats[%s]" % k] = t
    return out


def _tensors(tr, eval_phase, private=True):
    """{name: tensor} of the trainer's own tensor attributes of one phase: the test phase's carry "eval" in their names"""
    return {name: t for name, t in vars(tr).items()
            if torch.is_tensor(t) and ("eval" in name) == eval_phase and (private or not name.startswith("_"))}


def _digests(tensors):
    torch.cuda.synchronize()
    return {name: _sha(t) for name, t in sorted(tensors.items())}


def record(kind, with_eval):
    """One run of a case: {"surface": ..., "bits": {name: sha256}}; the isolation properties are asserted on the way."""
    tr, E, batch = build(kind, with_eval)
    B = tr.batch
    out = {"surface": surface(tr)}
    for i in range(STEPS - 1):
        tr.step(*batch(B, 100 + i))
    if E is None:
        tr.step(*batch(B, 100 + STEPS - 1))
        if hasattr(tr, "evaluate"):
            with pytest.raises(ValueError, match="eval_batch"):
                tr.evaluate()
    else:
        tr.evaluate(*batch(E, 200))
        eval_side = lambda: _digests(_tensors(tr, True))                        # noqa: E731
        before = eval_side()
        assert len(before) >= 3, sorted(before)
        tr.step(*batch(B, 100 + STEPS - 1))
        assert eval_side() == before, "step() wrote an eval-phase tensor"
        train_side = lambda: _digests({**_tensors(tr, False), **_state(tr)})     # noqa: E731
        before = train_side()
        loss = tr.evaluate(*batch(E, 201))
        assert loss is tr.eval_loss
        assert train_side() == before, "evaluate() wrote a training-phase tensor, a parameter or a statistic"
    out["bits"] = _digests({**_tensors(tr, False, private=False), **_tensors(tr, True, private=False), **_state(tr)})
    return out


# ------------------------------------------------------------------------------------------------ the tests


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(case_id(*c) for c in CASES)
    for entry in golden.values():
        assert set(entry) == {"surface", "bits"}
        assert all(len(h) == 64 and set(h) <= set("0123456789abcdef") for h in entry["bits"].values())
        for name in ("loss",):
            assert name in entry["bits"] and name in entry["surface"]["attributes"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,with_eval", CASES, ids=[case_id(*c) for c in CASES])
def test_surface_bits_and_isolation(kind, with_eval, golden):
    want = golden[case_id(kind, with_eval)]
    got = json.loads(json.dumps(record(kind, with_eval)))       # tuples and lists compare as the file holds them
    assert got["surface"]["methods"] == want["surface"]["methods"]
    assert got["surface"]["attributes"] == want["surface"]["attributes"]
    assert got["bits"] == want["bits"]
