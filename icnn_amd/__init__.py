_FF = ("FFSpec", "FFModel", "FFTrainer", "bibtex_ff_spec")
_FCN = ("FCNSpec", "FCNModel", "FCNTrainer", "olivetti_fcn_spec")


def __getattr__(name):
    # the feed-forward baseline (icnn_amd/ff.py), loaded on first use: importing the package alone loads nothing
    if name in _FF:
        from . import ff
        return getattr(ff, name)
    if name in _FCN:
        from . import fcn
        return getattr(fcn, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
