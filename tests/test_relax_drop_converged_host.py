"""CPU tests of ``drop_converged`` (LBFGS.set_drop_converged, relax_opt["drop_converged"]): the option's plumbing through
``ml_relax``, the constructor signature it must leave alone, its guards, and the C entries it adds."""
import inspect
import re
from pathlib import Path

import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd.lbfgs_torch import LBFGS
from adsorbdiff_amd.synthetic import make_batch

NEW_ENTRIES = ("adf_lbfgs_active_build", "adf_active_gather", "adf_active_scatter")


class _StubLBFGS:
    """The reference's interface: a constructor, ``run`` - and no ``set_drop_converged``."""
    seen = []

    def __init__(self, batch, calc, **kw):
        self.batch = batch
        _StubLBFGS.seen.append(kw)

    def run(self, fmax, steps):
        self.batch.y = torch.zeros(len(self.batch.sid))
        self.batch.force = torch.zeros_like(self.batch.pos)
        return self.batch


class _StubWithOption(_StubLBFGS):
    calls = []

    def set_drop_converged(self, on):
        _StubWithOption.calls.append(on)


def test_relax_opt_drop_converged_reaches_the_optimizer(monkeypatch):
    b = make_batch(2, n_slab=4, n_ads=1, seed=3)
    monkeypatch.setattr(MR, "LBFGS", _StubWithOption)
    _StubWithOption.calls = []
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7, "drop_converged": True}, False, device="cpu")
    assert _StubWithOption.calls == [True]
    assert "drop_converged" not in _StubLBFGS.seen[-1]         # not a constructor keyword
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7}, False, device="cpu")
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7, "drop_converged": False}, False, device="cpu")
    assert _StubWithOption.calls == [True]                     # absent or False: nothing is called
    # a stand-in with the reference's interface alone keeps working while the option is off
    monkeypatch.setattr(MR, "LBFGS", _StubLBFGS)
    out = MR.ml_relax(b, None, 5, 0.05, {"memory": 7}, False, device="cpu")
    assert out.sid == b.sid
    MR.ml_relax(b, None, 5, 0.05, {"memory": 7, "drop_converged": False}, False, device="cpu")
    with pytest.raises(AttributeError, match="set_drop_converged"):
        MR.ml_relax(b, None, 5, 0.05, {"memory": 7, "drop_converged": True}, False, device="cpu")


class _Calc:
    model = type("T", (), {"_unwrapped_model": type("M", (), {"otf_graph": True})()})()


def test_constructor_is_untouched_and_the_setter_guards():
    params = list(inspect.signature(LBFGS.__init__).parameters)
    assert params[-2:] == ["early_stop_batch", "per_system"] and "drop_converged" not in params
    b = make_batch(1, n_slab=4, n_ads=1, seed=3)
    opt = LBFGS(b, _Calc(), memory=5, device="cpu")
    assert opt.drop_converged is False and opt.forward_log == []
    early = LBFGS(b, _Calc(), memory=5, device="cpu", early_stop_batch=True)
    with pytest.raises(ValueError, match="early_stop_batch"):
        early.set_drop_converged(True)
    assert early.drop_converged is False
    early.set_drop_converged(False)                            # switching it off is always allowed
    for per_system in (False, True):
        opt = LBFGS(b, _Calc(), memory=5, device="cpu", per_system=per_system)
        opt.set_drop_converged(True)
        assert opt.drop_converged is True
        opt.set_drop_converged(False)
        assert opt.drop_converged is False


def test_new_entries_are_exported_bound_and_declared():
    lib = L.load()
    hdr = (Path(__file__).resolve().parent.parent / "include" / "adsorbdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(adf_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW_ENTRIES:
        assert name in L.EXPORTS and name in declared
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is L.C.c_int32
    assert L.ActiveField._fields_ == [("src", L.C.c_void_p), ("dst", L.C.c_void_p), ("row_bytes", L.C.c_int32),
                                      ("per_system", L.C.c_int32)]


def test_entries_refuse_bad_arguments_without_a_device():
    """The argument checks run before anything touches the device."""
    lib = L.load()
    one = (L.ActiveField * 1)()
    one[0].src, one[0].dst, one[0].row_bytes, one[0].per_system = 64, 128, 6, 0
    assert lib.adf_active_gather(64, 64, 64, 64, 2, 8, one, 1, None, None, None) == L.ADF_EINVAL
    assert b"multiple of 4" in lib.adf_last_error()
    one[0].row_bytes = 12
    assert lib.adf_active_gather(64, None, 64, 64, 2, 8, one, 1, None, None, None) == L.ADF_EINVAL
    one[0].dst = None
    assert lib.adf_active_gather(64, 64, 64, 64, 2, 8, one, 1, None, None, None) == L.ADF_EINVAL
    assert lib.adf_active_gather(64, 64, 64, 64, 2, 8, None, 0, None, None, None) == L.ADF_EINVAL
    assert lib.adf_active_scatter(64, 64, 64, 64, 2, 8, 64, None, 4, 64, 64, None, None, None) == L.ADF_EINVAL
    assert lib.adf_active_scatter(64, 64, 64, 64, 2, 8, 64, 64, 6, 64, 64, 64, 64, None) == L.ADF_EINVAL
    assert lib.adf_lbfgs_active_build(None, 64, 64, 64, 64, None) == L.ADF_EINVAL
