"""CPU tests of the anomaly flags and the site ranking: the float64 oracle on hand-built cases, the generated batch's margins
and flag balance, the C entries, the radius-table rule, the host-side regrouping of ``best_sites`` and ``ml_relax``'s options."""
import builtins
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from adsorbdiff_amd import flag_anomaly as FA
from adsorbdiff_amd import lib as L
from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd.synthetic import make_batch
from tests import helpers_flag_anomaly as H

ROOT = Path(__file__).resolve().parent.parent


def test_oracle_on_hand_built_cases():
    """CO on a slab: unchanged gives no flag, every perturbation raises its own flag alone, none near a threshold."""
    s, cases = H.co_on_slab()
    assert list(cases) == ["unchanged", "dissociated", "desorbed", "surface_changed", "intercalated"]
    for name, (final, want) in cases.items():
        flags, margin = H.oracle_flags(s["pos"], final, s["Z"], s["tags"], s["cell"], s["radii"])
        assert flags.astype(int).tolist() == want, name
        assert margin >= H.MIN_MARGIN, (name, margin)
    # a relaxed clean slab that differs from the initial one changes the reference of the surface test alone
    final, _ = cases["surface_changed"]
    slab = s["tags"] != 2
    flags, _ = H.oracle_flags(s["pos"], final, s["Z"], s["tags"], s["cell"], s["radii"], slab_ref=final[slab])
    assert flags.astype(int).tolist() == [0, 0, 0, 0]
    # no adsorbate: desorbed, as the reference's loop makes it
    flags, _ = H.oracle_flags(s["pos"][slab], s["pos"][slab], s["Z"][slab], s["tags"][slab], s["cell"], s["radii"])
    assert flags.astype(int).tolist() == [0, 1, 0, 0]


def test_generated_batch_margins_and_balance():
    systems, radii = H.generated_systems()
    assert len(systems) == H.N_SYSTEMS == 48 and radii.min() >= 0.3 and radii.max() <= 1.6
    assert all(s["margin"] >= H.MIN_MARGIN for s in systems)
    flags = np.stack([s["flags"] for s in systems])
    true, false = flags.sum(0), (~flags).sum(0)
    print("true per flag", true.tolist(), "redraws", sum(s["draws"] - 1 for s in systems))
    assert (true >= 5).all() and (false >= 5).all(), (true, false)
    sizes = [len(s["Z"]) for s in systems]
    assert min(sizes) == 3 and max(sizes) > 256 and len(set(sizes)) > 10      # ragged, one system beyond the j tile
    assert all(abs(np.linalg.det(s["cell"])) > 1 and s["cell"][1, 0] != 0 for s in systems)   # triclinic
    assert all(np.abs(s["pos"]).max() < 60 and np.abs(s["final"]).max() < 60 for s in systems)
    again, _ = H.generated_systems()
    assert again is systems


def test_tiled_slab_needs_every_tile_loop():
    """The hand-ordered 322-atom slab: every case gives its flag alone, and an evaluation that skipped the second j tile, did
    not stride over the row tiles, or dropped the last row tile would get a case wrong - which the generated systems, whose
    large members have their evidence everywhere or nowhere, cannot show (asserted too, so that nobody relies on them)."""
    faults = ("second_j_tile", "no_stride", "last_row_tile")
    caught = {f: set() for f in faults}
    for at in (0, 64, 128):
        s, cases = H.tiled_slab(at)
        n = len(s["Z"])
        assert n == 322 and (n + H.ROW_TILE - 1) // H.ROW_TILE == 6 and n > H.J_TILE
        for name, (final, want) in cases.items():
            flags, margin = H.oracle_flags(s["pos"], final, s["Z"], s["tags"], s["cell"], s["radii"])
            assert flags.astype(int).tolist() == want and margin >= H.MIN_MARGIN, (at, name, margin)
            for f in faults:
                seen, _ = H.oracle_flags(s["pos"], final, s["Z"], s["tags"], s["cell"], s["radii"],
                                         pair_mask=H.skipped_pairs_mask(n, f))
                if not np.array_equal(seen, flags):
                    caught[f].add((at, name))
    assert (0, "unchanged") in caught["second_j_tile"] and (0, "surface_changed") in caught["second_j_tile"]
    assert (64, "intercalated") in caught["second_j_tile"]
    assert (0, "dissociated") in caught["no_stride"] and (128, "unchanged") in caught["no_stride"]
    assert (128, "intercalated") in caught["no_stride"] and (0, "dissociated") in caught["last_row_tile"]
    systems, radii = H.generated_systems()
    big = [s for s in systems if len(s["Z"]) > H.J_TILE]
    assert len(big) == 1
    seen, _ = H.oracle_flags(big[0]["pos"], big[0]["final"], big[0]["Z"], big[0]["tags"], big[0]["cell"], radii,
                             pair_mask=H.skipped_pairs_mask(len(big[0]["Z"]), "second_j_tile"))
    assert np.array_equal(seen, big[0]["flags"])


def test_c_entries_are_declared_exported_and_reject_null_arguments():
    lib = L.load()
    header = (ROOT / "include" / "adsorbdiff_hip.h").read_text()
    for name in ("adf_flag_anomalies", "adf_select_best_sites"):
        assert name in L.EXPORTS and hasattr(lib, name) and f" {name}(" in header, name
    assert "flag_anomaly.py:6-154" in header and "eval.py:566-579" in header
    f = C.c_float
    assert lib.adf_flag_anomalies(None, None, None, None, None, 0, f(0.3), f(1.5), f(1.5), None, None) == L.ADF_EINVAL
    d = L.BatchDesc()
    d.num_systems, d.num_atoms = 1, 2
    assert lib.adf_flag_anomalies(C.byref(d), None, None, None, None, 10, f(0.3), f(1.5), f(1.5), None, None) == L.ADF_EINVAL
    assert b"flag_anomalies" in lib.adf_last_error()
    assert lib.adf_select_best_sites(None, None, None, 1, None, None, None, None) == L.ADF_EINVAL
    assert b"select_best_sites" in lib.adf_last_error()
    assert "anomaly.hip" in __import__("adsorbdiff_amd.build", fromlist=["SOURCES"]).SOURCES


def test_default_radii_need_ase_and_say_so(monkeypatch):
    real = builtins.__import__

    def no_ase(name, *a, **kw):
        if name == "ase" or name.startswith("ase."):
            raise ImportError("No module named 'ase'")
        return real(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", no_ase)
    with pytest.raises(ImportError, match="pass a table"):
        FA.default_radii()
    with pytest.raises(ImportError, match="pass a table"):       # before anything touches a device
        FA.flag_anomalies(make_batch(1, n_slab=4, n_ads=1, seed=3), torch.zeros(5, 3))
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FA.flag_anomalies(make_batch(1, n_slab=4, n_ads=1, seed=3), torch.zeros(5, 3), radii=H.synthetic_radii())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FA.best_sites(torch.zeros(3), None, torch.zeros(3, dtype=torch.long))
    # no table of radii lives in the package
    assert not any(isinstance(v, (list, tuple, np.ndarray)) and len(v) > 20 for v in vars(FA).values())


def test_regroup_against_numpy():
    rng = np.random.default_rng(2)
    group = rng.choice([7, -3, 12, 40, 41], size=57)
    perm, offsets, ids = FA.regroup(torch.tensor(group))
    assert ids.tolist() == sorted(set(group.tolist()))
    assert perm.tolist() == np.argsort(group, kind="stable").tolist()
    assert offsets.dtype == torch.int32 and offsets[0] == 0 and offsets[-1] == 57
    for k, g in enumerate(ids.tolist()):
        members = perm[offsets[k]:offsets[k + 1]].tolist()
        assert members == np.nonzero(group == g)[0].tolist()      # contiguous, the caller's order kept inside a group
    slab = FA.scatter_slab_positions(torch.tensor([0, 2, 1, 2]), torch.zeros(4, 3), torch.ones(2, 3))
    assert slab[:, 0].tolist() == [1.0, 0.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="slab atoms"):
        FA.scatter_slab_positions(torch.tensor([0, 2, 1, 2]), torch.zeros(4, 3), torch.ones(3, 3))


def test_ml_relax_option_parsing(monkeypatch):
    """Off by default: no ``anomaly``, nothing new reaches the optimizer.  On: one call on the collated result, with the given
    positions in the returned (split) order, the relaxed positions and the table."""
    kwargs, calls = [], []

    class StubLBFGS:
        def __init__(self, batch, calc, **kw):
            self.batch = batch
            kwargs.append(kw)

        def run(self, fmax, steps):
            if len(self.batch.sid) > 2:
                raise RuntimeError("HIP out of memory")
            self.batch.pos += 1.0            # in place, as the device optimizer moves them
            self.batch.y = torch.zeros(len(self.batch.sid))
            return self.batch

    def fake_flags(init_batch, final, radii=None):
        calls.append((init_batch.pos.clone(), list(init_batch.sid), final.clone(), radii))
        return torch.zeros(len(init_batch.sid), 4, dtype=torch.bool)

    monkeypatch.setattr(MR, "LBFGS", StubLBFGS)
    monkeypatch.setattr(MR._anomaly, "flag_anomalies", fake_flags)
    b = make_batch(3, n_slab=4, n_ads=1, seed=3)
    out = MR.ml_relax(b.clone(), None, 5, 0.05, {"memory": 7}, False, device="cpu")
    assert not hasattr(out, "anomaly") and not calls
    assert all("flag_anomalies" not in kw and "anomaly_radii" not in kw for kw in kwargs)
    table = np.arange(5.0)
    order = []
    out = MR.ml_relax(b.clone(), None, 5, 0.05, {"memory": 7, "flag_anomalies": True, "anomaly_radii": table}, False,
                      device="cpu", _order=order)
    assert out.sid == ["1", "2", "0"] and order == [1, 2, 0] and len(calls) == 1
    pos0, sids, final, radii = calls[0]
    assert sids == out.sid and radii is table and out.anomaly.shape == (3, 4)
    want = torch.cat([d.pos for d in [b.to_data_list()[i] for i in order]])
    assert torch.equal(pos0, want) and torch.equal(final, want + 1.0) and torch.equal(final, out.pos)
    assert all("flag_anomalies" not in kw and "anomaly_radii" not in kw for kw in kwargs)


def test_ml_relax_sharded_flags_after_the_gather(monkeypatch):
    """The shard relaxes without the option, the flags come from one call on the gathered batch against the positions the
    call was given (the shard moves positions in place), and without the option nothing is computed."""
    from adsorbdiff_amd import sampler

    shard_opts, calls = [], []

    def fake_ml_relax(mine, model, steps, fmax, relax_opt, save_full_traj, device=None, transform=None, _order=None):
        shard_opts.append(dict(relax_opt))
        mine.pos += 1.0                      # in place, as the optimizer does
        _order.extend(range(len(mine.sid)))
        return mine

    def fake_gather(local, ids, natoms, world, via="torch"):
        n = sum(natoms)
        return torch.full((n, 3), 7.0), torch.zeros(len(natoms)), torch.zeros(n, 3)

    def fake_flags(init_batch, final, radii=None):
        calls.append((init_batch.pos.clone(), final.clone(), radii))
        return torch.ones(len(init_batch.sid), 4, dtype=torch.bool)

    monkeypatch.setattr(MR, "ml_relax", fake_ml_relax)
    monkeypatch.setattr(sampler, "gather_relaxed", fake_gather)
    monkeypatch.setattr(MR._anomaly, "flag_anomalies", fake_flags)
    b = make_batch(4, n_slab=4, n_ads=1, seed=3)
    given = b.pos.clone()
    table = np.arange(3.0)
    opt = {"memory": 7, "per_system": True, "flag_anomalies": True, "anomaly_radii": table}
    out = MR.ml_relax_sharded(b, None, 5, 0.05, opt, False, rank=0, world=2, device="cpu")
    assert shard_opts and all(o["flag_anomalies"] is False and o["per_system"] and o["anomaly_radii"] is table for o in shard_opts)
    assert opt["flag_anomalies"] is True                         # the caller's dict is left alone
    assert len(calls) == 1 and out.anomaly.shape == (4, 4) and bool(out.anomaly.all())
    pos0, final, radii = calls[0]
    assert torch.equal(pos0, given) and torch.equal(final, out.pos) and float(final[0, 0]) == 7.0 and radii is table
    out = MR.ml_relax_sharded(make_batch(4, n_slab=4, n_ads=1, seed=3), None, 5, 0.05, {"memory": 7, "per_system": True}, False,
                              rank=0, world=2, device="cpu")
    assert not hasattr(out, "anomaly") and len(calls) == 1 and "flag_anomalies" not in shard_opts[-1]
