"""GPU tests of adf_flag_anomalies / adf_select_best_sites (csrc/anomaly.hip) and their Python layers: every comparison is
exact equality with the float64 oracle of tests/helpers_flag_anomaly.py on systems whose distances stay >= 1e-3 A away from
every threshold (float32 coordinate error there is below 1e-4 A)."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import flag_anomaly as FA
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.ml_relaxation import ml_relax
from tests import helpers_flag_anomaly as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_flags(systems, radii, pbc=None, slab=None, **kw):
    init, final = H.to_batch(systems, pbc=pbc, device=DEV), H.to_batch(systems, final=True, pbc=pbc, device=DEV)
    return FA.flag_anomalies(init, final, slab, radii=radii, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def generated():
    systems, radii = H.generated_systems()
    return systems, radii, _device_flags(systems, radii), H.oracle_batch(systems, radii)


def test_hand_built_cases():
    s, cases = H.co_on_slab()
    systems = [dict(s, final=final) for final, _ in cases.values()]
    got = _device_flags(systems, s["radii"])
    assert got.dtype == bool and got.astype(int).tolist() == [want for _, want in cases.values()]


def test_ragged_batch_equals_the_oracle(generated):
    systems, radii, got, want = generated
    assert got.shape == (48, 4)
    bad = np.nonzero((got != want).any(1))[0].tolist()
    assert not bad, [(k, len(systems[k]["Z"]), systems[k]["mode"], got[k].tolist(), want[k].tolist()) for k in bad]
    assert np.array_equal(want, np.stack([s["flags"] for s in systems]))     # float32 rounding of the inputs changed nothing
    again = _device_flags(systems, radii)
    assert np.array_equal(again, got)


@pytest.mark.parametrize("partners_at", [0, 64, 128])
def test_tiled_slab_reaches_every_tile(partners_at):
    """322 atoms in a hand-chosen order (tests/helpers_flag_anomaly.py, tiled_slab): the only evidence of each flag lies in the
    second j tile of a row tile, or in the last row tile.  Once with a workgroup per row tile, once among one-atom systems
    that bring the launch down to two row-tile slots, so that the six row tiles are reached by the stride alone."""
    s, cases = H.tiled_slab(partners_at)
    systems = [dict(s, final=final) for final, _ in cases.values()]
    want = [w for _, w in cases.values()]
    assert _device_flags(systems, s["radii"]).astype(int).tolist() == want
    one = dict(pos=s["pos"][:1], final=s["pos"][:1], Z=s["Z"][:1], tags=s["tags"][:1], cell=s["cell"])
    mixed = [one] * 20 + systems + [one] * 25
    atoms, count = sum(len(x["Z"]) for x in mixed), len(mixed)
    assert 2 * ((atoms // count + 63) // 64) == 2 < 6          # the launch's row-tile slots against this slab's row tiles
    got = _device_flags(mixed, s["radii"]).astype(int).tolist()
    assert got[20:25] == want and all(g == [0, 1, 0, 0] for g in got[:20] + got[25:])


def test_invariances(generated):
    systems, radii, got, _ = generated
    rng = np.random.default_rng(9)
    moved = []
    for s in systems:       # random atoms moved by integer lattice vectors, in the two frames independently
        m = dict(s)
        for key in ("pos", "final"):
            k = rng.integers(-1, 2, size=(len(s["Z"]), 3)) * (rng.uniform(size=(len(s["Z"]), 1)) < 0.5)
            m[key] = s[key] + k @ s["cell"]
        moved.append(m)
    assert np.array_equal(_device_flags(moved, radii), got)
    perm = rng.permutation(len(systems))
    assert np.array_equal(_device_flags([systems[k] for k in perm], radii), got[perm])
    for k in (0, 1, 2, 11):     # alone = its row in the batch (3 atoms, 328, 171, a small one)
        assert np.array_equal(_device_flags([systems[k]], radii)[0], got[k]), k


def test_small_cell_self_images():
    """2.6 A in-plane edges, one atom per layer: atoms bind their own images and thresholds reach past the first shell."""
    radii = np.zeros(100)
    radii[29], radii[6], radii[8] = 1.3, 0.75, 0.65
    cell = np.array([[2.6, 0.0, 0.0], [0.4, 2.6, 0.0], [0.0, 0.0, 18.0]])
    pos = np.array([[0.0, 0.0, 0.0], [1.3, 1.3, 2.0], [0.0, 0.0, 4.0], [0.3, 0.2, 5.9], [0.3, 0.2, 7.05]])
    base = dict(pos=pos, Z=np.array([29, 29, 29, 6, 8]), tags=np.array([0, 0, 1, 2, 2]), cell=cell)
    finals = [pos, pos + np.array([[0, 0, 0]] * 3 + [[0, 0, 4.0]] * 2), pos + np.array([[0, 0, 0]] * 2 + [[0, 0, 3.4]] + [[0, 0, 3.4]] * 2)]
    systems = [dict(base, final=f) for f in finals]
    for s in systems:
        flags, margin = H.oracle_flags(s["pos"], s["final"], s["Z"], s["tags"], s["cell"], radii)
        assert margin >= H.MIN_MARGIN
    want = H.oracle_batch(systems, radii)
    # the first shell alone is not enough here: (Cu, Cu) cushioned threshold 4.5 A against 2.6 A edges
    assert FA.cell_repeats(torch.tensor(cell, dtype=torch.float32).reshape(1, 3, 3), 4.5)[0] >= 2
    assert want.any() and np.array_equal(_device_flags(systems, radii), want)


def test_final_slab_positions_change_the_surface_test(generated):
    systems, radii, got, _ = generated
    pick = [k for k, s in enumerate(systems) if s["mode"] == "scattered"][:6]
    sub = [systems[k] for k in pick]
    slab = np.concatenate([s["final"][s["tags"] != 2] for s in sub])     # the relaxed slab = the final slab: nothing changed
    want = np.stack([H.oracle_flags(np.float32(s["pos"]).astype(float), np.float32(s["final"]).astype(float), s["Z"], s["tags"],
                                    np.float32(s["cell"]).astype(float), radii,
                                    slab_ref=np.float32(s["final"][s["tags"] != 2]).astype(float))[0] for s in sub])
    with_slab = _device_flags(sub, radii, slab=torch.tensor(slab, dtype=torch.float32))
    assert np.array_equal(with_slab, want) and not with_slab[:, 2].any()
    assert (with_slab[:, 2] != got[pick][:, 2]).any()
    assert np.array_equal(with_slab[:, [0, 1, 3]], got[pick][:, [0, 1, 3]])


def test_degenerate_systems():
    s, cases = H.co_on_slab()
    keep = lambda mask, case: dict(pos=s["pos"][mask], final=cases[case][0][mask], Z=s["Z"][mask], tags=s["tags"][mask],
                                   cell=s["cell"])
    tags, idx = s["tags"], np.arange(len(s["tags"]))
    # no adsorbate; no tag-0 atom; a one-atom adsorbate (twice); a one-atom system (slab atom, adsorbate atom)
    systems = [keep(tags != 2, "surface_changed"), keep(tags != 0, "intercalated"), keep(idx != idx[-1], "unchanged"),
               keep(idx != idx[-1], "desorbed"), keep(idx == 0, "unchanged"), keep(idx == idx[-1], "desorbed")]
    want = H.oracle_batch(systems, s["radii"])
    assert want.astype(int).tolist() == [[0, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]]
    assert np.array_equal(_device_flags(systems, s["radii"]), want)


def test_non_periodic_z():
    """A c-vector short enough that periodic z adds bonds: the (T,T,F) run differs from the all-periodic one."""
    s, cases = H.co_on_slab()
    cell = s["cell"].copy()
    cell[2, 2] = 9.6            # the slab is 5.2 A thick, the CO tops out at 8.25 A: the next image's bottom layer is in reach
    systems = [dict(s, cell=cell, final=final) for final, _ in cases.values()]
    per = H.oracle_batch(systems, s["radii"])
    open_z = H.oracle_batch(systems, s["radii"], pbc=(True, True, False))
    for sy in systems:
        for pbc in ((True, True, True), (True, True, False)):
            assert H.oracle_flags(sy["pos"], sy["final"], sy["Z"], sy["tags"], sy["cell"], s["radii"], pbc=pbc)[1] >= H.MIN_MARGIN
    assert (per != open_z).any()
    assert np.array_equal(_device_flags(systems, s["radii"]), per)
    assert np.array_equal(_device_flags(systems, s["radii"], pbc=(True, True, False)), open_z)


def test_atomic_number_outside_the_table_raises():
    s, cases = H.co_on_slab()
    with pytest.raises(ValueError, match="atomic number outside"):
        _device_flags([dict(s, final=s["pos"])], s["radii"][:20])
    assert _device_flags([dict(s, final=s["pos"])], s["radii"]).astype(int).tolist() == [[0, 0, 0, 0]]    # and works after it


def test_select_best_sites_against_numpy():
    rng = np.random.default_rng(4)
    group = np.concatenate([np.full(5, 3), np.full(1, 9), np.full(130, 4), np.full(4, 17), np.full(3, 20)])
    perm = rng.permutation(len(group))
    group = group[perm]
    energy = rng.normal(size=len(group)).astype(np.float32)
    flags = rng.uniform(size=(len(group), 4)) < 0.15
    flags[group == 17] = [False, True, False, False]                # an all-anomalous group
    tie = np.nonzero(group == 4)[0]
    flags[tie[[7, 60, 99]]] = False
    energy[tie[[7, 60, 99]]] = -50.0                                # an exact tie at the minimum: the lowest index wins
    energy[np.nonzero(group == 20)[0][0]] = np.nan
    flags[group == 20] = False
    energy[np.nonzero(group == 3)[0][1]] = np.nan
    e, f, g = torch.tensor(energy, device=DEV), torch.tensor(flags, device=DEV), torch.tensor(group, device=DEV)
    for fl_np, fl in ((flags, f), (None, None)):
        ids, best, best_e, n_valid = H.best_sites_numpy(energy, fl_np, group)
        got_best, got_e, got_n = FA.best_sites(e, fl, g)
        assert got_best.cpu().tolist() == best.tolist() and got_n.cpu().tolist() == n_valid.tolist()
        assert np.array_equal(got_e.cpu().numpy(), best_e)
    ids, best, _, n_valid = H.best_sites_numpy(energy, flags, group)
    assert best[ids.tolist().index(17)] == -1 and best[ids.tolist().index(4)] == tie[7] and n_valid[ids.tolist().index(20)] == 2


class _Atoms:
    def __init__(self, positions, cell, numbers):
        self.positions, self.cell, self.numbers, self.pbc = positions, cell, numbers, np.array([True, True, True])

    def get_positions(self):
        return self.positions


def test_detect_traj_anomaly_equals_the_batched_call(generated):
    systems, radii, got, _ = generated
    for k in (5, 6, 7):
        s = systems[k]
        det = FA.DetectTrajAnomaly(_Atoms(s["pos"], s["cell"], s["Z"]), _Atoms(s["final"], s["cell"], s["Z"]), s["tags"].tolist(),
                                   radii=radii, device=DEV)
        four = [det.is_adsorbate_dissociated(), det.is_adsorbate_desorbed(), det.has_surface_changed(), det.is_adsorbate_intercalated()]
        assert four == got[k].tolist() and det._flags is not None
    s = systems[7]
    slab = _Atoms(s["final"][s["tags"] != 2], s["cell"], s["Z"][s["tags"] != 2])
    det = FA.DetectTrajAnomaly(_Atoms(s["pos"], s["cell"], s["Z"]), _Atoms(s["final"], s["cell"], s["Z"]), s["tags"].tolist(),
                               final_slab_atoms=slab, radii=radii, device=DEV)
    assert det.has_surface_changed() is False


def test_ml_relax_returns_the_flags_and_changes_nothing_else():
    from tests.helpers import batch_from_fixture
    # the force model, the forced split and the bit comparison of the existing relax tests (private names of that module:
    # a rename there has to be followed here)
    from tests.test_gpu_relax_per_system import _painn, _same, _TwoAtMost

    fx, tr = _painn()
    radii = H.synthetic_radii()
    small = _TwoAtMost(tr)           # forces the split: four systems come back as 2, 3, 0, 1

    def run(**opt):
        b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
        return ml_relax(b, small, steps=int(fx["steps"]), fmax=float(fx["fmax"]),
                        relax_opt={"memory": int(fx["memory"]), "per_system": True, **opt}, save_full_traj=False, device=DEV)

    plain = run()
    flagged = run(flag_anomalies=True, anomaly_radii=radii)
    assert small.refused == 2 and flagged.sid == plain.sid == ["2", "3", "0", "1"]
    assert _same(plain, flagged) and not hasattr(plain, "anomaly")
    assert flagged.anomaly.shape == (4, 4) and flagged.anomaly.dtype == torch.bool and flagged.anomaly.is_cuda
    given = batch_from_fixture(fx, pos_key="pos_in", device=DEV).to_data_list()
    matched = Batch.from_data_list([given[int(s)] for s in flagged.sid])
    assert torch.equal(flagged.anomaly, FA.flag_anomalies(matched, flagged.pos, radii=radii))
