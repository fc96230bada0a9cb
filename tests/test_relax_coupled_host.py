"""CPU tests of the float64 statement of the coupled L-BFGS mode (tests/helpers_lbfgs_coupled.py): against the reference's
teacher-forced records, the layout table, the spread of the search direction between two summation orders (the reference
of the GPU test's tolerance) and a mutation check that shows why the direction has to be compared, not only positions."""
import pytest
import torch

from tests import helpers_lbfgs_coupled as H
from tests.helpers import batch_from_fixture, load_npz


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


@pytest.mark.parametrize("tag", ["ring", "early"])
def test_statement_reproduces_the_references_record(tag):
    fx = _sub(load_npz("relax_teacher.npz"), tag + "_")
    b = batch_from_fixture(fx, pos_key="pos_in")
    st = H.CoupledLBFGS(int(fx["memory"]), float(fx["maxstep"]), float(fx["damping"]), float(fx["alpha"]),
                        early_stop_batch=bool(fx["early"]))
    natoms = fx["natoms"].tolist()
    worst = 0
    for k in range(fx["forces"].shape[0]):
        f = torch.from_numpy(fx["forces"][k])
        mf = torch.stack([H.max_force(x) for x in H.split_systems(f, natoms)])
        mask = mf.ge(float(fx["fmax"]))
        assert torch.equal(mask, torch.from_numpy(fx["masks"][k])), k
        _, absmax, skipped = st.step(k, b.pos, f, b.batch, mask)
        assert skipped == bool(fx["skipped"][k]), (k, float(absmax))
        want = torch.from_numpy(fx["pos_after"][k])
        assert H.ulp_close(b.pos, want), (k, float((b.pos - want).abs().max()))
        worst = max(worst, int((b.pos.view(torch.int32) - want.view(torch.int32)).abs().max()))
    print(f"{tag}: worst position difference {worst} ulp")


def test_layout_is_the_case_table():
    for name, c in H.CASES.items():
        n = 3 * sum(c.natoms)
        G, chunk = H.layout(n)
        assert (G, chunk) == c.layout, name
        assert (G - 1) * chunk < n <= G * chunk, name         # no workgroup is empty
        assert 1 in c.natoms and c.natoms[c.fixed_sys] >= 1
    assert [3 * sum(H.CASES[k].natoms) for k in ("one_wg", "two_wg", "three_wg", "finish_256", "finish_257", "cap")] == \
        [1023, 1026, 2100, 262143, 262146, 1048800]
    assert H.CASES["many_systems"].layout[0] > 1 and len(H.CASES["many_systems"].natoms) == 300
    assert set(H.CASES["many_systems"].natoms) == {1, 2, 3, 4}
    for name in ("three_wg",) + H.BIG:
        assert max(H.CASES[name].natoms) > 512
    # a system seam inside a chunk and a chunk seam inside a system, wherever there is more than one chunk
    for name, c in H.CASES.items():
        G, chunk = c.layout
        seams = {3 * sum(c.natoms[:i]) for i in range(1, len(c.natoms))}
        assert any(s % chunk for s in seams), name
        assert G == 1 or any(g * chunk not in seams for g in range(1, G)), name


def _run(name, memory, early, iterations, other=None, begin=None, script=None):
    """The statement with torch.dot drives the trajectory under harmonic forces; ``other`` (a statement with another dot
    product) takes every step from the driver's positions and forces.  Returns the per-iteration records."""
    inp = H.make_inputs(name)
    gains = H.script_gains(inp, script)
    a = H.CoupledLBFGS(memory, early_stop_batch=early)
    pos = inp.pos.clone()
    rec = []
    for it in range(iterations):
        f = H.harmonic_forces(pos, inp, None if gains is None else gains[it])
        _, mask = H.system_masks(f, inp)
        pos_b = pos.clone()
        za, _, skipped = a.step(it, pos, f, inp.batch, mask)
        r = dict(mask=mask, skipped=skipped, zmax=float(za.abs().max()))
        if other is not None:
            if begin is not None:
                begin(it)
            zb, _, skipped_b = other.step(it, pos_b, f, inp.batch, mask)
            r.update(z_err=H.z_err(zb, za), skipped_b=skipped_b, close=H.ulp_close(pos_b, pos),
                     ulps=int((pos_b.view(torch.int32) - pos.view(torch.int32)).abs().max()))
        rec.append(r)
    return rec


@pytest.fixture(scope="module")
def spreads():
    """key of H.Z_SPREAD -> (largest z spread, worst position ulps) between torch.dot and ShuffledDot over the run's
    combinations, iterations and H.SHUFFLE_SEEDS, measured once."""
    out = {}
    todo = [(name, None, H.runs(name)) for name in H.CASES] + [(name, script, [(3, False, 5)]) for name, script in H.SKIP_RUNS]
    for name, script, runs in todo:
        n = 3 * sum(H.CASES[name].natoms)
        spread, ulps = 0.0, 0
        for memory, early, iterations in runs:
            for seed in H.SHUFFLE_SEEDS:
                rec = _run(name, memory, early, iterations, H.CoupledLBFGS(memory, early_stop_batch=early,
                                                                           dot=H.ShuffledDot(n, seed=seed)), script=script)
                assert all(r["skipped"] == r["skipped_b"] for r in rec), name
                if script is not None:
                    assert [r["skipped"] for r in rec] == [False, False, script == "skip", False, False]
                spread = max(spread, max(r["z_err"] for r in rec))
                ulps = max(ulps, max(r["ulps"] for r in rec))
        key = name if script is None else f"{name}:{script}"
        out[key] = (spread, ulps)
        print(f"{key}: n {n} spread {spread:.2e} positions {ulps} ulp")
    return out


def test_order_spread_is_within_the_stored_numbers(spreads):
    assert set(spreads) == set(H.Z_SPREAD)
    for name, (spread, ulps) in spreads.items():
        assert ulps <= 1, (name, ulps)
        assert 0.0 < spread <= H.Z_SPREAD[name], (name, spread, H.Z_SPREAD[name])


def test_z_tolerance_cap():
    for name in H.Z_SPREAD:
        assert 0.0 < H.z_tol(name) <= H.Z_TOL_CAP, (name, H.z_tol(name))


def test_restated_device_order_is_an_order_of_the_same_sum():
    """Integers sum exactly in any order: every entry of every workgroup is counted once, at each shape of the tree."""
    for n in (1, 255, 1023, 1026, 2100, 262143, 262146, 1048800):
        a = (torch.arange(n, dtype=torch.float64) % 1000.0) - 300.0
        b = (torch.arange(n, dtype=torch.float64) % 7.0) + 1.0
        assert float(H.DeviceOrderDot(n)(a, b)) == float((a.long() * b.long()).sum()), n


@pytest.mark.parametrize("name", list(H.CASES))
def test_inputs_reach_what_the_cases_are_for(name):
    """On the statement's own trajectory (the device's differs by at most an ulp a step): the ring wraps, a mask clears
    during the run and one is still set at the end, in every combination; the all-fixed system's mask is never set."""
    for memory, early, iterations in H.runs(name):
        rec = _run(name, memory, early, iterations)
        masks = torch.stack([r["mask"] for r in rec])
        if memory < 50:
            assert iterations > 2 * memory + 2
        assert bool((masks[:-1] & ~masks[1:]).any()), (name, memory, early)      # a mask cleared during the run
        assert bool(masks[-1].any()), (name, memory, early)
        assert not bool(masks[:, H.CASES[name].fixed_sys].any())
        assert not any(r["skipped"] for r in rec)


@pytest.mark.parametrize("name", list(H.CASES))
def test_a_dropped_entry_shows_in_z_and_not_in_the_positions(name):
    """One alpha dot product of iteration 3 loses the last entry of one chunk: z moves by more than 10 x the case's
    tolerance, every position stays within 1 f32 ulp.  Positions alone would not have noticed."""
    memory, early = H.combos(name)[0][0], name not in H.BIG      # the small cases with early_stop_batch: every system moves
    it = 3
    drop = H.DroppingDot(iteration=it, call=1, entry=H.mutate_entry(name))
    rec = _run(name, memory, early, it + 2, H.CoupledLBFGS(memory, early_stop_batch=early, dot=drop), begin=drop.begin)
    assert drop.dropped == 1
    print(f"{name}: z moved by {rec[it]['z_err']:.2e} (tolerance {H.z_tol(name):.2e}), positions by {rec[it]['ulps']} ulp")
    assert rec[it]["z_err"] > 10.0 * H.z_tol(name), (rec[it]["z_err"], H.z_tol(name))
    assert all(r["close"] for r in rec)
    assert all(r["z_err"] == 0.0 for k, r in enumerate(rec) if k != it)       # alpha is not kept: one iteration only
