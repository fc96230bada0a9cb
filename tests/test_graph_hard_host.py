"""The hard-cell graph cases and their float64 checker (tests/helpers_graph_hard.py) on the CPU: the float32 oracle's own
lists must pass on every case with at most 5 % boundary centres, every case must reach the branch of graph.hip it is in
the table for, and the checker must reject each planted fault.  tests/test_gpu_graph_hard.py runs the same checker on
the device's lists."""
import functools

import numpy as np
import pytest

from tests import helpers_graph_hard as H


@functools.lru_cache(maxsize=None)
def judged(name):
    """(case, oracle graph, stats of check_directed, share) - computed once per case."""
    c = H.case(name)
    g = H.oracle_graph(c)
    b, st = c.batch, {}
    share = H.check_directed(b.pos, b.cell, b.natoms, c.cutoff, c.K, c.pbc, g["cnt"], g["src"], g["shift"], st)
    return c, g, st, share


def directed(c, g):
    b = c.batch
    return H.check_directed(b.pos, b.cell, b.natoms, c.cutoff, c.K, c.pbc, g["cnt"], g["src"], g["shift"])


def symmetrised(c, g):
    b = c.batch
    return H.check_symmetrised(g["cnt"], g["src"], g["shift"], g["es"], g["ed"], g["dist"], g["vec"], b.pos, b.cell, b.natoms)


@pytest.mark.parametrize("name", H.CASES)
def test_oracle_lists_pass_both_checkers(name):
    c, g, st, share = judged(name)
    r = symmetrised(c, g)
    print(f"{name}: boundary share {share:.4f}, worst |dd2|/tau {st['worst']:.3f}, candidates per centre "
          f"{st['in_range'].min()}..{st['in_range'].max()}, E {r['E']}, dist err {r['err_dist']:.2e}, vec err {r['err_vec']:.2e}")
    if name != "close_pair":
        assert share <= H.MAX_BOUNDARY_SHARE, share


def test_cases_reach_their_branches():
    """Shift counts, candidate counts and list lengths of the case table - what makes each case take its branch."""
    C = {n: H.shift_tables(H.case(n).batch.cell, H.case(n).cutoff, H.case(n).pbc) for n in H.CASES}
    want = dict(uncached147=([3, 3, 1], 147), unwrapped147=([3, 3, 1], 147), seam256=([3, 3, 1], 147), k64=([3, 3, 1], 147),
                bulk343=([3, 3, 3], 343), bulk343_k128=([3, 3, 3], 343), near_cap=([3, 3, 3], 343), overflow=([3, 3, 3], 343),
                triclinic245=([3, 3, 2], 245), pbc_ttf=([3, 3, 0], 49), pbc_tff=([3, 0, 0], 7), pbc_fff=([0, 0, 0], 1))
    for n, (reps, count) in want.items():
        assert C[n][0] == reps and C[n][1].shape[0] == count, (n, C[n][0])
    assert max(C["tie"][0]) <= 2
    cand = {n: judged(n)[2]["in_range"] for n in H.CASES}
    assert 896 < cand["near_cap"].max() <= 960                  # T = 15 rounds of 64 in topk_select, below TOPK_CAP
    assert cand["overflow"].min() > 1024                        # every centre is beyond TOPK_CAP
    assert cand["bulk343_k128"].min() > 128 and H.case("bulk343_k128").K == 128
    for n in ("k1", "k64", "k65"):
        assert cand[n].min() > H.case(n).K                      # M > K: the rank selection runs
    assert H.case("seam256").batch.natoms.tolist() == [8, 256, 257]
    one = judged("one_atom")
    assert one[0].batch.natoms.tolist() == [1, 6] and one[1]["cnt"][0] > 0 and np.all(one[1]["src"][0, :one[1]["cnt"][0]] == 0)
    assert cand["pbc_fff"].min() < 20 < cand["pbc_fff"].max()   # lists shorter than K and lists cut at K
    hops = np.abs(np.linalg.solve(H.case("unwrapped147").batch.cell[0].double().numpy().T,
                                  H.case("unwrapped147").batch.pos.double().numpy().T)).max()
    assert hops > 2.0                                           # fractional coordinates far outside [0, 1)
    tri = H.case("triclinic245").batch.cell
    assert bool((tri != 0).all())


def test_close_pair_floor():
    """The 0.009 A partner is absent, the 0.011 A partner present, neither within the band of the 1e-4 floor."""
    c, g, st, _ = judged("close_pair")
    b = c.batch
    for (i, j, d), listed in zip(H.CLOSE_PAIRS, (False, True)):
        for x, y in ((i, j), (j, i)):
            row, u = H.candidate_d2(b.pos, b.cell, b.natoms, c.cutoff, c.pbc, 0, [x])
            _, sh = H.shift_tables(b.cell, c.cutoff, c.pbc)
            zero = int(np.nonzero((sh == 0).all(1))[0][0])
            d2 = row[0, y * sh.shape[0] + zero]
            assert abs(np.sqrt(d2) - d) < 1e-5 and abs(d2 - H.D2_FLOOR) > H.tau(H.D2_FLOOR, u), (x, y, d2)
            k = int(g["cnt"][x])
            has = bool(np.any((g["src"][x, :k] == y) & (g["shift"][x, :k] == 0).all(1)))
            assert has == listed, (x, y, d2)
    assert not st["boundary"][[8, 9, 10, 11]].any()


def test_offsets_exact_on_skew_cells_only():
    """torch.bmm (the oracle, the reference) against the unfused chain of graph.hip: same bits on the project's cell shape
    at every shift - every skew-cell case and `tie`.  The exact-order GPU test relies on this.
    On triclinic245 torch.bmm's bits are a property of the CPU: with one torch build they differed from the chain on one
    x86 host (184 of 735 elements) and equalled it on another (where the exact-order GPU test then collected and passed
    triclinic245 too), so `offsets_exact(triclinic245) is False` cannot be asserted.  What is asserted instead
    holds on every CPU and is the reason for both observations: on the skew cells no offset depends on the order in which
    its three rounded products are summed (at most two are non-zero), on triclinic245 140 of 735 elements do.  The GPU
    test takes its precondition from offsets_exact on the CPU it runs on."""
    for name in H.CASES:
        c = H.case(name)
        exact, free = H.offsets_exact(c), H.offsets_order_dependent(c)
        print(name, "offsets exact:", exact, " order-dependent elements:", free)
        if name == "triclinic245":
            assert free >= 100
        else:
            assert exact and free == 0, name


# ---- the checker must bite
def _copy(g):
    return {k: v.copy() for k, v in g.items()}


def _quiet_centre(name):
    """A centre that is no boundary centre and has more candidates than K."""
    c, g, st, _ = judged(name)
    ok = np.nonzero(~st["boundary"] & (st["in_range"] > c.K + 4))[0]
    return int(ok[0])


def fault_swap_for_farther(name):
    c, g, _, _ = judged(name)
    b, i = c.batch, _quiet_centre(name)
    row, u = H.candidate_d2(b.pos, b.cell, b.natoms, c.cutoff, c.pbc, 0, [i])
    row = row[0]
    reps, sh = H.shift_tables(b.cell, c.cutoff, c.pbc)
    C = sh.shape[0]
    index = {tuple(s): k for k, s in enumerate(sh.tolist())}
    k = int(g["cnt"][i])
    ids = np.array([int(g["src"][i, q]) * C + index[tuple(g["shift"][i, q].tolist())] for q in range(k)])
    far = int(np.argmax(row[ids]))
    dropped = np.setdiff1d(np.nonzero((row > H.D2_FLOOR) & (row <= c.cutoff ** 2))[0], ids)
    dropped = dropped[row[dropped] > row[ids[far]] + 2 * H.tau(row[ids[far]], u)]
    new = int(dropped[np.argmin(row[dropped])])
    g = _copy(g)
    g["src"][i, far], g["shift"][i, far] = new // C, sh[new % C]
    return g


def fault_shift_index(name):
    c, g, _, _ = judged(name)
    reps, _ = H.shift_tables(c.batch.cell, c.cutoff, c.pbc)
    i = _quiet_centre(name)
    q = int(np.nonzero(g["shift"][i, :g["cnt"][i], 2] < reps[2])[0][0])    # stays inside the table
    g = _copy(g)
    g["shift"][i, q, 2] += 1
    return g


def fault_drop(name):
    c, g, _, _ = judged(name)
    i = _quiet_centre(name)
    g = _copy(g)
    g["cnt"][i] -= 1
    return g


def fault_duplicate(name):
    c, g, _, _ = judged(name)
    i = _quiet_centre(name)
    g = _copy(g)
    g["src"][i, 1], g["shift"][i, 1] = g["src"][i, 0], g["shift"][i, 0]
    return g


def fault_swap_records(name):
    c, g, _, _ = judged(name)
    e = int(np.nonzero((g["ed"][1:] == g["ed"][:-1]) & (g["dist"][1:] != g["dist"][:-1]))[0][0])
    g = _copy(g)
    for k in ("es", "dist", "vec"):
        g[k][[e, e + 1]] = g[k][[e + 1, e]]
    return g


def fault_flip_vec(name):
    c, g, _, _ = judged(name)
    g = _copy(g)
    g["vec"][3] = -g["vec"][3]
    return g


@pytest.mark.parametrize("name", ["uncached147", "triclinic245"])
@pytest.mark.parametrize("fault,check", [(fault_swap_for_farther, directed), (fault_shift_index, directed),
                                         (fault_drop, directed), (fault_duplicate, directed),
                                         (fault_swap_records, symmetrised), (fault_flip_vec, symmetrised)],
                         ids=["swap_for_farther", "shift_index", "drop", "duplicate", "swap_records", "flip_vec"])
def test_checker_rejects_planted_fault(name, fault, check):
    c, g, _, _ = judged(name)
    check(c, g)                     # the unharmed lists pass
    bad = fault(name)
    assert any(not np.array_equal(bad[k], g[k]) for k in g)
    with pytest.raises(AssertionError) as info:
        check(c, bad)
    print(name, fault.__name__, "->", str(info.value)[:120])
