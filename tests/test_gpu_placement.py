"""GPU tests of adsorbdiff_amd.placement (csrc/placement.hip) against the float64 oracle of
tests/helpers_placement.py, with injected draws, and of the keyed draws and the hand-off to the later stages.

Tolerances: scaled_normal 1e-9 A (float64 on both sides; the generators' 1e-3 A margin bounds the square root's
amplification near tangency); n_combos exact; positions one float32 ulp of the largest coordinate of the case (the output
rounding and nothing else)."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import flag_anomaly as FA
from adsorbdiff_amd import placement as PL
from tests import helpers_flag_anomaly as HF
from tests import helpers_placement as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADII, MASSES = H.synthetic_radii(), H.synthetic_masses()
HEUR = "random_site_heuristic_placement"
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def placer(seed=0):
    return PL.AdsorbatePlacer(RADII, MASSES, device=DEV, seed=seed)


def run(cases, **kw):
    """Place every case's sites in one call with its own draw rows injected."""
    c0 = cases[0]
    sb = H.slab_batch([c["slab"] for c in cases], device=DEV, pbc=c0["pbc"])
    binding = None if c0["mode"] == "random" else [list(range(len(c["ads"][0]))) for c in cases]
    return sb, placer().place(sb, [c["ads"] for c in cases], [c["sites"] for c in cases], c0["n_aug"], c0["gap"], c0["mode"],
                              binding, draws=np.concatenate([c["rows"] for c in cases]), **kw)


def check(cases, out):
    oracle = [o for c in cases for o in c["oracle"]]
    P = len(oracle)
    assert int(out.natoms.numel()) == P
    sn, nc, meta = out.scaled_normal.cpu().numpy(), out.n_combos.cpu().numpy(), out.xyz_angles.cpu().numpy()
    pos, tags, batch = out.pos.cpu().numpy(), out.tags.cpu().numpy(), out.batch.cpu().numpy()
    worst_sn = worst_pos = 0.0
    for p, o in enumerate(oracle):
        assert nc[p] == o["n_combos"], (p, nc[p], o["n_combos"])
        worst_sn = max(worst_sn, abs(sn[p] - o["scaled_normal"]))
        assert np.abs(meta[p] - o["meta"]).max() <= 1e-12
        got = pos[(batch == p) & (tags == 2)].astype(np.float64)
        assert got.shape == o["pos"].shape
        ulp = float(np.spacing(np.float32(np.abs(o["pos"]).max())))
        err = float(np.abs(got - o["pos"]).max())
        worst_pos = max(worst_pos, err / ulp)
        assert err <= ulp, (p, err, ulp)
    print(f"placements {P}: |scaled_normal - oracle| <= {worst_sn:.2e} A, positions within {worst_pos:.2f} ulp")
    assert worst_sn <= 1e-9, worst_sn


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n_slab,n_ads", [(1, 1), (H.WAVE - 1, 1), (H.WAVE, 1), (H.WAVE + 1, 1), (200, 7)])
def test_one_placement_against_the_oracle(n_slab, n_ads):
    """B = 1, P = 1.  The kernel's per-step tile is 64 slab atoms (one per lane): 63, 64 and 65 atoms x a one-atom adsorbate
    are the pair counts one below, at and one above it; 7 x 200 = 1400 pairs takes four strides of seven pairs a lane."""
    c = H.draw_case(np.random.default_rng(100 + n_slab), n_slab, n_ads, RADII, MASSES)
    sb, out = run([c])
    check([c], out)
    assert out.pos.shape[0] == n_slab + n_ads and out.site_group.tolist() == [0]


def ragged_cases(mode="random"):
    def make():
        rng = np.random.default_rng(7 if mode == "random" else 8)
        shapes = [(1, 5), (200, 7), (37, 1), (64, 2), (129, 5), (12, 2)]
        return [H.draw_case(rng, ns, na, RADII, MASSES, n_sites=3, n_aug=2, mode=mode, left_handed=(k == 4))
                for k, (ns, na) in enumerate(shapes)]
    return memo(("ragged", mode), make)


def test_ragged_batch_against_the_oracle():
    """6 slabs of 1 to 200 atoms with different adsorbates, 3 sites x 2 augmentations each; slab 4 is left-handed."""
    cases = ragged_cases()
    sb, out = run(cases)
    check(cases, out)
    assert H.normal(H.f32(cases[4]["slab"]["cell"]))[2] < 0
    assert out.site_group.tolist() == [b for b in range(6) for _ in range(6)]
    assert torch.equal(out.site.cpu(), torch.tensor(np.repeat(np.concatenate([c["sites"] for c in cases]), 2, 0), dtype=torch.float32))
    assert out.sid == [f"slab{b}" for b in range(6) for _ in range(6)] and out.pbc.tolist() == [[True, True, False]] * 36


def test_hand_built_cases_against_the_oracle():
    rng = np.random.default_rng(9)
    last, hole, seam = H.last_atom_case(RADII, MASSES, rng), H.hole_case(RADII, MASSES, rng), H.wrap_only_case(RADII, MASSES, rng)
    # the only colliding slab atom is the last one of the slab
    assert last["oracle"][0]["n_combos"] == 1 and last["oracle"][0]["counted"][0, -1]
    # over a hole
    assert hole["oracle"][0]["n_combos"] == 0
    # collides through the wrap only: without it the oracle counts nothing
    s = seam["slab"]
    unwrapped = H.place_oracle(s["pos"], s["Z"], s["cell"], H.PBC, *seam["ads"], seam["sites"][0], seam["rows"][0], RADII, MASSES,
                               0.1, do_wrap=False)
    assert seam["oracle"][0]["n_combos"] == 1 and unwrapped["n_combos"] == 0
    for c in (last, hole, seam):
        check([c], run([c])[1])
    sb, out = run([hole])
    assert float(out.scaled_normal[0]) == 0.0 and torch.equal(out.pos[-1].cpu(), torch.tensor(hole["sites"][0], dtype=torch.float32))


def test_heuristic_placement_mode_with_other_binding_atoms():
    cases = ragged_cases(HEUR)
    for c in cases:   # the binding pick of every row selects the oracle's binding atom from range(n_ads)
        c["rows"][:, 6] = (c["binding"] + 0.5) / len(c["ads"][0])
    assert sum(int((c["binding"] != 0).sum()) for c in cases) >= 10
    sb, out = run(cases)
    check(cases, out)
    assert out.binding_idx.tolist() == [int(b) for c in cases for b in c["binding"]]
    assert all(o["meta"][3] >= H.COS_CONE for c in cases for o in c["oracle"] if len(c["ads"][0]) > 1)
    with pytest.raises(ValueError, match="binding_indices"):
        placer().place(sb, [c["ads"] for c in cases], [c["sites"] for c in cases], mode=HEUR)


def large_cases():
    def make():
        rng = np.random.default_rng(17)
        return [H.draw_case(rng, ns, na, RADII, MASSES, n_sites=3, n_aug=2) for ns, na in [(200, 7), (150, 2), (180, 5)]]
    return memo("large", make)


def test_device_output_touches_at_the_gap():
    """interstitial_distances over all slab atoms (every slab atom tagged 1) is the gap within 1e-5 A: the float32 rounding
    of the coordinates propagated to a distance.  The slabs are 20 A wide, so the frame centred on the adsorbate's mass
    centre holds the same slab images as the frame centred on the site."""
    cases = large_cases()
    sb, out = run(cases)
    assert int((out.n_combos > 0).sum()) == len(out.n_combos)
    out.tags = torch.where(out.tags == 2, out.tags, torch.ones_like(out.tags))
    d = PL.interstitial_distances(out, RADII, MASSES).cpu().numpy().astype(np.float64)
    print("interstitial distance - gap:", np.abs(d - 0.1).max())
    assert np.abs(d - float(np.float32(0.1))).max() <= 1e-5
    assert not PL.there_is_overlap(out, RADII, MASSES).any()


def test_interstitial_distances_against_the_oracle():
    """Placed systems as they are (touching, with the gap as margin), pushed 1.5 A towards the surface (overlapping), and
    without a surface atom (+inf); mixed tags 0 / 1 / 2 and the periodic flags of the placements (T, T, F)."""
    cases = large_cases()
    sb, out = run(cases)
    P = int(out.natoms.numel())
    pos = out.pos.clone()
    n = torch.tensor(np.stack([o["n"] for c in cases for o in c["oracle"]]), dtype=torch.float32, device=DEV)
    pushed = (out.tags == 2) & (out.batch % 3 == 1)
    pos[pushed] -= 1.5 * n[out.batch[pushed]]
    tags = out.tags.clone()
    tags[(out.batch % 3 == 2) & (tags == 1)] = 0
    out.pos, out.tags = pos, tags
    d = PL.interstitial_distances(out, RADII, MASSES).cpu().numpy()
    over = PL.there_is_overlap(out, RADII, MASSES).cpu().numpy()
    pos_h, Z, tg, bt, cell = pos.cpu().numpy(), out.atomic_numbers.cpu().numpy(), tags.cpu().numpy(), out.batch.cpu().numpy(), out.cell.cpu().numpy()
    compared = 0
    for p in range(P):
        m = bt == p
        want, seam = H.interstitial_oracle(pos_h[m], Z[m], tg[m], cell[p], (True, True, False), RADII, MASSES)
        if p % 3 == 2:
            assert want == np.inf and d[p] == np.inf and not over[p]
            continue
        if seam < H.MIN_SEAM_MARGIN:     # an atom within rounding of the seam may take either image
            continue
        assert abs(float(d[p]) - want) <= 1e-6 * max(1.0, abs(want)), (p, d[p], want)   # float32 output of a float64 value
        assert bool(over[p]) == (want < 0)
        compared += 1
    assert compared >= P // 2 and over[1::3].any() and not over[0::3].any()


# ------------------------------------------------------------------------------------------------ candidate sites
def site_slabs():
    def make():
        rng = np.random.default_rng(31)
        return [H.make_slab(rng, 40, 70.0), H.make_slab(rng, 90, 115.0, left_handed=True)]
    return memo("site_slabs", make)


@pytest.mark.parametrize("num_sites", [1, 5, 40])
def test_candidates_and_selection_against_the_oracle(num_sites):
    """Two slabs with hand-built triangle tables (32 and 50 triangles, a ring of lattice cells outside the central cell).
    40 sites are more than are kept on the first slab: a ragged, shorter result."""
    slabs = site_slabs()
    tris = [H.lattice_triangles(H.f32(slabs[0]["cell"]), 2, slabs[0]["top"]), H.lattice_triangles(H.f32(slabs[1]["cell"]), 3, slabs[1]["top"])]
    per = [H.per_triangle(num_sites, len(t)) for t in tris]
    rng = np.random.default_rng(40 + num_sites)
    rows = [H.candidate_rows(rng, t, p, s["cell"]) for t, p, s in zip(tris, per, slabs)]
    st = placer().sites(H.slab_batch(slabs, device=DEV), num_sites, triangles=tris, draws=np.concatenate(rows))
    cand, keep = st.candidates.cpu().numpy().astype(np.float64), st.keep.cpu().numpy()
    start, want_sites, want_slab = 0, [], []
    for b, (t, p, s, r) in enumerate(zip(tris, per, slabs, rows)):
        oc, ok, margin = H.candidates_oracle(t, p, s["cell"], r)
        n = len(oc)
        assert margin >= H.MIN_SEAM_MARGIN and n == len(t) * p
        ulp = np.spacing(np.abs(oc).max(axis=1).astype(np.float32)).astype(np.float64)[:, None]
        assert (np.abs(cand[start:start + n] - oc) <= ulp).all()
        assert np.array_equal(keep[start:start + n], ok)
        sel = H.select_oracle(ok, r[:, 2], num_sites)
        assert st.counts[b] == len(sel)
        want_sites.append(cand[start + sel])
        want_slab += [b] * len(sel)
        start += n
    assert start == len(cand)
    assert np.array_equal(st.pos.cpu().numpy().astype(np.float64), np.concatenate(want_sites)) and st.slab.tolist() == want_slab
    assert all(c <= num_sites for c in st.counts)
    if num_sites == 40:
        assert st.counts[0] < 40


# ------------------------------------------------------------------------------------------------ keyed draws
def test_keyed_draws_follow_the_slab():
    """Slab X (noise_key 77) gets bit-identical sites, orientations and positions alone, as member 0 and as member 4 of a
    batch, and with the batch reversed; two runs are bit-identical; another seed differs."""
    rng = np.random.default_rng(51)
    X = H.make_slab(rng, 60, 80.0)
    others = [H.make_slab(rng, n) for n in (20, 75, 33, 48)]
    tri = lambda s: H.lattice_triangles(H.f32(s["cell"]), 2, s["top"])
    ads_X, ads_o = H.make_adsorbate(rng, 5), H.make_adsorbate(rng, 2)

    def go(slabs, keys, seed=0):
        k = keys.index(77)
        pl = placer(seed)
        sb = H.slab_batch(slabs, device=DEV, keys=keys)
        st = pl.sites(sb, 4, triangles=[tri(s) for s in slabs])
        out = pl.place(sb, [ads_X if i == k else ads_o for i in range(len(slabs))], st, 2)
        mine = out.site_group == k
        atoms = mine[out.batch] & (out.tags == 2)
        return st.pos[st.slab == k].cpu(), out.xyz_angles[mine].cpu(), out.pos[atoms].cpu(), out.scaled_normal[mine].cpu()

    alone = go([X], [77])
    assert alone[0].shape == (4, 3) and alone[1].shape == (8, 4) and alone[2].shape == (40, 3)
    first = go([X] + others, [77, 1, 2, 3, 4])
    fifth = go(others + [X], [1, 2, 3, 4, 77])
    rev = go(([X] + others)[::-1], [77, 1, 2, 3, 4][::-1])
    again = go([X], [77])
    for other in (first, fifth, rev, again):
        for a, b in zip(alone, other):
            assert torch.equal(a, b)
    different = go([X], [77], seed=1)
    assert not torch.equal(alone[0], different[0]) and not torch.equal(alone[1], different[1])
    assert len(torch.unique(alone[1][:, 0])) == 8          # every augmentation has its own orientation


# ------------------------------------------------------------------------------------------------ hand-off
def test_hand_off_to_flags_ranking_and_the_sampler():
    from adsorbdiff_amd.denoising_torch import Denoiser, DiffTorchCalc
    from adsorbdiff_amd.painn_denoising import PaiNN
    from adsorbdiff_amd.trainer import DenoisingTrainer

    cases = large_cases()
    sb, out = run(cases)
    P = int(out.natoms.numel())
    # the slab rows, tags, fixed and natoms are the inputs' bit for bit
    n_ads = [len(c["ads"][0]) for c in cases]
    for p in range(P):
        b = p // 6
        m, ms = out.batch == p, sb.batch == b
        k = int(ms.sum())
        assert int(out.natoms[p]) == k + n_ads[b]
        assert torch.equal(out.pos[m][:k], sb.pos[ms]) and torch.equal(out.tags[m][:k], sb.tags[ms])
        assert torch.equal(out.fixed[m][:k], sb.fixed[ms]) and torch.equal(out.atomic_numbers[m][:k], sb.atomic_numbers[ms])
        assert (out.tags[m][k:] == 2).all() and (out.fixed[m][k:] == 0).all()
        assert out.atomic_numbers[m][k:].tolist() == cases[b]["ads"][0].tolist() and torch.equal(out.cell[p], sb.cell[b])
    # flags of the unrelaxed placement against itself: nothing dissociates or reconstructs, every adsorbate is bound at
    # the gap; "intercalated" is what the geometry dictates (the anomaly oracle, where its margin clears rounding)
    flags = FA.flag_anomalies(out, out, radii=RADII).cpu().numpy()
    assert (out.n_combos > 0).all() and not flags[:, [0, 1, 2]].any()
    pos, Z, tg, bt = (t.cpu().numpy() for t in (out.pos, out.atomic_numbers, out.tags, out.batch))
    for p in range(0, P, 5):
        m = bt == p
        want, margin = HF.oracle_flags(pos[m], pos[m], Z[m], tg[m], out.cell[p].cpu().numpy(), RADII, pbc=(True, True, False))
        if margin >= HF.MIN_MARGIN:
            assert flags[p].tolist() == want.tolist()
    # ranking per slab
    energy = torch.randn(P, generator=torch.Generator().manual_seed(5)).to(DEV)
    best, best_e, n_valid = FA.best_sites(energy, torch.as_tensor(flags).to(DEV), out.site_group)
    ids, wb, we, wn = HF.best_sites_numpy(energy.cpu().numpy(), flags, out.site_group.cpu().numpy())
    assert best.tolist() == wb.tolist() and n_valid.tolist() == wn.tolist() and ids.tolist() == [0, 1, 2]
    # one sampler step of a tiny PaiNN: the sampled adsorbate keeps the placed centre's z
    torch.manual_seed(3)
    model = PaiNN(None, 50, 1, hidden_channels=128, num_layers=1, num_rbf=128, cutoff=6.0, max_neighbors=20,
                  so3_denoising=True).to(DEV).eval()
    params = dict(num_steps=2, ads_std_low=0.1, ads_std_high=10, rot_std_low=0.01, rot_std_high=1.55, early_stop=False)
    start = out.clone()
    start.atomic_numbers = (start.atomic_numbers - 1) % 83 + 1      # the tiny model embeds 83 elements
    den = Denoiser(start, DiffTorchCalc(DenoisingTrainer(model, device=DEV)), params, device=DEV)
    sampled = den.run()
    ads = out.tags == 2
    cnt = torch.zeros(P, device=DEV).index_add_(0, out.batch[ads], torch.ones(int(ads.sum()), device=DEV))
    zc = lambda b: torch.zeros(P, device=DEV).index_add_(0, out.batch[ads], b.pos[ads][:, 2]) / cnt
    assert torch.isfinite(sampled.pos).all() and torch.equal(sampled.pos[~ads], out.pos[~ads])
    assert not torch.equal(sampled.pos[ads], out.pos[ads])
    assert float((zc(sampled) - zc(out)).abs().max()) < 1e-3


def test_atomic_number_outside_the_tables_is_an_error():
    c = H.draw_case(np.random.default_rng(61), 30, 2, RADII, MASSES)
    sb = H.slab_batch([c["slab"]], device=DEV)
    sb.atomic_numbers[-1] = 150
    with pytest.raises(ValueError, match="atomic number outside"):
        placer().place(sb, c["ads"], [c["sites"]], draws=c["rows"])
    sb.atomic_numbers[-1] = 29
    with pytest.raises(ValueError, match="atomic number outside"):
        placer().place(sb, (np.array([6, 120]), c["ads"][1]), [c["sites"]], draws=c["rows"])
    out = placer().place(sb, c["ads"], [c["sites"]], draws=c["rows"])
    out.atomic_numbers[0] = -3
    out.tags[0] = 1
    with pytest.raises(ValueError, match="atomic number outside"):
        PL.interstitial_distances(out, RADII, MASSES)


def test_a_candidate_of_a_slab_outside_the_batch_is_refused():
    """The range bit of the placement error word, through the raw entry (the wrapper builds cand_slab itself): the
    kernel tests the slab index before it indexes any per-slab array with it, zeroes the candidate's own row and reports."""
    from adsorbdiff_amd import lib as L
    tri = torch.tensor([[0.0, 0.0, 5.0, 1.0, 0.0, 5.0, 0.0, 1.0, 5.0]], device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    tri_off, per_tri, cand_off, cell = i32([0, 1]), i32([2]), i32([0, 2]), torch.eye(3, device=DEV).mul(4.0).reshape(1, 9).contiguous()
    draws = torch.full((2, 8), 0.25, dtype=torch.float64, device=DEV)
    for slab, status in (([0, 0], L.ADF_OK), ([0, 1], L.ADF_EINVAL), ([-1, 0], L.ADF_EINVAL)):
        cand, keep, cand_slab = torch.full((2, 3), -7.0, device=DEV), i32([-7, -7]), i32(slab)
        got = L.load().adf_place_site_candidates(tri.data_ptr(), tri_off.data_ptr(), per_tri.data_ptr(), cand_off.data_ptr(),
                                                 cand_slab.data_ptr(), cell.data_ptr(), draws.data_ptr(), 1, 2, cand.data_ptr(),
                                                 keep.data_ptr(), None)
        torch.cuda.synchronize()
        assert got == status, (slab, L.load().adf_last_error())
        if status != L.ADF_OK:
            assert b"place_site_candidates: an offset, slab index or output row out of range" in L.load().adf_last_error()
            bad = slab.index(1) if 1 in slab else slab.index(-1)
            assert keep.tolist()[bad] == 0 and cand[bad].tolist() == [0.0, 0.0, 0.0]


def test_a_binding_index_outside_the_adsorbate_is_refused():
    """The binding bit of the placement error word, through the raw entry (the wrapper refuses such an index itself): one
    slab of four atoms, one adsorbate of two, heuristic placement.  pl_place_kernel replaces the index by 0 before it
    reads ads_pos with it, and an atomic number outside the radius table by row 0, so nothing is indexed out of range.
    The bit outranks the atomic-number bit in the message."""
    import ctypes as C

    from adsorbdiff_amd import lib as L
    from adsorbdiff_amd.hostargs import desc
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    slab_pos = torch.tensor([[0.0, 0.0, 5.0], [2.0, 0.0, 5.0], [0.0, 2.0, 5.0], [2.0, 2.0, 5.0]], device=DEV)
    cell = torch.tensor([[4.0, 0.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 20.0]], device=DEV)
    slab_Z, slab_off = i32([29, 29, 29, 29]), i32([0, 4])
    d = desc(slab_pos, cell, slab_Z, slab_off, 1, 4)
    site = torch.tensor([[1.0, 1.0, 5.0]], device=DEV)
    draws = torch.full((1, 8), 0.25, dtype=torch.float64, device=DEV)
    ads_off, ads_pos = i32([0, 2]), torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 1.1]], device=DEV)
    radii, masses = torch.ones(120, device=DEV), torch.ones(120, device=DEV)
    slab_of, pbc, out_row = i32([0]), i32([[1, 1, 0]]), i32([0])
    for bind, ads_Z, status in ((1, [6, 8], L.ADF_OK), (2, [6, 8], L.ADF_EINVAL), (-1, [6, 8], L.ADF_EINVAL),
                                (2, [6, 500], L.ADF_EINVAL)):
        b, z = i32([bind]), i32(ads_Z)
        out = torch.full((2, 3), -7.0, device=DEV)
        sn = torch.zeros(1, dtype=torch.float64, device=DEV)
        nc, meta = i32([0]), torch.zeros(1, 4, dtype=torch.float64, device=DEV)
        got = L.load().adf_place_adsorbates(C.byref(d), slab_of.data_ptr(), site.data_ptr(), draws.data_ptr(), ads_off.data_ptr(),
                                            ads_pos.data_ptr(), z.data_ptr(), radii.data_ptr(), 120, masses.data_ptr(), 120,
                                            C.c_float(0.1), 1, b.data_ptr(), pbc.data_ptr(), 1, out_row.data_ptr(), 2,
                                            out.data_ptr(), sn.data_ptr(), nc.data_ptr(), meta.data_ptr(), None)
        torch.cuda.synchronize()
        assert got == status, (bind, ads_Z, L.load().adf_last_error())
        if status != L.ADF_OK:
            assert b"place_adsorbates: binding_idx outside the adsorbate" in L.load().adf_last_error(), (bind, ads_Z)


def test_adsorbate_slab_config_interface():
    """The reference's keyword names on duck-typed objects: given sites are placed as ``place`` places them; sampled
    sites come from the triangle table."""
    from types import SimpleNamespace as NS

    c = ragged_cases(HEUR)[3]
    s = c["slab"]
    atoms = NS(positions=H.f32(s["pos"]), cell=H.f32(s["cell"]), numbers=s["Z"], tags=s["tags"], pbc=[True, True, True])
    ads = NS(atoms=NS(positions=H.f32(c["ads"][1]), numbers=c["ads"][0]), binding_indices=[1])
    kw = dict(radii=RADII, masses=MASSES, device=DEV, seed=4)
    cfg = PL.AdsorbateSlabConfig(NS(atoms=atoms), ads, num_sites=3, num_augmentations_per_site=2, interstitial_gap=0.1,
                                 mode=HEUR, sites=c["sites"], **kw)
    assert np.array_equal(cfg.sites, c["sites"]) and len(cfg.metadata_list) == 6     # the given sites, as given
    sb = H.slab_batch([s], device=DEV, pbc=H.PBC)
    sb.sid = None
    want = placer(4).place(sb, c["ads"], [c["sites"]], 2, 0.1, HEUR, [1])
    assert torch.equal(cfg.batch.pos, want.pos) and (cfg.batch.binding_idx == 1).all()
    for p, m in enumerate(cfg.metadata_list):
        assert np.array_equal(m["site"], H.f32(c["sites"][p // 2]))
        assert m["xyz_angles"][0] == float(want.xyz_angles[p, 0]) and np.array_equal(m["xyz_angles"][1], want.xyz_angles[p, 1:].cpu().numpy())
    tri = H.lattice_triangles(H.f32(s["cell"]), 2, s["top"])
    cfg = PL.AdsorbateSlabConfig(NS(atoms=atoms), ads, num_sites=4, mode="random", triangles=tri, **kw)
    assert cfg.sites.shape == (4, 3) and int(cfg.batch.natoms.numel()) == 4 and H.keep_rule(cfg.sites, H.f32(s["cell"]))[0].all()
    with pytest.raises(ValueError):
        PL.AdsorbateSlabConfig(NS(atoms=atoms), ads, mode="heuristic", **kw)
