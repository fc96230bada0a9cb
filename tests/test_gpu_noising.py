"""Device noising (csrc/noising.hip) against its host functions: the counter-based draws against the numpy Philox
reference, adf_noise_tr_so3 / adf_noise_com against noising.*_from_draws, adf_igso3_score_norm against
Igso3Tables.score_norm.  Bound: rtol = atol = 2e-5, what tests/test_oracle_golden.py grants the host mirror against the
reference.  The wraps have jumps; tests/helpers_tr_only.py::safe_rows keeps the chosen rows 1e-4 away from them in float64
(at most one row in ten may need its one redraw)."""
import numpy as np
import pytest
import torch

from adsorbdiff_amd import noising
from adsorbdiff_amd.so3_tables import Igso3Tables
from tests import helpers_tr_only as HO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=2e-5, atol=2e-5)


@pytest.fixture(scope="module")
def tables():
    return Igso3Tables.shared()


@pytest.fixture(scope="module")
def batches():
    return HO.noising_batches()


def test_draws_equal_the_numpy_philox_reference_and_depend_on_the_key_alone():
    rng = np.random.RandomState(5)
    keys = np.concatenate([rng.randint(0, 2**31, size=12), rng.randint(2**32, 2**62, size=12, dtype=np.int64),
                           -rng.randint(1, 2**62, size=10, dtype=np.int64), [0, 2**32 - 1, 2**32]]).astype(np.int64)
    assert keys.size == 37 and (np.abs(keys) >= 2**32).sum() > 10 and (np.abs(keys) < 2**32).sum() > 10
    tk = torch.from_numpy(keys)
    for seed in (0, (3 << 40) + 17):
        nz = noising.DeviceNoiser(HO.PARAMS, None, DEV, seed=seed)
        per_step = []
        for step in (0, 7):
            got = nz.draws(step, tk).cpu().numpy()
            want = HO.reference_draws(seed, step, keys)
            err = float(np.abs(got - want).max())
            print(f"draws seed {seed} step {step}: max |device - numpy| = {err:.2e}")
            assert got.shape == (37, 8) and err <= 1e-12
            # permuted, split in two, one system alone: the row follows the key
            perm = rng.permutation(37)
            assert np.array_equal(nz.draws(step, tk[perm]).cpu().numpy(), got[perm])
            halves = np.concatenate([nz.draws(step, tk[:20]).cpu().numpy(), nz.draws(step, tk[20:]).cpu().numpy()])
            assert np.array_equal(halves, got)
            assert np.array_equal(nz.draws(step, tk[33:34]).cpu().numpy(), got[33:34])
            per_step.append(got)
        assert not np.array_equal(per_step[0], per_step[1])
    with pytest.raises(ValueError, match="int64"):
        nz.draws(0, torch.arange(3, dtype=torch.int32))


def _compare(got, want, keys, label):
    for key in keys:
        g, w = getattr(got, key).detach().cpu().numpy(), getattr(want, key).detach().cpu().numpy()
        assert g.shape == w.shape, (label, key, g.shape, w.shape)
        print(f"{label} {key}: max abs diff {float(np.abs(g - w).max()):.2e}")
        np.testing.assert_allclose(g, w, err_msg=f"{label} {key}", **TOL)


TR_SO3_KEYS = ("pos", "tr_sigma", "rot_sigma", "tr_score", "rot_score", "ads_center_noise_vec")


@pytest.mark.parametrize("name", ["ragged", "big_adsorbate", "single", "interleaved", "skewed"])
def test_tr_so3_kernel_vs_host_function(name, tables, batches):
    b0 = batches[name]
    B = int(b0.natoms.numel())
    rows, redrawn = HO.safe_rows(b0, HO.PARAMS, seed=40, kinds=("tr_so3",))
    assert redrawn <= max(1, B // 10), redrawn
    want = noising.tr_so3_schedule_from_draws(b0.clone(), HO.PARAMS, rows, tables)
    nz = noising.DeviceNoiser(HO.PARAMS, tables, DEV, seed=1)
    bd = b0.clone().to(DEV)
    pos_in = bd.pos
    keep = pos_in.clone()
    got = nz.tr_so3(bd, draws=rows)
    _compare(got, want, TR_SO3_KEYS, name)
    assert got.pos.data_ptr() != pos_in.data_ptr() and torch.equal(pos_in, keep)   # a copy; the input is untouched
    off = (b0.tags != 2)
    assert torch.equal(got.pos.cpu()[off], b0.pos[off])                            # bit-equal off the adsorbate
    assert not torch.equal(got.pos.cpu()[~off], b0.pos[~off])
    np.testing.assert_array_equal(got.rot_norm.cpu().numpy(), tables.score_norm(want.rot_sigma.reshape(-1)).numpy())
    assert got.tr_sigma.shape == (B, 1) and got.rot_sigma.shape == (B, 1) and got.rot_norm.shape == (B,)
    # the generator path gives what the rows of the same (seed, step, keys) give
    keys = noising.noise_keys(b0)
    own = nz.tr_so3(b0.clone().to(DEV), step=3)
    replay = nz.tr_so3(b0.clone().to(DEV), draws=nz.draws(3, keys))
    assert torch.equal(own.pos, replay.pos) and torch.equal(own.rot_score, replay.rot_score)


def test_tr_so3_kernel_reaches_both_table_clips_and_both_end_branches(tables, batches):
    """rot_std 1e-3 .. 3.0: sigma_rot below the first and above the last eps row (both eps_index clips).  Supplied u_om = 0
    takes the angle look-up's lower end branch.  The supplied u_om = 1 - 1e-12 is kept, but on the real tables it is an
    interior look-up: every row's CDF ends at 1 - 6.3e-14 or above (up to 1.0005), so the upper end branch needs
    u_om >= 1, which the generator never draws; a third supplied row (u_om = the end of its CDF row, at least 1) takes it."""
    b0 = batches["ragged"]
    P = HO.PARAMS_WIDE_ROT
    rows, redrawn = HO.safe_rows(b0, P, seed=41, kinds=("tr_so3",))
    assert redrawn <= 1
    rows[0, 0], rows[1, 0] = 0.05, 0.99        # t: sigma_rot = 1.5e-3 and 2.77
    rows[2, 7], rows[3, 7] = 0.0, 1.0 - 1e-12
    rows[0, 7] = max(1.0, float(tables.cdf[0, -1]))   # system 0 reads eps row 0 (asserted below)
    assert (HO.boundary_margin(b0, P, rows, "tr_so3") >= HO.MARGIN).all()
    want = noising.tr_so3_schedule_from_draws(b0.clone(), P, rows, tables)
    sig = want.rot_sigma.reshape(-1).double().numpy()
    raw = (np.log10(sig) - np.log10(0.01)) / (np.log10(2) - np.log10(0.01)) * 1000
    assert raw[0] < -1 and raw[1] > 1000, raw
    idx = tables.eps_index(sig)
    assert idx[0] == 0 and idx[1] == 999
    assert rows[2, 7] < tables.cdf[idx[2], 0] and rows[0, 7] >= tables.cdf[idx[0], -1], "the end branches are not reached"
    om = np.linalg.norm(want.rot_score.double().numpy(), axis=1)   # |score| = |table value| at the ends
    assert np.isclose(om[2], abs(tables.score[idx[2], 0]), rtol=1e-6) and np.isclose(om[0], abs(tables.score[0, -1]), rtol=1e-6)
    got = noising.DeviceNoiser(P, tables, DEV).tr_so3(b0.clone().to(DEV), draws=rows)
    _compare(got, want, TR_SO3_KEYS, "wide rot")
    np.testing.assert_array_equal(got.rot_norm.cpu().numpy(), tables.score_norm(want.rot_sigma.reshape(-1)).numpy())


@pytest.mark.parametrize("name", ["ragged", "big_adsorbate", "single", "interleaved", "skewed"])
def test_com_kernel_vs_host_function(name, batches):
    b0 = batches[name]
    B = int(b0.natoms.numel())
    rows, redrawn = HO.safe_rows(b0, HO.PARAMS, seed=50, kinds=("com",))
    assert redrawn <= max(1, B // 10), redrawn
    want = noising.ads_COM_gaussian_schedule_from_draws(b0.clone(), HO.PARAMS, rows)
    nz = noising.DeviceNoiser(HO.PARAMS, None, DEV, seed=1)
    bd = b0.clone().to(DEV)
    keep = bd.pos.clone()
    pos_in = bd.pos
    got = nz.com(bd, draws=rows)
    _compare(got, want, ("pos", "tr_sigma", "tr_score", "ads_center_noise_vec"), name)
    assert torch.equal(pos_in, keep)
    off = (b0.tags != 2)
    pos = got.pos.cpu()
    assert torch.equal(pos[off], b0.pos[off])
    for s in range(B):   # all adsorbate atoms of a system end on one point
        mine = pos[(~off) & (b0.batch == s)]
        assert mine.shape[0] > 0 and bool((mine == mine[0]).all())
    # one key gives the same t under both schedules
    keys = noising.noise_keys(b0)
    a = nz.com(b0.clone().to(DEV), step=2, keys=keys)
    t = nz.draws(2, keys)[:, 0].float()
    so3 = noising.DeviceNoiser(HO.PARAMS, Igso3Tables.shared(), DEV, seed=1).tr_so3(b0.clone().to(DEV), step=2, keys=keys)
    assert torch.equal(a.tr_sigma, so3.tr_sigma)
    assert torch.allclose(a.tr_sigma.reshape(-1), 0.1 ** (1 - t) * 10 ** t, rtol=2e-5, atol=0)


def test_score_norm_kernel_equals_the_host_look_up(tables):
    rng = np.random.RandomState(7)
    eps = np.concatenate([10 ** rng.uniform(np.log10(0.01), np.log10(1.55), size=61), [0.01, 1.55, 1e-3, 3.0]])
    sig = torch.from_numpy(eps.astype(np.float32))
    want = tables.score_norm(sig)
    got = noising.device_score_norm(sig.to(DEV), tables, DEV).cpu()
    assert got.shape == (65,) and torch.equal(got, want)
