"""GPU tests of the default (coupled) L-BFGS mode beyond one workgroup (csrc/lbfgs.hip: lb_prep / lb_loop1 / lb_loop2 with
their G partials, lb_finish, lb_step, lb_apply): the device's own trajectory followed step by step by the float64
statement of the reference's step (tests/helpers_lbfgs_coupled.py) at the sizes where the reductions change shape.  The
search direction z is compared in fp64 (``LBFGS.direction()``): f32 positions cannot see a dot product that is off by
1 / n of its value.  The tolerance on z is 16 x the spread between two summation orders of the statement itself, measured on
the CPU by tests/test_relax_coupled_host.py (H.Z_SPREAD); the device's order is a third one.  On top of that a statement
that sums in the device's restated order has to give the device's z bit for bit (lbfgs.hip is built without FMA
contraction, so every operation of the recursion is the correctly rounded one the statement performs).

Measured on one MI355X (profiles/relax_coupled_pytest_gpu.txt): z within 5.0e-16 of the statement's in every trajectory
case (tolerances 6.4e-15 to 8e-13), 7.6e-15 on the skipped iteration of two_wg (3.6e-13), max |dr| within 6.6e-16,
positions 0 ulp, and the same bits as the restated order at every iteration.  With lb_finish reading only
part[threadIdx.x] (an experiment, not kept) finish_257 fails with a z error of 3.5e-6 and cap with 7.0e-2 while their
positions stay within 0 and 1 ulp."""
import ctypes as C
import math

import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
from tests import helpers_lbfgs_coupled as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_FORCE_TOL = 8.0 * 2.0 ** -53     # two evaluations of three squares, two adds and a square root, each correctly rounded


class _Harmonic:
    """A trainer whose forces are f = -(k_s (x - x*)) in f32 from the batch's current positions, times the gain (a number
    or one per atom) the test put there; ``nan_atom`` gets a NaN component."""

    def __init__(self, inp):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.inp, self.gain, self.nan_atom = inp, None, None

    def predict(self, batch, per_image=False, disable_tqdm=True):
        f = H.harmonic_forces(batch.pos, self.inp, self.gain)
        if self.nan_atom is not None:
            f[self.nan_atom, 1] = float("nan")
        return {"energy": torch.zeros(len(self.inp.natoms), device=DEV), "forces": f}


def _on_device(inp):
    return inp._replace(xstar=inp.xstar.to(DEV), k_atom=inp.k_atom.to(DEV), fixed=inp.fixed.to(DEV))


def _batch(inp):
    b = Batch()
    b.pos = inp.pos.clone().to(DEV)
    b.natoms = torch.tensor(inp.natoms, dtype=torch.long, device=DEV)
    b.batch = inp.batch.to(DEV)
    b.fixed = inp.fixed.long().to(DEV)
    b.sid = [str(i) for i in range(len(inp.natoms))]
    return b


def _optimizer(b, tr, memory, early, fmax, per_system=False):
    opt = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=memory, damping=1.0, alpha=70.0, device=DEV, early_stop_batch=early,
                per_system=per_system)
    opt.fmax = fmax
    opt._setup()
    return opt


def _ulps(a, b):
    """Largest distance in f32 ulps between two positive finite f32 tensors (NaN rows excluded by the caller)."""
    return int((a.contiguous().view(torch.int32) - b.contiguous().view(torch.int32)).abs().max()) if a.numel() else 0


def _follow(name, memory, early, iterations, script=None, nan=None):
    """The device runs ``iterations`` steps of case ``name`` on its own trajectory; at every iteration the statement takes
    the same step from the device's positions and forces and every observable is compared.  script: H.script_gains; nan:
    (iteration, atom).  A second statement sums its dot products in the device's restated order (H.DeviceOrderDot): every
    other operation of the recursion is a correctly rounded one on both sides, so its z has to equal the device's bit for
    bit.  Returns one record per iteration."""
    inp = H.make_inputs(name)
    gains = H.script_gains(inp, script)
    tol = H.z_tol(name if script is None else f"{name}:{script}")
    b = _batch(inp)
    tr = _Harmonic(_on_device(inp))
    opt = _optimizer(b, tr, memory, early, inp.fmax)
    st = H.CoupledLBFGS(memory, early_stop_batch=early)
    st_bits = H.CoupledLBFGS(memory, early_stop_batch=early, dot=H.DeviceOrderDot(3 * sum(inp.natoms)))
    fixed_rows = inp.fixed
    rec = []
    for it in range(iterations):
        tr.gain = None if gains is None else gains[it]
        tr.nan_atom = nan[1] if nan is not None and nan[0] == it else None
        before = b.pos.cpu()
        _, _, forces = opt.check_convergence(it)
        opt.step(it, forces)
        mask_dev, mf_dev = opt.update_mask().cpu().bool(), opt.max_force_log[-1].cpu()
        z_dev, am_dev, after = opt.direction().cpu(), float(opt.last_step_max()), b.pos.cpu()
        f_cpu, pos_st = forces.cpu(), before.clone()
        mf, mask = H.system_masks(f_cpu, inp)
        z, absmax, skipped = st.step(it, pos_st, f_cpu, inp.batch, mask)
        absmax = float(absmax)
        finite = bool(torch.isfinite(z).all())
        z_bits, _, _ = st_bits.step(it, before.clone(), f_cpu, inp.batch, mask)
        same_bits = torch.equal(z_bits[~torch.isnan(z_bits)], z_dev[~torch.isnan(z_dev)])
        r = dict(mask=mask, skipped=skipped, absmax=absmax, z=z_dev, pos=after, finite=finite, same_bits=same_bits,
                 z_err=H.z_err(z_dev, z) if finite else float("nan"),
                 am_err=abs(am_dev - absmax) / absmax if finite and absmax > 0 else float("nan"))
        ok = torch.isfinite(pos_st) & torch.isfinite(after)
        r["ulps"] = _ulps(after[ok], pos_st[ok])
        rec.append(r)
        print(f"{name} m{memory} early {int(early)} it {it}: masks {int(mask.sum())} |dr|max {am_dev:.3e} "
              f"z err {r['z_err']:.2e} (tol {tol:.2e}) |dr|max err {r['am_err']:.2e} positions {r['ulps']} ulp, "
              f"z bits of the restated order: {'same' if same_bits else 'DIFFERENT'}")
        assert torch.equal(mask_dev, mask), (it, mask_dev.tolist(), mask.tolist())
        assert torch.equal(torch.isnan(mf_dev), torch.isnan(mf)), it
        live = ~torch.isnan(mf)
        assert bool(((mf_dev[live] - mf[live]).abs() <= MAX_FORCE_TOL * mf[live]).all()), (it, (mf_dev - mf).abs().max())
        assert torch.equal(torch.isnan(z_dev), torch.isnan(z)), it
        assert (am_dev < 1e-7) == skipped and math.isnan(am_dev) == math.isnan(absmax), (it, am_dev, absmax)
        assert same_bits, (it, r["z_err"])
        if finite:
            assert r["z_err"] <= tol, (it, r["z_err"], tol)
            assert abs(am_dev - absmax) <= tol * absmax, (it, am_dev, absmax)
        assert torch.equal(torch.isnan(after), torch.isnan(pos_st)), it
        assert H.ulp_close(after[ok], pos_st[ok]), (it, r["ulps"])
        if skipped:
            assert torch.equal(after, before), it
        elif not early:
            still = ~mask[inp.batch]
            assert torch.equal(after[still], before[still]), it          # bit-unchanged where the mask is clear
        assert torch.equal(after[fixed_rows], inp.pos[fixed_rows]), it   # the all-fixed system never moves
    opt.close()
    return rec


def _summary(tag, rec):
    live = [r for r in rec if r["finite"]]
    print(f"{tag} SUMMARY z err {max(r['z_err'] for r in live):.2e} |dr|max err "
          f"{max([r['am_err'] for r in live if not math.isnan(r['am_err'])], default=0.0):.2e} "
          f"positions {max(r['ulps'] for r in rec)} ulp, z bits of the restated device order: "
          f"{sum(r['same_bits'] for r in rec)} of {len(rec)} iterations the same")


TRAJECTORIES = [(name, m, e, k) for name in H.CASES for m, e, k in H.runs(name)]     # three_wg also with memory 50


@pytest.mark.parametrize("name, memory, early, iterations", TRAJECTORIES,
                         ids=[f"{n}-m{m}-{'early' if e else 'masked'}" for n, m, e, _ in TRAJECTORIES])
def test_trajectory_vs_the_float64_statement(name, memory, early, iterations):
    rec = _follow(name, memory, early, iterations)
    _summary(f"{name} m{memory} early {int(early)}", rec)
    masks = torch.stack([r["mask"] for r in rec])
    # the inputs reach what the case is for (the same conditions hold on the statement's own trajectory, on the CPU)
    if memory < iterations:
        assert iterations > 2 * memory + 2                                   # the ring wraps
    assert bool((masks[:-1] & ~masks[1:]).any())                             # a mask cleared during the run
    assert bool(masks[-1].any())                                             # and one is still set at the end
    assert not any(r["skipped"] for r in rec)


@pytest.mark.parametrize("name", ["many_systems", "two_wg"])
def test_one_skip_decision_over_the_batch(name):
    """Forces scaled by 1e-9 at iteration 2 (H.SKIP_GAINS): the step is skipped on both sides (positions bit-unchanged),
    r0 / f0 are kept, which shows in iteration 3's z still matching the statement.  The tolerance on z is the one of this
    script (H.Z_SPREAD["<case>:skip"]): the skipped iteration is worse conditioned than any of the trajectory runs."""
    assert (name, "skip") in H.SKIP_RUNS
    rec = _follow(name, 3, False, 5, script="skip")
    _summary(f"{name} skip", rec)
    assert [r["skipped"] for r in rec] == [False, False, True, False, False]
    assert rec[2]["absmax"] < 1e-7 and torch.equal(rec[2]["pos"], rec[1]["pos"])
    assert rec[3]["z_err"] <= H.z_tol(name) and not torch.equal(rec[3]["pos"], rec[2]["pos"])    # the trajectory tolerance


def test_system_299_alone_keeps_the_step_from_being_skipped():
    """The same script, but system 299 keeps its forces at iteration 2: its |dr| is read by the second pass of the strided
    maxima over the 300 systems, and the step is not skipped."""
    inp = H.make_inputs("many_systems")
    rec = _follow("many_systems", 3, False, 5, script="only_299")
    _summary("many_systems only-299", rec)
    assert not any(r["skipped"] for r in rec)
    assert rec[2]["mask"].nonzero().reshape(-1).tolist() == [299] and rec[2]["absmax"] > 1e-3
    rows = inp.batch == 299
    assert not torch.equal(rec[2]["pos"][rows], rec[1]["pos"][rows]) and torch.equal(rec[2]["pos"][~rows], rec[1]["pos"][~rows])


def test_nan_force_in_the_last_chunk():
    """A NaN force on atom 250 of two_wg (system 0, entries 750 - 752: workgroup 1) at iteration 1: the system's mask is
    clear, |dr|max is NaN, the step is not skipped, and the NaN reaches exactly the positions the statement says - every
    system whose mask is set (the coupled dot products spread it), none whose mask is clear."""
    inp = H.make_inputs("two_wg")
    assert inp.batch[250] == 0 and 3 * 250 >= H.layout(3 * sum(inp.natoms))[1]
    rec = _follow("two_wg", 3, False, 2, nan=(1, 250))
    assert rec[0]["mask"][0] and not rec[1]["mask"][0] and bool(rec[1]["mask"].any())
    assert math.isnan(rec[1]["absmax"]) and not rec[1]["skipped"]
    nan_rows = torch.isnan(rec[1]["pos"]).any(1)
    assert torch.equal(nan_rows, rec[1]["mask"][inp.batch]) and bool(torch.isnan(rec[1]["z"]).all())


def test_same_bits_twice_reset_and_the_direction_guard():
    inp = H.make_inputs("three_wg")
    dinp = _on_device(inp)
    runs = []
    for _ in range(2):
        b, tr = _batch(inp), _Harmonic(dinp)
        opt = _optimizer(b, tr, 3, False, inp.fmax)
        with pytest.raises(ValueError, match="lbfgs_get_direction"):
            opt.direction()                                   # no step yet
        out = []
        for it in range(8):
            _, _, forces = opt.check_convergence(it)
            opt.step(it, forces)
            out.append((b.pos.clone(), opt.direction()))
        runs.append((opt, b, out))
    for (pa, za), (pb, zb) in zip(runs[0][2], runs[1][2]):
        assert torch.equal(pa, pb) and torch.equal(za.view(torch.int64), zb.view(torch.int64))
    runs[1][0].close()
    opt, b, out = runs[0]
    opt.reset()
    with pytest.raises(ValueError, match="lbfgs_get_direction"):
        opt.direction()                                       # forgotten with the history
    b.pos.copy_(inp.pos.to(DEV))
    for it in range(4):
        _, _, forces = opt.check_convergence(it)
        opt.step(it, forces)
        assert torch.equal(b.pos, out[it][0]) and torch.equal(opt.direction().view(torch.int64), out[it][1].view(torch.int64)), it
    # the C entry: null arguments
    lib = L.load()
    assert lib.adf_lbfgs_get_direction(opt.handle, None, None) == L.ADF_EINVAL
    assert lib.adf_lbfgs_get_direction(None, C.c_void_p(out[0][1].data_ptr()), None) == L.ADF_EINVAL
    opt.close()


def test_coupled_and_per_system_agree_on_one_system():
    """One system of 342 atoms (n = 1026, two workgroups in the coupled mode, one in the per-system mode) stepped in both
    modes from the same positions and forces: the same mathematics in two summation orders, so z agrees within the
    two_wg tolerance and the new positions within 1 ulp."""
    inp = H.make_inputs("two_wg", natoms=[342])
    dinp = _on_device(inp)
    bc, bp, tr = _batch(inp), _batch(inp), _Harmonic(dinp)
    coupled = _optimizer(bc, tr, 3, False, inp.fmax)
    alone = _optimizer(bp, tr, 3, False, inp.fmax, per_system=True)
    worst = 0.0
    for it in range(12):
        bp.pos.copy_(bc.pos)
        _, _, forces = coupled.check_convergence(it)
        alone.check_convergence(it, forces=forces, energy=torch.zeros(1, device=DEV))
        assert coupled.update_mask().tolist() == alone.update_mask().tolist() == [1]
        coupled.step(it, forces)
        alone.step(it, forces)
        e = H.z_err(alone.direction(), coupled.direction())
        worst = max(worst, e)
        assert e <= H.z_tol("two_wg"), (it, e)
        assert H.ulp_close(bp.pos, bc.pos), it
    print(f"coupled vs per-system, 342 atoms: z differs by {worst:.2e} (tol {H.z_tol('two_wg'):.2e})")
    assert int(alone.step_state()[0][0]) == 12
    coupled.close()
    alone.close()
