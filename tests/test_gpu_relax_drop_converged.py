"""GPU tests of ``drop_converged``: the active-set kernels (adf_lbfgs_active_build in csrc/lbfgs.hip, adf_active_gather /
adf_active_scatter in csrc/active.hip) against torch indexing on the host, and relaxations with the option on against the
same relaxation with it off.  Every comparison is bit equality: a system that is not moved gets the bits of its last
forward, so there is no tolerance to measure."""
import ctypes as C

import numpy as np
import pytest
import torch

from adsorbdiff_amd import lib as L
from adsorbdiff_amd import ml_relaxation as MR
from adsorbdiff_amd import sampler as S
from adsorbdiff_amd.data import Batch
from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.synthetic import make_system
from adsorbdiff_amd.trainer import ForcesTrainer
from tests.helpers import batch_from_fixture, load_npz
from tests.helpers_lbfgs_per_system import split_systems

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE_ATOMS = (1, 2, 85, 7, 86, 171, 300)     # 3 n either side of 256 and of 512; system 3 has every atom fixed
FIXED_SYS = 3
SENTINEL = -777.0


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offsets(natoms):
    off = torch.zeros(len(natoms) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.as_tensor(natoms), 0).to(torch.int32)
    return off


class _Handle:
    """An L-BFGS handle whose update mask the test sets through adf_lbfgs_converge: zero forces clear a system's mask,
    forces of 10 eV/A set it (fmax 1)."""

    def __init__(self, natoms):
        self.lib = L.load()
        self.natoms = torch.as_tensor(natoms, dtype=torch.int64)
        self.B, self.N = len(natoms), int(self.natoms.sum())
        self.off = _offsets(natoms).to(DEV)
        self.h = C.c_void_p()
        L.check(self.lib.adf_lbfgs_create(self.N, self.B, 3, 0.04, 1.0, 70.0, 0, C.byref(self.h)))
        self.act_sys = torch.full((self.B,), -5, dtype=torch.int32, device=DEV)
        self.act_off = torch.full((self.B + 1,), -5, dtype=torch.int32, device=DEV)
        self.info = torch.full((4,), -5, dtype=torch.int32, device=DEV)

    def converge(self, flags):
        flags = torch.as_tensor(flags, dtype=torch.bool)
        f = torch.repeat_interleave(flags.float() * 10.0, self.natoms).reshape(-1, 1).repeat(1, 3).contiguous().to(DEV)
        L.check(self.lib.adf_lbfgs_converge(self.h, self.off.data_ptr(), f.data_ptr(), 1.0, None, None, _stream()))

    def build(self):
        L.check(self.lib.adf_lbfgs_active_build(self.h, self.off.data_ptr(), self.act_sys.data_ptr(),
                                                self.act_off.data_ptr(), self.info.data_ptr(), _stream()))
        return self.act_sys.cpu(), self.act_off.cpu(), self.info.cpu().tolist()

    def lists(self):
        return self.off.data_ptr(), self.act_sys.data_ptr(), self.act_off.data_ptr(), self.info.data_ptr(), self.B, self.N

    def close(self):
        torch.cuda.synchronize()
        self.lib.adf_lbfgs_destroy(self.h)


def _expected_lists(natoms, flags):
    natoms, flags = torch.as_tensor(natoms, dtype=torch.int64), torch.as_tensor(flags, dtype=torch.bool)
    B = len(natoms)
    ids = flags.nonzero().reshape(-1)
    counts = natoms[ids]
    n_act = int(counts.sum())
    sys_ = torch.cat([ids, torch.full((B - len(ids),), -1)]).to(torch.int32)
    off = torch.cat([torch.cumsum(counts, 0) - counts, torch.full((B + 1 - len(ids),), n_act)]).to(torch.int32)
    return sys_, off, len(ids), n_act


def _build_cases():
    g = torch.Generator().manual_seed(17)
    many = torch.randint(1, 4, (1500,), generator=g).tolist()
    seven = [3, 1, 4, 1, 5, 9, 2]
    return [
        ("b1_on", [5], [1]), ("b1_off", [5], [0]),
        ("b7_all", seven, [1] * 7), ("b7_none", seven, [0] * 7), ("b7_alternating", seven, [1, 0, 1, 0, 1, 0, 1]),
        ("b7_first", seven, [1] + [0] * 6), ("b7_last", seven, [0] * 6 + [1]),
        ("b1500_seam", many, (torch.rand(1500, generator=g) < 0.6).tolist()),
        ("b1500_all", many, [1] * 1500),
    ]


@pytest.mark.parametrize("name,natoms,flags", _build_cases(), ids=[c[0] for c in _build_cases()])
def test_active_build_vs_nonzero_and_cumsum(name, natoms, flags):
    h = _Handle(natoms)
    h.converge(flags)
    sys_, off, info = h.build()
    want_sys, want_off, b_act, n_act = _expected_lists(natoms, flags)
    assert torch.equal(sys_, want_sys) and torch.equal(off, want_off)
    assert info == [b_act, n_act, 1, 0]          # the first build always reports a change
    h.close()


@pytest.mark.parametrize("natoms", [[3, 1, 4, 1, 5, 9, 2], None], ids=["b7", "b1500"])
def test_active_build_changed_flag(natoms):
    g = torch.Generator().manual_seed(23)
    if natoms is None:
        natoms = torch.randint(1, 4, (1500,), generator=g).tolist()
    B = len(natoms)
    first = torch.rand(B, generator=g) < 0.7
    first[-1] = True
    smaller = first.clone()
    smaller[-1] = False                          # the list loses its last system, past the chunk seam at B = 1500
    h = _Handle(natoms)
    seen = []
    for flags in (first, first, smaller, smaller):
        h.converge(flags)
        sys_, off, info = h.build()
        want_sys, want_off, b_act, n_act = _expected_lists(natoms, flags)
        assert torch.equal(sys_, want_sys) and torch.equal(off, want_off) and info[:2] == [b_act, n_act]
        seen.append(info[2])
    assert seen == [1, 0, 1, 0]
    # reset forgets the previous list (and the mask: a build needs a converge first)
    L.check(h.lib.adf_lbfgs_reset(h.h, _stream()))
    assert h.lib.adf_lbfgs_active_build(h.h, h.off.data_ptr(), h.act_sys.data_ptr(), h.act_off.data_ptr(),
                                        h.info.data_ptr(), _stream()) == L.ADF_EINVAL
    assert b"converge" in h.lib.adf_last_error()
    h.converge(smaller)
    assert h.build()[2][2] == 1
    h.close()


def test_build_before_any_converge_is_refused():
    h = _Handle([2, 3])
    assert h.lib.adf_lbfgs_active_build(h.h, h.off.data_ptr(), h.act_sys.data_ptr(), h.act_off.data_ptr(),
                                        h.info.data_ptr(), _stream()) == L.ADF_EINVAL
    assert h.lib.adf_lbfgs_active_build(h.h, h.off.data_ptr(), None, h.act_off.data_ptr(), h.info.data_ptr(),
                                        _stream()) == L.ADF_EINVAL
    h.close()


def test_gather_and_scatter_vs_torch_indexing():
    natoms = list(SHAPE_ATOMS)
    B, N = len(natoms), sum(natoms)
    flags = [0, 1, 1, 0, 1, 0, 1]
    h = _Handle(natoms)
    h.converge(flags)
    _, _, info = h.build()
    b_act, n_act = info[:2]
    g = torch.Generator().manual_seed(5)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(natoms))
    rows = torch.as_tensor(flags, dtype=torch.bool)[batch].nonzero().reshape(-1)
    ids = torch.as_tensor(flags).nonzero().reshape(-1)
    src = {
        "w4": (torch.randint(-9, 9, (N,), generator=g, dtype=torch.int32), False),
        "w8": (torch.randint(-2 ** 40, 2 ** 40, (N,), generator=g, dtype=torch.int64), False),
        "w12": (torch.randn(N, 3, generator=g), False),
        "w36": (torch.randn(B, 3, 3, generator=g), True),
        "s8": (torch.randint(0, 2 ** 40, (B,), generator=g, dtype=torch.int64), True),
    }
    dev_src = {k: v.to(DEV) for k, (v, _) in src.items()}
    dst = {k: torch.full_like(v, 77) for k, v in dev_src.items()}
    table = (L.ActiveField * len(src))()
    for j, (k, (v, per_system)) in enumerate(src.items()):
        table[j].src, table[j].dst = dev_src[k].data_ptr(), dst[k].data_ptr()
        table[j].row_bytes, table[j].per_system = v.element_size() * v[0].numel(), int(per_system)
    assert sorted(t.row_bytes for t in table) == [4, 8, 8, 12, 36]
    c_batch = torch.full((N,), 77, dtype=torch.int64, device=DEV)
    c_natoms = torch.full((B,), 77, dtype=torch.int64, device=DEV)
    L.check(h.lib.adf_active_gather(*h.lists(), table, len(src), c_batch.data_ptr(), c_natoms.data_ptr(), _stream()))   # ONE call
    for k, (v, per_system) in src.items():
        sel, cnt = (ids, b_act) if per_system else (rows, n_act)
        got = dst[k].cpu()
        assert torch.equal(got[:cnt], v[sel]), k
        assert bool((got[cnt:] == 77).all()), k              # nothing past the compact rows
    assert torch.equal(c_natoms.cpu()[:b_act], torch.tensor(natoms)[ids]) and bool((c_natoms.cpu()[b_act:] == 77).all())
    assert torch.equal(c_batch.cpu()[:n_act], torch.repeat_interleave(torch.arange(b_act), torch.tensor(natoms)[ids]))
    assert bool((c_batch.cpu()[n_act:] == 77).all())
    # a row width that is no multiple of 4 is refused
    table[0].row_bytes = 6
    assert h.lib.adf_active_gather(*h.lists(), table, 1, None, None, _stream()) == L.ADF_EINVAL

    # scatter
    fixed = (torch.rand(N, generator=g) < 0.4).to(torch.int32)
    f_c = torch.randn(n_act, 3, generator=g) + 3.0           # no zero in it: a zero in the output is the constraint's
    e_c = torch.randn(b_act, generator=g)
    raw = torch.full((N, 3), SENTINEL, device=DEV)
    con = torch.full((N, 3), SENTINEL, device=DEV)
    energy = torch.full((B,), SENTINEL, device=DEV)
    fc_d, ec_d, fx_d = f_c.to(DEV), e_c.to(DEV), fixed.to(DEV)
    L.check(h.lib.adf_active_scatter(*h.lists(), fc_d.data_ptr(), ec_d.data_ptr(), 4, fx_d.data_ptr(), raw.data_ptr(),
                                     con.data_ptr(), energy.data_ptr(), _stream()))
    want_raw = torch.full((N, 3), SENTINEL)
    want_raw[rows] = f_c
    want_con = want_raw.clone()
    want_con[rows] = f_c.masked_fill((fixed[rows] != 0).reshape(-1, 1), 0.0)
    want_e = torch.full((B,), SENTINEL)
    want_e[ids] = e_c
    assert torch.equal(raw.cpu(), want_raw) and torch.equal(energy.cpu(), want_e)
    assert torch.equal(con.cpu().view(torch.int32), want_con.view(torch.int32))      # exact +0 on the fixed rows
    inactive = ~torch.as_tensor(flags, dtype=torch.bool)[batch]
    assert bool((raw.cpu()[inactive] == SENTINEL).all()) and bool((con.cpu()[inactive] == SENTINEL).all())
    assert bool((con.cpu()[rows][fixed[rows] != 0] == 0).all()) and not bool((raw.cpu()[rows] == 0).any())
    h.close()


# ------------------------------------------------------------------------------------------------- harmonic relaxation
STIFFNESS = [2.0, 5.0, 9.0, 4.0, 3.0, 7.0, 6.0]
AMPLITUDE = [0.01, 0.03, 0.06, 0.1, 0.1, 0.15, 0.2]
HARMONIC_SEED = 91
# Optimizer settings of the harmonic runs.  alpha is the guess of the curvature (H0 = 1 / alpha): the largest stiffness of
# the batch.  With the relaxation default of 70 the coupled recursion, whose three history pairs correct H0 along three
# directions of the whole batch only, contracts a system of stiffness k by about 1 - k / 70 per iteration everywhere else
# (0.97 for k = 2) and clears no mask but the all-fixed system's in 30 steps.  maxstep: the largest displacement is about
# 0.2 x 3.5 = 0.7 A, which alone takes 18 of the 30 steps at 0.04 A per step; 0.08 leaves the coupled mode a margin.
HARMONIC_ALPHA = 9.0
HARMONIC_MAXSTEP = 0.08


def harmonic_setup():
    """The seven systems (system 3 all fixed) on the CPU, and every system's minimum x* by sid."""
    gen = torch.Generator().manual_seed(HARMONIC_SEED)
    systems = [make_system(gen, n - 1, 1, sid=str(i)) for i, n in enumerate(SHAPE_ATOMS)]
    systems[FIXED_SYS].fixed = torch.ones_like(systems[FIXED_SYS].fixed)
    xstar = {d.sid: (d.pos + a * torch.randn(d.pos.shape, generator=gen)).float() for d, a in zip(systems, AMPLITUDE)}
    return Batch.from_data_list(systems), xstar


class _HarmonicBySid:
    """F = -k_s (x - x*_s), E = k_s / 2 |x - x*_s|^2 with k_s and x*_s looked up by ``sid`` and the rows split by the batch's
    own ``natoms``: a system's rows come from its own rows alone, whatever batch it sits in.  Records every call's sids."""

    def __init__(self, xstar):
        self._unwrapped_model = type("M", (), {"otf_graph": True})()
        self.xstar = {s: x.to(DEV) for s, x in xstar.items()}
        self.k = {str(i): k for i, k in enumerate(STIFFNESS)}
        self.calls = []

    def predict(self, batch, per_image=False, disable_tqdm=True):
        self.calls.append(list(batch.sid))
        forces, energy = [], []
        for s, p in zip(batch.sid, split_systems(batch.pos, batch.natoms.tolist())):
            d = p - self.xstar[s]
            forces.append(-(self.k[s] * d))
            energy.append((0.5 * self.k[s] * d * d).sum().reshape(1))
        return {"energy": torch.cat(energy), "forces": torch.cat(forces)}


def _harmonic_run(per_system, drop, **kw):
    b, xstar = harmonic_setup()
    b = b.to(DEV)
    tr = _HarmonicBySid(xstar)
    opt = LBFGS(b, TorchCalc(tr), maxstep=HARMONIC_MAXSTEP, memory=3, damping=1.0, alpha=HARMONIC_ALPHA, device=DEV,
                per_system=per_system, **kw)
    if drop:
        opt.set_drop_converged(True)
    state = []
    if per_system:      # the handle is gone after run(): read the step state right before it closes
        close = opt.close

        def closing():
            if opt.handle:
                state[:] = [t.cpu() for t in opt.step_state()]
            close()
        opt.close = closing
    out = opt.run(fmax=1e-3, steps=30)
    return opt, out, tr, state


@pytest.mark.parametrize("per_system", [False, True], ids=["coupled", "per_system"])
def test_harmonic_run_with_and_without_the_option(per_system):
    """The on-run against the off-run, then the precondition on the inputs (a staggered batch that converges inside the
    step budget), which says whether the comparison above it covered a spread.

    A float64 simulation of these inputs on the CPU converges the systems at iterations 2, 2, 3, 0, 4, 7, 10 in the
    per-system mode (11 iterations) and at 15, 18, 9, 0, 15, 11, 16 in the coupled mode (19 iterations); see
    HARMONIC_ALPHA / HARMONIC_MAXSTEP for why the optimizer settings are what they are."""
    B, N = len(SHAPE_ATOMS), sum(SHAPE_ATOMS)
    off, out_off, tr_off, state_off = _harmonic_run(per_system, False)
    masks = torch.stack(off.max_force_log).cpu().ge(1e-3)                  # [iterations, B]
    converged_at = masks.sum(0).tolist()
    print("iterations", off.iterations, "set masks per system", converged_at, "last max forces",
          off.max_force_log[-1].tolist())
    assert tr_off.calls == [[str(i) for i in range(B)]] * (off.iterations + 1)
    assert off.forward_log == [(B, N)] * (off.iterations + 1)

    on, out_on, tr_on, state_on = _harmonic_run(per_system, True)
    assert torch.equal(out_on.pos, out_off.pos) and torch.equal(out_on.y, out_off.y)
    assert torch.equal(out_on.force, out_off.force)
    assert torch.equal(torch.stack(on.max_force_log), torch.stack(off.max_force_log)) and on.iterations == off.iterations
    if per_system:
        assert torch.equal(state_on[0], state_off[0]) and torch.equal(state_on[1], state_off[1])
    # the model calls: everything once, then exactly the systems whose mask was set at the check before; nothing after
    # the last check
    want = [[str(i) for i in range(B)]] + [[str(i) for i in masks[it - 1].nonzero().reshape(-1).tolist()]
                                           for it in range(1, off.iterations)]
    assert tr_on.calls == want
    natoms = list(SHAPE_ATOMS)
    assert on.forward_log == [(len(c), sum(natoms[int(s)] for s in c)) for c in want]
    assert sum(len(c) for c in tr_on.calls) < (off.iterations + 1) * B
    # the inputs: at least four distinct convergence iterations, every system converged before `steps`
    assert len(set(converged_at)) >= 4 and off.iterations < 30 and not bool(masks[-1].any()), (off.iterations, converged_at)


@pytest.mark.parametrize("full", [True, False], ids=["full_traj", "first_and_last"])
def test_trajectory_files_are_the_same(tmp_path, full):
    names = [f"s{i}" for i in range(len(SHAPE_ATOMS))]
    for tag, drop in (("off", False), ("on", True)):
        _harmonic_run(True, drop, save_full_traj=full, traj_dir=tmp_path / tag, traj_names=names)
    for name in names:
        with np.load(tmp_path / "off" / f"{name}.npz") as a, np.load(tmp_path / "on" / f"{name}.npz") as b:
            assert sorted(a.files) == sorted(b.files)
            for k in a.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (name, k)
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} {k}")
            # the all-fixed system never has its mask set: no frame with save_full_traj, the first and the last without
            assert a["positions"].shape[0] >= (0 if name == f"s{FIXED_SYS}" else 1) if full else a["positions"].shape[0] == 2


# ------------------------------------------------------------------------------------------------------- model runs
HP_SMALL = dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20)
SCALES_SMALL = {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9}


class _Recording(LBFGS):
    made = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        _Recording.made.append(self)


def _painn(fixture, **kw):
    fx = load_npz(fixture)
    torch.manual_seed(int(fx["seed"]))
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES_SMALL), **{**HP_SMALL, **kw}).to(DEV).eval()
    return fx, m


def _model_case(name):
    if name == "painn":
        fx, m = _painn("relax_run.npz")
    elif name == "grad":
        fx = load_npz("relax_grad_run.npz")
        fx, m = _painn("relax_grad_run.npz", max_neighbors=int(fx["max_neighbors"]))
        m.force_mode = "energy_gradient"
    else:
        from tests.helpers_s2ef import RELAX_KW, small_model

        fx, m = load_npz("relax_eqv2_run.npz"), small_model(RELAX_KW)
    return fx, ForcesTrainer(m, device=DEV)


def _ml_relax(monkeypatch, fx, tr, per_system, drop, batch=None, **opt):
    """ml_relax on the fixture's batch -> (the returned Batch, the optimizers it made)."""
    monkeypatch.setattr(MR, "LBFGS", _Recording)
    _Recording.made = []
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV) if batch is None else batch
    relax_opt = {"memory": int(fx["memory"]), "per_system": per_system, "drop_converged": drop, **opt}
    out = MR.ml_relax(b, tr, steps=int(fx["steps"]), fmax=float(fx["fmax"]), relax_opt=relax_opt, save_full_traj=False,
                      device=DEV)
    return out, list(_Recording.made)


def _same(a, b):
    return torch.equal(a.pos, b.pos) and torch.equal(a.y, b.y) and torch.equal(a.force, b.force)


@pytest.mark.parametrize("name,per_system", [("painn", False), ("painn", True), ("eqv2", False), ("grad", False)],
                         ids=["painn_coupled", "painn_per_system", "eqv2", "gradient_forces"])
def test_model_runs_with_and_without_the_option(monkeypatch, name, per_system):
    fx, tr = _model_case(name)
    B, N = len(fx["natoms"]), int(fx["natoms"].sum())
    off, (o_off,) = _ml_relax(monkeypatch, fx, tr, per_system, False)
    on, (o_on,) = _ml_relax(monkeypatch, fx, tr, per_system, True)
    assert o_on.drop_converged and not o_off.drop_converged
    assert _same(on, off)
    assert torch.equal(torch.stack(o_on.max_force_log), torch.stack(o_off.max_force_log))
    assert o_on.iterations == o_off.iterations
    masks = torch.stack(o_on.max_force_log).cpu().ge(float(fx["fmax"]))
    if not per_system:      # the reference's recorded run is a coupled one: the on-run meets the existing criteria too
        assert o_on.iterations == int(fx["iterations"])
        assert torch.equal(masks, torch.from_numpy(fx["masks"]))
        assert float((on.pos.cpu() - torch.from_numpy(fx["pos_final"])).abs().max()) < 1e-4
        masks = torch.from_numpy(fx["masks"])
    assert sum(s for s, _ in o_on.forward_log) == B + int(masks[:-1].sum())
    assert o_on.forward_log[0] == (B, N) and len(o_on.forward_log) == o_on.iterations
    assert sum(s for s, _ in o_on.forward_log) < sum(s for s, _ in o_off.forward_log)
    # option off is today's path
    assert o_off.forward_log == [(B, N)] * (o_off.iterations + 1)
    again, _ = _ml_relax(monkeypatch, fx, tr, per_system, False)       # an off-run after an on-run in this process
    assert _same(again, off)


class _TwoAtMost:
    """A trainer that does not fit more than two systems (ml_relax then relaxes the halves)."""

    def __init__(self, tr):
        self.tr, self._unwrapped_model, self.refused = tr, tr._unwrapped_model, 0

    def predict(self, batch, per_image=False, disable_tqdm=True):
        if int(batch.natoms.shape[0]) > 2:
            self.refused += 1
            raise RuntimeError("HIP out of memory (stand-in)")
        return self.tr.predict(batch, per_image=per_image, disable_tqdm=disable_tqdm)


def test_split_and_shards_reproduce_the_whole_on_run(monkeypatch):
    fx, tr = _model_case("painn")
    whole, _ = _ml_relax(monkeypatch, fx, tr, True, True)
    natoms = fx["natoms"].tolist()
    small = _TwoAtMost(tr)
    split, made = _ml_relax(monkeypatch, fx, small, True, True)
    assert small.refused == 1 and split.sid == ["2", "3", "0", "1"] and all(o.drop_converged for o in made)
    back = [split.sid.index(s) for s in whole.sid]
    sp, sf = split_systems(split.pos, split.natoms.tolist()), split_systems(split.force, split.natoms.tolist())
    assert torch.equal(torch.cat([sp[i] for i in back]), whole.pos)
    assert torch.equal(split.y[back], whole.y)
    assert torch.equal(torch.cat([sf[i] for i in back]), whole.force)
    # two shards, packed and merged as the all-gather of ml_relax_sharded does
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    bounds = S.relaxed_bounds(natoms, 2)
    msgs, dealt = [], []
    for r in range(2):
        mine, ids = S.shard_batch(b, r, 2)
        out, _ = _ml_relax(monkeypatch, fx, tr, True, True, batch=mine)
        msgs.append(S.pack_relaxed(out, ids, bounds))
        dealt += ids
    assert sorted(dealt) == [0, 1, 2, 3]
    pos, y, force = S.merge_packed_relaxed(torch.stack(msgs), natoms)
    assert torch.equal(pos, whole.pos) and torch.equal(y, whole.y) and torch.equal(force, whole.force)
