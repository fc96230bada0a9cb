"""GPU tests of forces as the gradient of the energy for the S2EF PaiNN (``PaiNN.force_mode = "energy_gradient"``,
``adf_painn_forward_energy_gradient``: csrc/energy_grad.hip, csrc/message_geo.hip) against the reference's float64 autograd
recorded by tools/make_golden_grad_forces.py, and against the float64 oracle of tests/helpers_grad_forces.py at ragged
shapes.  Every bound is relative to the case's max|F| (REL_TOL: the project's parity budget) or a multiple of what the
reference's own float32 autograd leaves, as stored in the fixture."""
import os
import subprocess
import sys

import pytest
import torch

from adsorbdiff_amd.lbfgs_torch import LBFGS, TorchCalc
from adsorbdiff_amd.ml_relaxation import ml_relax
from adsorbdiff_amd.painn import PaiNN
from adsorbdiff_amd.trainer import ForcesTrainer
from tests import helpers_grad_forces as HG
from tests.helpers import batch_from_fixture, load_npz, rel_err, row_rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 1e-4
HP = {"small": dict(hidden_channels=128, num_layers=2, num_rbf=128, cutoff=6.0, max_neighbors=20),
      "full": dict(hidden_channels=512, num_layers=6, num_rbf=128, cutoff=12.0, max_neighbors=50)}
SCALES = {"small": {"upd_out_scalar_scale_0": 1.05, "upd_out_scalar_scale_1": 0.9},
          "full": {f"upd_out_scalar_scale_{i}": 1.0 - 0.04 * i for i in range(6)}}
CASES = {"small": ("small", {}), "full": ("full", {}), "nohead": ("small", dict(regress_forces=False)), "ragged": ("small", {})}


def _sub(fx, prefix):
    return {k[len(prefix):]: v for k, v in fx.items() if k.startswith(prefix)}


def _model(size, seed, mode="energy_gradient", **kw):
    torch.manual_seed(seed)
    m = PaiNN(None, 50, 1, scale_file=dict(SCALES[size]), **{**HP[size], **kw}).to(DEV).eval()
    m.force_mode = mode
    return m


def _max_rel(a, ref):
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / ref.abs().max())


def _net(forces, batch, B):
    f = forces.double().cpu()
    return float(torch.zeros(B, 3, dtype=torch.float64).index_add_(0, batch.cpu().long(), f).abs().max() / f.abs().max())


def _check_case(case):
    """Parity (1) and zero net force (3) of one fixture case in the arithmetic the process runs in."""
    size, kw = CASES[case]
    fx = _sub(load_npz("grad_forces.npz"), case + "_")
    m = _model(size, int(fx["seed"]), **kw)
    b = batch_from_fixture(fx, device=DEV)
    out = m(b)
    assert set(out) == {"energy", "forces"} and out["forces"].shape == b.pos.shape
    e_err = row_rel_err(out["energy"].cpu().reshape(-1, 1), torch.from_numpy(fx["energy"]).reshape(-1, 1))
    f_err = _max_rel(out["forces"], fx["forces"])
    net = _net(out["forces"], b.batch, len(fx["natoms"]))
    print(f"grad_forces[{case}] exact_f32={m.engine(DEV).exact_f32}: energy row-rel {e_err:.3e}, forces max-rel {f_err:.3e} "
          f"(float32 reference {float(fx['err32']):.3e}), net force {net:.3e} (float32 reference {float(fx['net32']):.3e})")
    assert e_err < REL_TOL
    assert f_err < REL_TOL
    assert net < 4 * float(fx["net32"])


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_forces_vs_reference_float64_autograd(case):
    """Default arithmetic (f16x3 split products, the fused message kernels)."""
    _check_case(case)


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_forces_vs_reference_in_exact_f32(case):
    """ADF_GEMM=f32 is read when a handle is created: a fresh process per case (it opens the GPU itself)."""
    env = dict(os.environ, ADF_GEMM="f32", ADF_GRAD_CASE=case)
    code = "import os; from tests import test_gpu_grad_forces as T; T._check_case(os.environ['ADF_GRAD_CASE'])"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stderr[-4000:]
    assert "exact_f32=True" in res.stdout


def test_exact_f32_switch_on_the_same_engine_meets_the_budget():
    """The retry path of the error protocol: the handle switched to exact f32 after construction (use_exact_f32)."""
    fx = _sub(load_npz("grad_forces.npz"), "small_")
    m = _model("small", int(fx["seed"]))
    b = batch_from_fixture(fx, device=DEV)
    first = m(b)["forces"].clone()
    assert m.engine(DEV).use_exact_f32()
    out = m(b)
    assert _max_rel(out["forces"], fx["forces"]) < REL_TOL and _max_rel(first, fx["forces"]) < REL_TOL
    assert row_rel_err(out["energy"].cpu().reshape(-1, 1), torch.from_numpy(fx["energy"]).reshape(-1, 1)) < REL_TOL


def test_direct_mode_untouched_by_gradient_evaluations():
    """force_mode="direct" returns what it returned before (tests/test_gpu_relax.py's check against relax_painn.npz), and
    the same bits before and after a gradient evaluation on the same engine."""
    fx = _sub(load_npz("relax_painn.npz"), "small_")
    m = _model("small", int(fx["seed"]), mode="direct")
    b = batch_from_fixture(fx, device=DEV)
    before = m(b)
    assert row_rel_err(before["energy"].cpu().reshape(-1, 1), torch.from_numpy(fx["energy"]).reshape(-1, 1)) < REL_TOL
    assert rel_err(before["forces"].cpu(), fx["forces"]) < REL_TOL
    before = {k: v.clone() for k, v in before.items()}
    m.force_mode = "energy_gradient"
    grad = m(b)
    assert not torch.equal(grad["forces"], before["forces"])
    m.force_mode = "direct"
    after = m(b)
    assert torch.equal(after["energy"].view(torch.int32), before["energy"].view(torch.int32))
    assert torch.equal(after["forces"].view(torch.int32), before["forces"].view(torch.int32))
    # the gradient call's energy is the direct call's up to the unfused activation of its head
    assert row_rel_err(grad["energy"].cpu().reshape(-1, 1), before["energy"].cpu().reshape(-1, 1)) < 1e-5


def test_directional_derivative_on_the_device():
    """(E(pos + h v) - E(pos - h v)) / 2h from two forward_energy calls against -F . v from one gradient call, both
    compared with the fixture's float64 central difference at the same h (the truncation cancels in the first; the second
    differs from it by the recorded truncation).  Bound: 4 x the float32 reference's deviation recorded in the fixture."""
    fx = _sub(load_npz("grad_forces.npz"), "dir_")
    m = _model("small", int(fx["seed"]), max_neighbors=int(fx["max_neighbors"]))
    b = batch_from_fixture(fx, device=DEV)
    eng = m.engine(DEV)
    v = torch.from_numpy(fx["v"])
    h = float(fx["h"])
    p0 = b.pos.double().cpu()
    es = []
    for sgn in (1.0, -1.0):
        bb = b.clone()
        bb.pos = (p0 + sgn * h * v).float().to(DEV)
        es.append(float(eng.forward_energy(bb)[0].double().sum()))
    fd = (es[0] - es[1]) / (2 * h)
    _, forces = eng.forward_energy_gradient(b)
    ana = float(-(forces.double().cpu() * v).sum())
    fd64, ana64, bound = float(fx["fd64"]), float(fx["ana64"]), 4 * float(fx["dev32"])
    print(f"directional: device difference {fd:.8e} (fixture {fd64:.8e}, dev {abs(fd - fd64) / abs(fd64):.3e}); "
          f"-F.v {ana:.8e} (fixture's float64 {ana64:.8e}, dev {abs(ana - ana64) / abs(ana64):.3e}); bound {bound:.3e}")
    assert abs(fd - fd64) / abs(fd64) < bound
    assert abs(ana - ana64) / abs(ana64) < bound


def test_reproducible_and_bit_identical_alone_and_in_batch():
    fx = _sub(load_npz("grad_forces.npz"), "ragged_")
    m = _model("small", int(fx["seed"]))
    b = batch_from_fixture(fx, device=DEV)
    full = {k: v.clone() for k, v in m(b).items()}
    again = m(b)
    assert torch.equal(again["forces"].view(torch.int32), full["forces"].view(torch.int32))
    assert torch.equal(again["energy"].view(torch.int32), full["energy"].view(torch.int32))
    off = 0
    for s, d in enumerate(b.to_data_list()):
        n = d.pos.shape[0]
        d.batch = torch.zeros(n, dtype=torch.long, device=DEV)
        one = m(d)
        assert torch.equal(one["energy"].view(torch.int32), full["energy"][s:s + 1].view(torch.int32)), s
        assert torch.equal(one["forces"].view(torch.int32), full["forces"][off:off + n].view(torch.int32)), s
        off += n


def test_relaxation_with_gradient_forces_vs_reference():
    """Same criteria as test_gpu_relax.py::test_painn_relaxation_vs_reference_and_reproducible, the reference run driven by
    its own autograd forces (relax_grad_run.npz)."""
    fx = load_npz("relax_grad_run.npz")
    m = _model("small", int(fx["seed"]), max_neighbors=int(fx["max_neighbors"]))
    tr = ForcesTrainer(m, device=DEV)
    b = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    opt = LBFGS(b, TorchCalc(tr), maxstep=0.04, memory=int(fx["memory"]), damping=1.0, alpha=70.0, device=DEV)
    out = opt.run(fmax=float(fx["fmax"]), steps=int(fx["steps"]))
    assert opt.iterations == int(fx["iterations"])
    assert torch.equal(torch.stack(opt.max_force_log).cpu().ge(float(fx["fmax"])), torch.from_numpy(fx["masks"]))
    assert float((out.pos.cpu() - torch.from_numpy(fx["pos_final"])).abs().max()) < 1e-4
    assert row_rel_err(out.y.cpu().reshape(-1, 1), torch.from_numpy(fx["y"]).reshape(-1, 1)) < REL_TOL
    assert _max_rel(out.force, fx["force"]) < REL_TOL
    b2 = batch_from_fixture(fx, pos_key="pos_in", device=DEV)
    out2 = ml_relax(b2, tr, steps=int(fx["steps"]), fmax=float(fx["fmax"]), relax_opt={"memory": int(fx["memory"])},
                    save_full_traj=False, device=DEV)
    assert torch.equal(out2.pos, out.pos) and torch.equal(out2.y, out.y) and torch.equal(out2.force, out.force)


def _check_config(name):
    """One ragged configuration against float64 autograd on the engine's own edge list, in the arithmetic the process
    runs in."""
    cfg = HG.CONFIGS[name]
    m = HG.make_config_model(name).to(DEV)
    m.force_mode = "energy_gradient"
    b = HG.make_config_batch(name).to(DEV)
    out = m(b)
    es, ed, vec = HG.engine_graph(m, b)
    rows = torch.bincount(ed, minlength=b.pos.shape[0])
    if name == "ragged":
        assert int(rows[rows > 0].min()) < 32
    if name == "many_rows":
        assert int(rows.max()) > 64
    bc = b.to("cpu")
    off = HG.edge_offsets(bc.pos, bc.cell, bc.batch, es, ed, vec)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    e, f = HG.energy_forces(sd, bc.pos, bc.atomic_numbers, bc.batch, len(bc.natoms), es, ed, off, hidden_channels=cfg["H"],
                            num_layers=cfg["L"], num_rbf=cfg["R"], cutoff=cfg["cutoff"], scale_factors=m.scale_factors())
    e_err = row_rel_err(out["energy"].cpu().reshape(-1, 1), e.reshape(-1, 1))
    f_err = _max_rel(out["forces"], f)
    print(f"grad_forces[{name}] exact_f32={m.engine(DEV).exact_f32}: energy row-rel {e_err:.3e}, forces max-rel {f_err:.3e}, "
          f"max|F| {float(f.abs().max()):.3f}, edge rows per atom {int(rows.min())}..{int(rows.max())}")
    assert e_err < REL_TOL
    assert f_err < REL_TOL


@pytest.mark.parametrize("name", list(HG.CONFIGS))
def test_ragged_shapes_vs_float64_oracle(name):
    """Systems of different sizes, atoms with fewer than 32 and more than 64 edge rows, 64 and 128 basis functions, one and
    six layers, three channel slices: against float64 autograd on the engine's own edge list."""
    _check_config(name)


@pytest.mark.parametrize("name", ["one_layer", "six_layers_r64", "many_rows"])
def test_ragged_shapes_in_exact_f32(name):
    """The plain kernel of the exact arithmetic on its own branches: a vec == 0 layer alone, a basis narrower than 128, a
    width that is not a multiple of its 256-channel block.  A fresh process (ADF_GEMM is read at handle creation)."""
    env = dict(os.environ, ADF_GEMM="f32", ADF_GRAD_CASE=name)
    code = "import os; from tests import test_gpu_grad_forces as T; T._check_config(os.environ['ADF_GRAD_CASE'])"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    print(res.stdout[-2000:])
    assert res.returncode == 0, res.stderr[-4000:]
    assert "exact_f32=True" in res.stdout
