"""CPU side of the EquiformerV2 training step: csrc/eqv2_train.h lists the new entries and lib.py binds them, the references the GPU tests use are sound
(the restated block loop equals the oracle's forward when nothing is masked; masks and the energy term act), and the
calibration the GPU tests print: how far float32 autograd through the oracle is from float64, per group and parameter."""
import re
from pathlib import Path

import torch

from adsorbdiff_amd import lib as L
from oracle import eqv2_oracle as Q
from tests import helpers_eqv2_train as T

ROOT = Path(__file__).resolve().parent.parent
NEW_ENTRIES = ["adf_eqv2_export_graph", "adf_op_eq_linear_fwd", "adf_op_eq_linear_bwd", "adf_op_eq_silu_fwd", "adf_op_eq_silu_bwd",
               "adf_op_eq_edge_scalars", "adf_op_eq_rotate_in_fwd", "adf_op_eq_rotate_in_bwd", "adf_op_eq_s2act_fwd",
               "adf_op_eq_s2act_bwd", "adf_op_eq_alpha_fwd", "adf_op_eq_alpha_bwd", "adf_op_eq_rotate_out_fwd",
               "adf_op_eq_rotate_out_bwd"]


def test_header_lists_every_new_export_and_the_library_has_them():
    header = L.TRAIN_HEADER.read_text()
    assert L.TRAIN_HEADER == ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_train.h"
    declared = re.findall(r"\b(adf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert declared == NEW_ENTRIES == list(L.TRAIN_SIGNATURES)
    assert not set(NEW_ENTRIES) & set(L.EXPORTS)          # include/adsorbdiff_hip.h is as it was
    lib = L.load()
    i32, i64, vp = L.C.c_int32, L.C.c_int64, L.C.c_void_p
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype is i32 and list(getattr(lib, name).argtypes) == L.TRAIN_SIGNATURES[name][1]
    # two bindings written out by hand: a host struct by reference with an int64 out-pointer, and the strided product
    assert lib.adf_eqv2_export_graph.argtypes == [vp, L.C.POINTER(L.BatchDesc), i64, vp, vp, vp, vp, vp, vp, vp]
    assert lib.adf_op_eq_linear_fwd.argtypes == [vp, i32, vp, i32, vp, vp, i32, i32, i64, i32, i32, vp]
    # what the translation unit defines and what the header declares are the same set
    src = (ROOT / "adsorbdiff_amd" / "csrc" / "eqv2_train.hip").read_text()
    defined = re.findall(r'extern "C" int32_t (adf_[a-z_0-9]+)\(', src)
    assert sorted(defined) == sorted(n for n in NEW_ENTRIES if n != "adf_eqv2_export_graph")
    assert "atomicAdd" not in src and "atomicMax" not in src      # no atomics at all in the training operators
    # null handles and null buffers are refused before anything is launched
    assert lib.adf_op_eq_rotate_in_fwd(None, None, None, None, None, None, 0, None, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_linear_fwd(None, 1, None, 1, None, None, 1, 0, 1, 1, 1, None) == L.ADF_EINVAL
    assert lib.adf_op_eq_silu_fwd(None, None, 4, None) == L.ADF_EINVAL


def test_index_helpers_match_the_oracle_layouts():
    Lm, M = 4, 2
    vec = torch.randn(7, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    D = Q.wigner_from_rotation(Lm, Q.edge_frames(vec))
    rm = Q.reduced_mask(Lm, M)
    # pack the kept rows as the device does: degree l, rows |m'| <= min(l, M), row-major [rows][2l+1]
    wig = torch.cat([D[:, l * l + l - min(l, M):l * l + l + min(l, M) + 1, l * l:(l + 1) ** 2].reshape(7, -1) for l in range(Lm + 1)], 1)
    assert torch.equal(T.wigner_rows_to_D(wig, Lm, M), D[:, rm, :])
    perm = Q.order_major_perm(Lm, M)
    red = Q.lm_list(Lm, M)
    rows = T.radial_rows(Lm, M)
    off = {0: 0, 1: Lm + 1, 2: Lm + 1 + Lm}
    for k, p in enumerate(perm.tolist()):
        l, m = red[p]
        assert int(rows[k]) == off[abs(m)] + l - abs(m)


def _case():
    m = T.train_model("small")
    b, ei, vec = T.ragged_case()
    return m, b, T.make_targets(1), (ei, vec)


def test_restated_forward_equals_the_oracle_when_nothing_is_masked():
    m, b, targets, graph = _case()
    plain = T.reference_step(m, b, targets, graph)
    again = T.reference_step(m, b, targets, graph, restated=True)
    assert T.frob(again["out1"], plain["out1"]) < 1e-12 and T.frob(again["out2"], plain["out2"]) < 1e-12
    assert abs(float(again["loss"][0] - plain["loss"][0])) < 1e-12 * abs(float(plain["loss"][0]))
    for k, g in plain["grads"].items():
        if g is None:
            assert again["grads"][k] is None and k.startswith("energy_block."), k
        elif float(g.norm()) > 0.0:
            assert T.frob(again["grads"][k], g) < 1e-9, k
    # masks with every entry kept at rate 0.1 only rescale by 1 / keep: they act
    m.alpha_drop, m.drop_path_rate = 0.1, 0.1
    E = graph[0].shape[1]
    masks = {"alpha": [torch.ones(E, m.num_heads) for _ in range(m.num_layers)], "path": torch.ones(m.num_layers, 2, 1)}
    kept = T.reference_step(m, b, targets, graph, masks=masks)
    assert T.frob(kept["out1"], plain["out1"]) > 1e-3


def test_identically_zero_gradients_and_unused_parameters():
    m, b, targets, graph = _case()
    ref = T.reference_step(m, b, targets, graph)
    for k, g in ref["grads"].items():
        if T.identically_zero(k):
            assert g is not None and float(g.abs().max()) == 0.0, k
    one = T.train_model("small", two_heads=False)
    ref1 = T.reference_step(one, b, targets, graph)
    assert all(g is None for k, g in ref1["grads"].items() if k.startswith(("force_block2.", "energy_block.")))
    assert float(ref1["loss"][2]) == 0.0 and float(ref1["loss"][0]) == float(ref1["loss"][1])


def test_float32_oracle_distance_from_float64_is_the_calibration():
    """The figures the GPU tests compare against: float32 torch autograd through the oracle on the ragged graph, per group
    and per parameter.  The groups stay inside the 1e-4 budget; single parameters (node sums with cancellation over the
    128-edge hub) may come close to it, which is why the per-parameter bound has the 10 x float32 clause."""
    m, b, targets, graph = _case()
    r64 = T.reference_step(m, b, targets, graph)
    r32 = T.reference_step(m, b, targets, graph, torch.float32)
    live = {k: g for k, g in r64["grads"].items() if g is not None}
    groups = T.grouped_ratio(r32["grads"], live)
    per = sorted((T.frob(r32["grads"][k], g), k) for k, g in live.items() if float(g.norm()) > 0.0)
    print("float32 oracle vs float64, groups:", {g: f"{e:.1e}" for g, e in groups.items()})
    print("worst parameters:", [(k, f"{e:.1e}") for e, k in per[-3:]], "median", f"{per[len(per) // 2][0]:.1e}")
    assert max(groups.values()) < T.REL_TOL
    assert per[len(per) // 2][0] < 1e-5
    assert abs(float(r32["loss"][0] - r64["loss"][0])) < 1e-5 * abs(float(r64["loss"][0]))
