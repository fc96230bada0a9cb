"""ctypes binding of libadsorbdiff_hip.so (the C ABI in include/adsorbdiff_hip.h).

This is the stub a reference maintainer would add.  The header
is the one description of the ABI: ``EXPORTS`` and every function's ``argtypes`` /
``restype`` are parsed from its prototypes (``parse_header``), so a new entry point
is declared there and nowhere else; only the struct mirrors and the status codes
are repeated here, and tests/test_host_logic.py compares them with the header.  There is
no fallback: if the library is missing or a call fails, an exception is
raised — ``RuntimeError`` for out-of-memory / HIP errors (so that
``ml_diffuse``'s split-and-retry contract works, reference
relaxation/ml_relaxation.py:146-165) and ``ValueError`` for an image without
neighbours (reference painn_denoising.py:370-375) and for a structure beyond a
fixed capacity of the graph builder (``ADF_EOVERFLOW``: splitting the batch does
not help).
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

ADF_OK, ADF_EINVAL, ADF_EOOM, ADF_ENONEIGHBOR, ADF_EHIP, ADF_EOVERFLOW, ADF_ENUMERIC = 0, 1, 2, 3, 4, 5, 6


class NumericRangeError(ArithmeticError):
    """Non-finite model output (ADF_ENUMERIC).  Not a RuntimeError on purpose: ``ml_diffuse`` must not answer it by
    splitting the batch; the engine answers it by re-running in exact f32."""


class Hparams(C.Structure):
    _fields_ = [
        ("hidden_channels", C.c_int32), ("num_layers", C.c_int32), ("num_rbf", C.c_int32),
        ("num_elements", C.c_int32), ("max_neighbors", C.c_int32), ("envelope_exponent", C.c_int32),
        ("num_heads", C.c_int32), ("cutoff", C.c_float),
    ]


class EqV2Hparams(C.Structure):
    _fields_ = [
        ("lmax", C.c_int32), ("mmax", C.c_int32), ("num_layers", C.c_int32), ("sphere_channels", C.c_int32),
        ("attn_hidden_channels", C.c_int32), ("num_heads", C.c_int32), ("attn_alpha_channels", C.c_int32),
        ("attn_value_channels", C.c_int32), ("ffn_hidden_channels", C.c_int32), ("grid_resolution", C.c_int32),
        ("edge_channels", C.c_int32), ("num_distance_basis", C.c_int32), ("max_num_elements", C.c_int32),
        ("max_neighbors", C.c_int32), ("max_radius", C.c_float), ("avg_degree", C.c_float),
    ]


class EqV2Counters(C.Structure):
    _fields_ = [("num_edges", C.c_int64), ("num_atoms", C.c_int64), ("dense_flops", C.c_int64), ("conv_flops", C.c_int64),
                ("inc_rows", C.c_int64), ("inc_rows_full", C.c_int64), ("forwards_total", C.c_int64),
                ("conv_flops_total", C.c_int64)]


class Tune(C.Structure):
    """adf_tune: the kernel-selection switches a handle holds (include/adsorbdiff_hip.h)."""
    _fields_ = [(name, C.c_int32) for name in (
        "gemm_stream", "head_gate_fused", "lift_emit", "graph_sys_csr", "train_gemm16", "wgrad_f32",
        "eqv2_gemm_tile256", "eqv2_rotin_generic", "eqv2_rotout_generic", "sample_split")]


class SplitView(C.Structure):
    """adf_split_view: view B of a split sampling run (include/adsorbdiff_hip.h, "Two half-batches, two streams")."""
    _fields_ = [("cut", C.c_int32), ("atoms_a", C.c_int32), ("n_out_a", C.c_int32), ("n_out_b", C.c_int32),
                ("atom_offset", C.c_void_p), ("batch", C.c_void_p), ("out_idx", C.c_void_p), ("mov_idx", C.c_void_p),
                ("mov_off", C.c_void_p)]


class BatchDesc(C.Structure):
    _fields_ = [
        ("num_systems", C.c_int32), ("num_atoms", C.c_int32), ("pos", C.c_void_p), ("cell", C.c_void_p),
        ("atomic_numbers", C.c_void_p), ("batch", C.c_void_p), ("atom_offset", C.c_void_p), ("reps", C.c_int32 * 3),
    ]


class ActiveField(C.Structure):
    """adf_active_field: one array of adf_active_gather (rows per atom, or per system)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int32), ("per_system", C.c_int32)]


class StepCoef(C.Structure):
    _fields_ = [
        ("coef_tr", C.c_float), ("rot_pre", C.c_float), ("rot_dt", C.c_float), ("rot_g2", C.c_float),
        ("noise_tr", C.c_float), ("noise_rot", C.c_float),
    ]


class TrCoef(C.Structure):
    """adf_tr_coef: per-step scalars of the translation-only samplers (dcom = coef * score + noise * z)."""
    _fields_ = [("coef", C.c_float), ("noise", C.c_float)]


class Counters(C.Structure):
    _fields_ = [
        ("num_edges", C.c_int64), ("num_atoms", C.c_int64), ("message_bytes_per_layer", C.c_int64),
        ("dense_flops", C.c_int64),
        ("inc_rows", C.c_int64), ("inc_rows_full", C.c_int64), ("inc_msg_launches", C.c_int64),
        ("inc_msg_edges", C.c_int64),
    ]


# ---- the header is the one description of the ABI: every prototype in it is bound from its own text
HEADER = Path(__file__).resolve().parent.parent / "include" / "adsorbdiff_hip.h"

_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RETURNS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p}
# the structs that are always host structs handed over with byref(); adf_step_coef / adf_tr_coef are also device tables
# passed as data_ptr(), so a pointer to one is a plain address, and so is one to adf_split_view
_BYREF = {"adf_batch": BatchDesc, "adf_painn_hparams": Hparams, "adf_eqv2_hparams": EqV2Hparams, "adf_tune": Tune,
          "adf_counters": Counters, "adf_eqv2_counters": EqV2Counters, "adf_active_field": ActiveField}


def parse_header(text: str) -> dict:
    """``{name: (restype, argtypes)}`` for every function the header text declares, in its order.  Whatever is no
    comment, preprocessor line, enum, struct or handle typedef has to be a prototype in the vocabulary above: anything else
    raises ``ValueError`` naming the function and the type, so that an entry is bound correctly or not at all."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs = set(re.findall(r"typedef\s+struct\s*\w*\s*\{[^}]*\}\s*(\w+)\s*;", text))
    text = re.sub(r"(typedef\s+struct|enum)\s*\w*\s*\{[^}]*\}\s*\w*\s*;", " ", text)
    handles = set(re.findall(r"typedef\s+struct\s+\w+\s*\*\s*(adf_\w+_t)\s*;", text))
    text = re.sub(r"typedef\s+struct\s+\w+\s*\*\s*adf_\w+_t\s*;|extern\s+\"C\"\s*\{|\}", " ", text)
    pointees = set(_SCALARS) | structs | handles | {"void", "char", "uint8_t"}

    def argtype(fn: str, param: str):
        tokens = [t for t in re.findall(r"\w+|\*|\S", param) if t != "const"]
        base, stars, name = tokens[:1], tokens[1:-1], tokens[-1:]
        if len(tokens) < 2 or any(t != "*" for t in stars) or not re.fullmatch(r"[A-Za-z_]\w*", name[0]) or name[0] in pointees:
            raise ValueError(f"{fn}: parameter {param.strip()!r} is not `type name`")
        base = base[0]
        if stars:
            if base not in pointees:
                raise ValueError(f"{fn}: parameter {param.strip()!r} points to the unknown type {base!r}")
            return C.POINTER(_BYREF[base]) if base in _BYREF and len(stars) == 1 else C.c_void_p
        if base in handles:
            return C.c_void_p
        if base not in _SCALARS:
            raise ValueError(f"{fn}: parameter {param.strip()!r} has the unknown type {base!r}")
        return _SCALARS[base]

    out = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(adf_[a-z_0-9]+)\s*\((.*)\)", stmt, flags=re.S)
        if m is None:
            raise ValueError(f"not a prototype, an enum, a struct or a handle typedef: {' '.join(stmt.split())!r}")
        ret, fn, params = re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise ValueError(f"{fn}: unknown return type {ret!r}")
        if fn in out:
            raise ValueError(f"{fn}: declared twice")
        out[fn] = (_RETURNS[ret], [] if params == "void" else [argtype(fn, p) for p in params.split(",")])
    return out


SIGNATURES = parse_header(HEADER.read_text())
EXPORTS = tuple(SIGNATURES)

# the EquiformerV2 training operators are declared beside their translation unit (csrc/eqv2_train.h, which builds on the
# header's types); they are bound from that text by the same parser, so they too are bound correctly or not at all
TRAIN_HEADER = Path(__file__).resolve().parent / "csrc" / "eqv2_train.h"
TRAIN_SIGNATURES = {name: sig for name, sig in parse_header(HEADER.read_text() + "\n" + TRAIN_HEADER.read_text()).items()
                    if name not in SIGNATURES}

# the S2EF training operators of EquiformerV2 (csrc/eqv2_s2ef_train.h): the same parser, a table of their own
S2EF_TRAIN_HEADER = Path(__file__).resolve().parent / "csrc" / "eqv2_s2ef_train.h"
S2EF_TRAIN_SIGNATURES = {name: sig
                         for name, sig in parse_header(HEADER.read_text() + "\n" + S2EF_TRAIN_HEADER.read_text()).items()
                         if name not in SIGNATURES}

# the geometric gradient of the EquiformerV2 training graph (csrc/eqv2_geo.h): the same parser, a table of their own
GEO_HEADER = Path(__file__).resolve().parent / "csrc" / "eqv2_geo.h"
GEO_SIGNATURES = {name: sig for name, sig in parse_header(HEADER.read_text() + "\n" + GEO_HEADER.read_text()).items()
                  if name not in SIGNATURES}

# the dual operators of the PaiNN step that trains on energy-gradient forces (csrc/dual_ops.h): the same
# parser, a table of their own
DUAL_HEADER = Path(__file__).resolve().parent / "csrc" / "dual_ops.h"
DUAL_SIGNATURES = {name: sig for name, sig in parse_header(HEADER.read_text() + "\n" + DUAL_HEADER.read_text()).items()
                   if name not in SIGNATURES}

_LIB = None


def lib_path() -> Path:
    import os

    override = os.environ.get("ADF_LIB_PATH")  # development only: A/B a differently built library
    if override:
        return Path(override)
    return Path(__file__).resolve().parent / "libadsorbdiff_hip.so"


def load():
    """Load the shared library (once) and bind every function of the header.  Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not path.exists():
        raise RuntimeError(
            f"{path} not found: build it with `python -m adsorbdiff_amd.build` "
            "(the HIP path has no CPU fallback)"
        )
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in {**SIGNATURES, **TRAIN_SIGNATURES, **S2EF_TRAIN_SIGNATURES, **GEO_SIGNATURES,
                                      **DUAL_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = lib
    return lib


def check(status: int) -> None:
    """Translate a status code into the exception the reference's callers expect."""
    if status == ADF_OK:
        return
    msg = load().adf_last_error().decode("utf-8", "replace")
    if status == ADF_ENONEIGHBOR:
        raise ValueError(msg)
    if status == ADF_EOVERFLOW:
        # a property of one structure (candidates around a centre, incoming edges of an atom): halving the batch, which is
        # what ``ml_diffuse`` / ``ml_relax`` answer a RuntimeError with, cannot cure it
        raise ValueError(f"adsorbdiff_hip: capacity exceeded: {msg}")
    if status == ADF_EOOM:
        raise RuntimeError(f"HIP out of memory: {msg}")
    if status == ADF_ENUMERIC:
        raise NumericRangeError(msg)
    if status == ADF_EINVAL:
        raise ValueError(f"adsorbdiff_hip: invalid argument: {msg}")
    raise RuntimeError(f"adsorbdiff_hip error {status}: {msg}")
