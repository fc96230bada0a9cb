// The environment switches of the library (INTEGRATION.md 4 documents each): one struct, one table, one reader.  Host only,
// no HIP.  adf_switches_from_env() is the only place under csrc/ that reads the environment; a new switch is a field here,
// a row of the table below and a line of INTEGRATION.md (tests/test_host_logic.py compares the three).
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/adsorbdiff_hip.h"

struct adf_switches {
    adf_tune tune;               // the kernel-selection switches: the public struct (adf_painn_get_tune), variables named there
    // adf_painn_create
    int32_t incremental;         // ADF_INCREMENTAL: 0 = every row of every layer at every forward, else 1 (default)
    int32_t inc_sync;            // ADF_INC_SYNC: 1 = read the recompute-list lengths back at every forward, else 0 (default)
    int32_t gemm_f32;            // ADF_GEMM: "f32" = 1, every product in exact f32, else 0 (adf_eqv2_create too)
    int32_t lift;                // ADF_LIFT: 0 = no per-row lifts of the f16x3 A operands, else 1 (default)
    int32_t msg_f32;             // ADF_MSG: "f32" = 1, the message kernel in exact f32; another word = 0; unset = gemm_f32
    int32_t msg_rbf_direct;      // ADF_MSG_RBF: "direct" = 1, every Gaussian by its own exp2, else 0 (used at weight binding)
    int32_t row_maxima;          // ADF_ROW_MAXIMA: 0 = the layers' row magnitudes by measuring passes, else 1 (default)
    // adf_eqv2_create
    int32_t eqv2_s2_emit;        // ADF_EQV2_S2_EMIT: 1 = the S2 activation hands its output rows' magnitudes to the second convolution
                                 // (atomics in its epilogue) instead of a pass over them, else 0 (default: measured slower on
                                 // MI355X, +8 ms vs -3 ms per forward at 256 k edges)
    int32_t eqv2_presplit;       // ADF_EQV2_PRESPLIT: 0 = rotate-in writes fp32 rows, else 1 (default): fp16 hi / lo images
    int32_t eqv2_conv1_wr;       // ADF_EQV2_CONV1_WR: 0 = first convolution with its weights staged through LDS, else 1 (default)
    int32_t eqv2_conv2_wr;       // ADF_EQV2_CONV2_WR: 0 = second convolution on eq_gemm16_256_kernel throughout, else 1 (default)
    int32_t eqv2_alpha_generic;  // ADF_EQV2_ALPHA_GENERIC: 1 = attention logits one head at a time for every width, else 0 (default)
    int32_t eqv2_fold;           // ADF_EQV2_FOLD: 0 = the grid MLP as three products on the grid rows, else 1 (default)
    int32_t eqv2_compact;        // ADF_EQV2_COMPACT: 0 = force blocks evaluate every column of their second convolution, else 1
    int32_t eqv2_radial_edge;    // ADF_EQV2_RADIAL: "edge" = 1, radial MLPs per edge, never tabulated, else 0 (used at weight binding)
    int64_t eqv2_chunk_edges;    // ADF_EQV2_CHUNK_EDGES: edges per node chunk, a positive integer (default 2^19; used when the
                                 // workspaces grow)
};

enum adf_switch_kind {
    ADF_SW_FLAG,      // an integer: 0 = off, any other = on
    ADF_SW_PRESENT,   // set at all, whatever the value = on
    ADF_SW_WORD,      // the expected word = `hit`, any other string = !hit
    ADF_SW_POSINT     // a positive integer (the int64 field)
};
struct adf_switch_row { const char* name; adf_switch_kind kind; const char* word; int32_t hit; int64_t unset; size_t field; };

// The switches as the environment sets them now.  A flag or a count that is no integer - a word, an integer with something
// behind it, an empty string - leaves the default, as an unset variable does.  Handles copy the struct at creation
// (a twin follows its parent); adf_linear_forward takes ADF_LIFT from a fresh read at each call.
inline adf_switches adf_switches_from_env() {
#define ADF_SW_FIELD(f) offsetof(adf_switches, f)
    static const adf_switch_row table[] = {
        // variable, kind, word, value of the word, value when unset or malformed, field
        {"ADF_GEMM_STREAM", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(tune.gemm_stream)},
        {"ADF_HEAD_GATE_FUSED", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(tune.head_gate_fused)},
        {"ADF_LIFT_EMIT", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(tune.lift_emit)},
        {"ADF_GRAPH_SYS_CSR", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(tune.graph_sys_csr)},
        {"ADF_TRAIN_GEMM", ADF_SW_WORD, "f32", 0, 1, ADF_SW_FIELD(tune.train_gemm16)},
        {"ADF_WGRAD", ADF_SW_WORD, "f32", 1, 0, ADF_SW_FIELD(tune.wgrad_f32)},
        {"ADF_EQV2_GEMM_TILE", ADF_SW_WORD, "128", 0, 1, ADF_SW_FIELD(tune.eqv2_gemm_tile256)},
        {"ADF_EQV2_ROTIN_GENERIC", ADF_SW_PRESENT, nullptr, 0, 0, ADF_SW_FIELD(tune.eqv2_rotin_generic)},
        {"ADF_EQV2_ROTOUT_GENERIC", ADF_SW_PRESENT, nullptr, 0, 0, ADF_SW_FIELD(tune.eqv2_rotout_generic)},
        {"ADF_SAMPLE_SPLIT", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(tune.sample_split)},
        {"ADF_INCREMENTAL", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(incremental)},
        {"ADF_INC_SYNC", ADF_SW_FLAG, nullptr, 0, 0, ADF_SW_FIELD(inc_sync)},
        {"ADF_GEMM", ADF_SW_WORD, "f32", 1, 0, ADF_SW_FIELD(gemm_f32)},
        {"ADF_LIFT", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(lift)},
        {"ADF_MSG", ADF_SW_WORD, "f32", 1, -1, ADF_SW_FIELD(msg_f32)},   // unset: follows ADF_GEMM, below
        {"ADF_MSG_RBF", ADF_SW_WORD, "direct", 1, 0, ADF_SW_FIELD(msg_rbf_direct)},
        {"ADF_ROW_MAXIMA", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(row_maxima)},
        {"ADF_EQV2_S2_EMIT", ADF_SW_FLAG, nullptr, 0, 0, ADF_SW_FIELD(eqv2_s2_emit)},
        {"ADF_EQV2_PRESPLIT", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(eqv2_presplit)},
        {"ADF_EQV2_CONV1_WR", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(eqv2_conv1_wr)},
        {"ADF_EQV2_CONV2_WR", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(eqv2_conv2_wr)},
        {"ADF_EQV2_ALPHA_GENERIC", ADF_SW_FLAG, nullptr, 0, 0, ADF_SW_FIELD(eqv2_alpha_generic)},
        {"ADF_EQV2_FOLD", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(eqv2_fold)},
        {"ADF_EQV2_COMPACT", ADF_SW_FLAG, nullptr, 0, 1, ADF_SW_FIELD(eqv2_compact)},
        {"ADF_EQV2_RADIAL", ADF_SW_WORD, "edge", 1, 0, ADF_SW_FIELD(eqv2_radial_edge)},
        {"ADF_EQV2_CHUNK_EDGES", ADF_SW_POSINT, nullptr, 0, 1 << 19, ADF_SW_FIELD(eqv2_chunk_edges)},
    };
#undef ADF_SW_FIELD
    adf_switches s = {};
    for (const adf_switch_row& r : table) {
        const char* e = getenv(r.name);
        char* end = nullptr;
        errno = 0;
        const long long n = e ? strtoll(e, &end, 10) : 0;
        const bool integer = e && end != e && *end == '\0' && errno == 0;   // the whole string, in range
        int64_t v = r.unset;
        if (r.kind == ADF_SW_FLAG && integer) v = n != 0;
        if (r.kind == ADF_SW_PRESENT) v = e != nullptr;
        if (r.kind == ADF_SW_WORD && e) v = strcmp(e, r.word) == 0 ? r.hit : !r.hit;
        if (r.kind == ADF_SW_POSINT && integer && n > 0) v = n;
        char* field = reinterpret_cast<char*>(&s) + r.field;
        if (r.kind == ADF_SW_POSINT) *reinterpret_cast<int64_t*>(field) = v;
        else *reinterpret_cast<int32_t*>(field) = (int32_t)v;
    }
    if (s.msg_f32 < 0) s.msg_f32 = s.gemm_f32;
    return s;
}
// Callers without a handle (adf_eqv2_linear_forward, adf_linear_forward's kernel selection, the adf_op_* / tr_* operators of
// train.hip) share one copy, read at its first use in the process; the initialisation is thread-safe.
inline const adf_switches& adf_switches_process() {
    static const adf_switches s = adf_switches_from_env();
    return s;
}
