// What every translation unit of libadsorbdiff_hip.so needs: the public header, the status macros, the error text, the
// one owner type of device memory and the event profiler.  Nothing model-specific lives here (common.h: the PaiNN handle).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/adsorbdiff_hip.h"

void adf_set_error(const char* fmt, ...);

#define ADF_HIP_CHECK(expr)                                                             \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            adf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                          __FILE__, __LINE__);                                          \
            return (_e == hipErrorOutOfMemory) ? ADF_EOOM : ADF_EHIP;                   \
        }                                                                               \
    } while (0)

#define ADF_TRY(expr)                     \
    do {                                  \
        int32_t _s = (expr);              \
        if (_s != ADF_OK) return _s;      \
    } while (0)

// ---- device memory: the one owner type.  A pool fills pointer fields (of a handle, or locals of the function that holds
// the pool) and remembers their ADDRESSES, so it frees whatever a field holds at release time (fields that are swapped
// among themselves stay correct) and nulls the field itself.  Handles are heap objects: their fields do not move.
// It never synchronises: the caller does where enqueued work may still use the buffers.
struct adf_pool {
    std::vector<void**> slots;
    adf_pool() = default;
    adf_pool(const adf_pool&) = delete;
    adf_pool& operator=(const adf_pool&) = delete;
    ~adf_pool() { release(); }
    // *field = new buffer of `bytes` bytes (0 is rounded up: a filled field is never null).  A field this pool filled
    // before is re-allocated: its old buffer is freed first.  On failure *field is null.
    int32_t alloc(void** field, size_t bytes) {
        bool known = false;
        for (void** s : slots) known = known || s == field;
        if (known) { if (*field) (void)hipFree(*field); } else slots.push_back(field);
        *field = nullptr;
        if (bytes == 0) bytes = 16;
        const hipError_t e = hipMalloc(field, bytes);
        if (e == hipSuccess) return ADF_OK;
        *field = nullptr;
        (void)hipGetLastError();
        adf_set_error("device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
        return ADF_EOOM;
    }
    template <typename T>
    int32_t alloc(T** field, size_t count) { return alloc(reinterpret_cast<void**>(field), count * sizeof(T)); }
    void release() {
        for (void** s : slots) {
            if (*s) (void)hipFree(*s);
            *s = nullptr;
        }
        slots.clear();
    }
};

// ---- HIP-event profiling (bench.py roofline): pairs of events on the launch stream around kernel groups, a category per pair
struct adf_prof {
    bool on = false;
    bool open = false;                // a begin has recorded its event and waits for its end
    std::vector<hipEvent_t> ev;       // pool of events, used pairwise
    std::vector<int> cat;             // category of every recorded pair
    size_t used = 0;                  // events of the finished pairs
    adf_prof() = default;
    adf_prof(const adf_prof&) = delete;
    adf_prof& operator=(const adf_prof&) = delete;
    ~adf_prof() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    // no events to be had: this begin and its end do nothing
    void begin(int c, hipStream_t s) {
        open = false;
        if (!on) return;
        if (used + 2 > ev.size())
            for (int i = 0; i < 512; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); break; }
                ev.push_back(e);
            }
        if (used + 2 > ev.size()) return;
        cat.resize(used / 2);         // (drops a pair that an error return left without its end)
        cat.push_back(c);
        (void)hipEventRecord(ev[used], s);
        open = true;
    }
    void end(hipStream_t s) {
        if (!on || !open) return;
        (void)hipEventRecord(ev[used + 1], s);
        used += 2;
        open = false;
    }
    void enable(bool o) { on = o; open = false; used = 0; cat.clear(); }
    // per category: summed milliseconds and number of pairs since the last read (the stream must be idle); then empty
    int32_t read(float* ms, int64_t* count, int ncat) {
        for (int c = 0; c < ncat; ++c) { ms[c] = 0.f; count[c] = 0; }
        for (size_t i = 0; i < used; i += 2) {
            float t = 0.f;
            ADF_HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            ms[cat[i / 2]] += t;
            count[cat[i / 2]] += 1;
        }
        enable(on);
        return ADF_OK;
    }
    struct scope {
        adf_prof& p; hipStream_t s;
        scope(adf_prof& p_, int c, hipStream_t s_) : p(p_), s(s_) { p.begin(c, s); }
        ~scope() { p.end(s); }
    };
};
