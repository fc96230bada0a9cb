// Host side shared by the slab-preparation entries: the device error word and the scratch carver.
#pragma once
#include <limits.h>

#include "base.h"

// One row of an entry's error table.  fmt is a printf format of (who, a, b): a "%s" first, then up to two "%d".
// a == ADF_ERR_ATOM stands for the error word's second word (the least offending atom).
#define ADF_ERR_ATOM INT_MIN
struct adf_errrow {
    int32_t bit, status;
    const char* fmt;
    int a, b;
};

// The device error word of one entry call: kernels atomicOr bits into word 0; with two words, word 1 starts at 0x7f7f7f7f
// and takes an atomicMin of the offending atom.  Either the word is its own allocation (create) or it lies in a block the
// caller carved (adopt).  finish() is the call's one read-back and synchronisation; the word is freed with this object, so
// keep it alive until finish() has returned.
struct adf_errword {
    int32_t* dev = nullptr;
    int words = 1;
    adf_pool own;
    int32_t create(hipStream_t s, int n_words = 1) {
        ADF_TRY(own.alloc(&dev, (size_t)n_words));
        return adopt(dev, s, n_words);
    }
    int32_t adopt(int32_t* p, hipStream_t s, int n_words = 1) {
        dev = p;
        words = n_words;
        ADF_HIP_CHECK(hipMemsetAsync(dev, 0, sizeof(int32_t), s));
        if (words == 2) ADF_HIP_CHECK(hipMemsetAsync(dev + 1, 0x7f, sizeof(int32_t), s));
        return ADF_OK;
    }
    // copy back, synchronise, report the first row of `rows` (priority order) whose bit is set
    int32_t finish(hipStream_t s, const char* who, const adf_errrow* rows, int n) {
        int32_t bad[2] = {0, 0};
        ADF_HIP_CHECK(hipMemcpyAsync(bad, dev, words * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        ADF_HIP_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i)
            if (bad[0] & rows[i].bit) {
                adf_set_error(rows[i].fmt, who, rows[i].a == ADF_ERR_ATOM ? bad[1] : rows[i].a, rows[i].b);
                return rows[i].status;
            }
        return ADF_OK;
    }
    template <int N>
    int32_t finish(hipStream_t s, const char* who, const adf_errrow (&rows)[N]) { return finish(s, who, rows, N); }
};

// Bump allocator over one block: run the same sequence of take<T>() calls twice, first on a null base to measure
// (bytes()), then on the block.  Every region starts at a multiple of max(alignof(T), align) from the base, and bytes() is
// rounded up to `align`.
struct adf_carver {
    unsigned char* base;
    size_t align, used = 0;
    explicit adf_carver(void* block = nullptr, size_t min_align = 1) : base((unsigned char*)block), align(min_align) {}
    template <typename T>
    T* take(size_t count) {
        const size_t al = alignof(T) > align ? alignof(T) : align;
        used = (used + al - 1) / al * al;
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return (used + align - 1) / align * align; }
};
