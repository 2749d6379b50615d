// grx_sort.h -- what the 64-bit LSD radix sort (grx_sort.hip) shares with the window sort of grx_prune.hip and the
// median of grx_aggx.hip: the tile shape, the order keys of fp64 values and the workspace plan.
#pragma once
#include "grx_common.h"

constexpr int SORT_THREADS = 256;
constexpr int SORT_ITEMS = 16;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;     // 4096 keys per workgroup
constexpr int RADIX = 256;

// total order of the doubles as unsigned integers, and back
__device__ __forceinline__ uint64_t f64_to_key(double x)
{
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

__device__ __forceinline__ double key_to_f64(uint64_t k)
{
    const uint64_t b = k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull);
    return __longlong_as_double((long long)b);
}

struct SortPlan {
    int ntiles;
    size_t keys_bytes;      // one key buffer: ncols * n * 8
    size_t hist_bytes;      // ncols * RADIX * ntiles * 4
};

static inline SortPlan make_plan(int64_t n, int ncols)
{
    SortPlan p;
    p.ntiles = (int)grx_ceil_div(n, SORT_TILE);
    p.keys_bytes = grx_align_up((size_t)ncols * (size_t)n * 8, 256);
    // per-tile counters + digit totals + digit bases
    p.hist_bytes = grx_align_up((size_t)ncols * RADIX * (size_t)p.ntiles * 4, 256) +
                   2 * grx_align_up((size_t)ncols * RADIX * 4, 256);
    return p;
}
