// grx_peel.h -- the bucket peeling that grx_kcore.hip (nodes by degree) and grx_truss.hip (edges by support) share: a
// level-synchronous peel whose frontier is a list, not a scan.
//
//   thr = 0, round = 1, every item alive with a value (degree, support)
//   while an item is alive:
//       F = {alive i : value(i) <= thr}          if empty: thr = min value over the alive items, then F
//       the caller's kernels: F leaves, and the values of what F touches go down
//       round += 1
//
// An item that is alive and outside F at the start of a round has value > thr, so the F of the next round is exactly
// the set of items some decrement of this round takes from above thr to thr or below, and of all the decrements an item
// receives exactly one does that (integer atomicSub returns the value before: pl_crosses).  The thread that sees it
// calls the item's leave() there and then and appends the item to the next round's list (pl_append: through an LDS
// buffer per workgroup, one global atomic per workgroup and round on the list counter).  Only when that list comes out
// empty (thr must jump) do two sweeps over all `count` items run: pl_min_kernel (the chip-wide minimum value of the
// alive items: a wavefront reduction, one integer atomicMin per workgroup) and pl_collect_kernel (F by the new thr,
// appended one atomic per wavefront).  A one-thread pl_finalize_kernel subtracts |F| from the alive count, advances
// `round` or sets `done`, and raises the sweep flag when the next list is empty; the rounds run as a device-steered
// round loop (grx_common.h).  Integer arithmetic only; the order of the lists is never visible in a result.
//
// The items are a struct of kernel arguments with
//   PlLists pl;                                              the two lists and the control words
//   bool alive(int64_t i) const;                             i has not left and is in no list
//   int value(int64_t i) const;                              what the threshold is compared with
//   void leave(int64_t i, int round, int thr) const;         i is in the F of `round`, at threshold thr: the state word
//                                                            and the caller's outputs
// Everything has internal linkage; the items are a template argument, so every call inlines.
#pragma once
#include "grx_common.h"

#include <climits>

namespace {

constexpr int PL_BLOCK = 256;                                // threads of the sweeps, and of every kernel that appends
constexpr int PL_SWEEP_MAX_WG = 2048;                        // workgroups of the two sweeps (grid-stride above that)
constexpr int PL_APPEND_CAP = 2048;                          // LDS append buffer of a workgroup (entries)

// words 0 and 1 where grx_run_rounds and every round loop have them; PL_LEVELS counts the sweeps that found a new thr
enum { PL_DONE = 0, PL_ROUND, PL_THR, PL_MIN, PL_SWEEP, PL_ALIVE, PL_CNT0, PL_CNT1, PL_LEVELS, PL_WORDS };
static_assert(PL_WORDS <= GRX_CTRL_MAX_WORDS, "control words: one pinned block");

struct PlLists {
    int32_t *list0, *list1, *ctrl;                           // int32[count] each, and int32[PL_WORDS]
};

// what a round's kernels read from ctrl: the list of this round (F) and the one they append to
struct PlRound {
    int round, thr, count;
    const int32_t *cur;
    int32_t *next, *next_count;
};

__device__ __forceinline__ PlRound round_of(const PlLists &p)
{
    PlRound r;
    r.round = p.ctrl[PL_ROUND];
    r.thr = p.ctrl[PL_SWEEP] ? max(p.ctrl[PL_THR], p.ctrl[PL_MIN]) : p.ctrl[PL_THR];
    const int odd = r.round & 1;
    r.count = p.ctrl[PL_CNT0 + odd];
    r.cur = odd ? p.list1 : p.list0;
    r.next = odd ? p.list0 : p.list1;
    r.next_count = &p.ctrl[PL_CNT0 + (odd ^ 1)];
    return r;
}

// `old` was above the threshold and old - c is not: the one decrement of an item that takes it into the next F
__device__ __forceinline__ bool pl_crosses(int old, int c, int thr) { return old > thr && old - c <= thr; }

// the appends of a workgroup in one round (__shared__; thread 0 zeroes `count` before a barrier)
struct PlAppends {
    int32_t buf[PL_APPEND_CAP];
    int count, base;
};

// one item into the next round's list: through the workgroup's buffer, directly beyond its cap
__device__ __forceinline__ void pl_append(int32_t item, const PlRound &r, PlAppends &a)
{
    const int slot = atomicAdd(&a.count, 1);
    if (slot < PL_APPEND_CAP) a.buf[slot] = item;
    else r.next[atomicAdd(r.next_count, 1)] = item;
}

// the workgroup's buffered appends, one atomic on the list counter; every thread of the workgroup calls it
__device__ __forceinline__ void pl_flush(const PlRound &r, PlAppends &a)
{
    __syncthreads();
    const int c = min(a.count, PL_APPEND_CAP);
    if (threadIdx.x == 0 && c) a.base = atomicAdd(r.next_count, c);
    __syncthreads();
    for (int i = threadIdx.x; i < c; i += PL_BLOCK) r.next[a.base + i] = a.buf[i];
}

// by one thread, before the first round: `alive` items, no list, the first round sweeps
__device__ __forceinline__ void pl_init_ctrl(int32_t *ctrl, int32_t alive)
{
    ctrl[PL_DONE] = 0; ctrl[PL_ROUND] = 1; ctrl[PL_THR] = 0; ctrl[PL_MIN] = INT_MAX; ctrl[PL_SWEEP] = 1;
    ctrl[PL_ALIVE] = alive; ctrl[PL_CNT0] = 0; ctrl[PL_CNT1] = 0; ctrl[PL_LEVELS] = 0;
}

// sweep 1 (only when the list is empty): min value over the alive items
template <class Items>
__global__ __launch_bounds__(PL_BLOCK) void pl_min_kernel(int64_t count, const Items items)
{
    __shared__ int smin;
    int32_t *ctrl = items.pl.ctrl;
    if (ctrl[PL_DONE] || !ctrl[PL_SWEEP]) return;
    if (threadIdx.x == 0) smin = INT_MAX;
    __syncthreads();
    int m = INT_MAX;
    for (int64_t i = (int64_t)blockIdx.x * PL_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * PL_BLOCK)
        if (items.alive(i)) m = min(m, items.value(i));
#pragma unroll
    for (int off = GRX_WAVE / 2; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, GRX_WAVE));
    if (threadIdx.x % GRX_WAVE == 0 && m < INT_MAX) atomicMin(&smin, m);
    __syncthreads();
    if (threadIdx.x == 0 && smin < INT_MAX) atomicMin(&ctrl[PL_MIN], smin);
}

// sweep 2: F = the alive items with value <= max(thr, min), appended one atomic per wavefront
template <class Items>
__global__ __launch_bounds__(PL_BLOCK) void pl_collect_kernel(int64_t count, const Items items)
{
    int32_t *ctrl = items.pl.ctrl;
    if (ctrl[PL_DONE] || !ctrl[PL_SWEEP]) return;
    const int round = ctrl[PL_ROUND];
    const int thr = max(ctrl[PL_THR], ctrl[PL_MIN]);
    int32_t *cur = (round & 1) ? items.pl.list1 : items.pl.list0;
    int32_t *cur_count = &ctrl[PL_CNT0 + (round & 1)];
    const int lane = threadIdx.x % GRX_WAVE;
    // the trip count is the same in every lane of the workgroup: the ballot sees every lane
    for (int64_t first = (int64_t)blockIdx.x * PL_BLOCK; first < count; first += (int64_t)gridDim.x * PL_BLOCK) {
        const int64_t i = first + threadIdx.x;
        const bool leaves = i < count && items.alive(i) && items.value(i) <= thr;
        const unsigned long long m = __ballot(leaves);
        if (!m) continue;
        int base = 0;
        if (lane == 0) base = atomicAdd(cur_count, __popcll(m));
        base = __shfl(base, 0, GRX_WAVE);
        if (leaves) {
            cur[base + __popcll(m & ((1ull << lane) - 1))] = (int32_t)i;
            items.leave(i, round, thr);
        }
    }
}

// one thread: F has left; the next round, or done when nothing is alive.  An empty next list asks for the sweeps
__global__ void pl_finalize_kernel(int32_t *ctrl)
{
    if (ctrl[PL_DONE]) return;
    const int odd = ctrl[PL_ROUND] & 1;
    if (ctrl[PL_SWEEP]) {
        ctrl[PL_THR] = max(ctrl[PL_THR], ctrl[PL_MIN]);
        ctrl[PL_LEVELS] += 1;                                // every sweep finds a thr above the last one
    }
    ctrl[PL_ALIVE] -= ctrl[PL_CNT0 + odd];
    ctrl[PL_CNT0 + odd] = 0;
    ctrl[PL_MIN] = INT_MAX;
    if (ctrl[PL_ALIVE] <= 0) {
        ctrl[PL_DONE] = 1;                                   // PL_ROUND stays: the number of rounds run
        return;
    }
    ctrl[PL_SWEEP] = ctrl[PL_CNT0 + (odd ^ 1)] == 0;
    ctrl[PL_ROUND] += 1;
}

// the two sweeps of a round over `count` items; early returns unless the round's list is empty
template <class Items>
void pl_sweeps(int64_t count, const Items &items, hipStream_t st)
{
    const unsigned grid = grx_grid(count, PL_BLOCK, PL_SWEEP_MAX_WG);
    pl_min_kernel<<<grid, PL_BLOCK, 0, st>>>(count, items);
    pl_collect_kernel<<<grid, PL_BLOCK, 0, st>>>(count, items);
}

}  // namespace
