// rc_reduce.h -- what the per-slot product kernels share on the way from a lane's sum to the launch's last block: wave reductions,
// the accumulator words in memory, and the hand-off to the last-arriving block.  Nothing of one product, and not for the Farneback
// hot path.
#pragma once

#include "rc_device.h"

// ---------------------------------------------------------------------------------------------------- wave reductions
// Two forms of each, and the name says where the result is.  _all: a butterfly (__shfl_xor), the total in every lane.  _lane0: a
// fold towards lane 0 (__shfl_down), the total in lane 0 and nothing of use elsewhere.  Floating point adds in the tree the
// shuffle gives, 32 16 8 4 2 1 apart; lane 0 adds the same pairs in the same order in both forms, so its bits are the same.
template <typename T>
__device__ __forceinline__ T rc_wave_sum_all(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T rc_wave_sum_lane0(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ int rc_wave_max_all(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned rc_wave_max_all(unsigned v) {      // as a rule the bits of floats that are not negative
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ float rc_wave_max_lane0(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------- runs of lanes
// The wave's lanes fall into runs of consecutive lanes with one key (a cell, a pixel; -1 for none): where neighbours in memory are
// neighbours in the picture the runs are long, and a run needs one atomic per word, not one per lane (the drifters, the offshore
// table).  Every lane of the wave calls these.  -> the last lane of the lane's run; head: the lane is its run's first
__device__ __forceinline__ int rc_run(int key, int lane, bool& head) {
    const int prev = __shfl_up(key, 1, 64);
    head = lane == 0 || key != prev;
    const unsigned long long heads = __ballot(head);
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    return after ? lane + __ffsll((long long)after) - 1 : 63;
}
// the sum of v over the lane's run from the lane on: in the run's first lane, the run's sum
__device__ __forceinline__ long long rc_run_sum(long long v, int lane, int end) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_down(v, o, 64);
        if (lane + o <= end) v += t;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------- accumulator words
// Words in memory that every block of a launch adds to and the last block reads.  Relaxed, agent scope: each is one atomic
// performed in L2, which orders nothing else; what orders them against the ticket is the hand-off below.
template <typename T>
__device__ __forceinline__ void rc_acc_add(T* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T rc_acc_add_old(T* p, T v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T rc_acc_load(T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// read and zero in one operation, where the adds were made
__device__ __forceinline__ long long rc_acc_take(long long* p) { return __hip_atomic_exchange(p, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long rc_acc_take(unsigned long long* p) { return __hip_atomic_exchange(p, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned rc_acc_take(unsigned* p) { return __hip_atomic_exchange(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------------------------------- the hand-off
// A ticket word that every block adds to takes a 128-byte line of its own
struct RcTicketLine { unsigned ticket; unsigned pad[31]; };
static_assert(sizeof(RcTicketLine) == 128, "a line");

// The contract, for both dialects below.
//   Before the call   the block has issued everything the last block is to find: its rc_acc_add's, and plain stores to memory
//                     that the last block reads.  The _ticket forms are called by the one thread that issued all of it (or after a
//                     barrier of the caller's that followed it); the _hand_off forms are called by every thread of the block, from
//                     uniform control flow, and `last` is an int in LDS.
//   After it          it returns true in exactly one block of the launch: the one whose arrival was the n-th (n: the launch's
//                     blocks, or the arrivals the ticket is shared by).  There, every other arrival's adds and stores are visible:
//                     to the calling thread for the _ticket forms, to every thread of the block for the _hand_off forms, whose
//                     second barrier passes the flag and the acquire on.  A block that gets false has nothing more to read and leaves.
//   The ticket        counts up from zero and is left at n.  The caller of the last block stores zero to it when it has finished
//                     with the totals, and takes (rc_acc_take) or zeroes what it read, so that the next push, which stream order
//                     puts behind this launch, finds ticket and words zero.  Nothing in here re-zeroes.
//
// The release dialect: ONE release a block.  s_waitcnt vmcnt(0) first, in every wave: the wave's stores and atomics have been
// performed where agent scope performs them (L2) before the barrier lets thread 0 go on; thread 0's release fence then writes back
// what needs it, the second wait drains that, and only then the ticket.  The last arriver's acquire invalidates what its CU may
// hold of the other blocks' lines.  The waits are explicit because the fence of one thread does not wait for another wave's counters.
__device__ __forceinline__ void rc_wait_performed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ bool rc_released_ticket_(unsigned* ticket, unsigned n) {   // what follows the first wait
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    rc_wait_performed();
    const bool l = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n - 1u;
    if (l) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return l;
}
__device__ __forceinline__ bool rc_ticket_release(unsigned* ticket, unsigned n) {
    rc_wait_performed();
    return rc_released_ticket_(ticket, n);
}
__device__ __forceinline__ bool rc_hand_off_release(unsigned* ticket, unsigned n, int* last) {
    rc_wait_performed();
    __syncthreads();
    if (threadIdx.x == 0) *last = rc_released_ticket_(ticket, n);
    __syncthreads();
    return *last != 0;
}

// The fenced dialect: __threadfence() (sequentially consistent, agent scope) before the ticket, by the one thread or by every
// thread of the block, and once more after it in the last arriver only: the second fence serves the reader of the totals, and
// only the last block reads.
__device__ __forceinline__ bool rc_fenced_ticket_(unsigned* ticket, unsigned n) {     // what follows the first fence
    const bool l = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == n - 1u;
    if (l) __threadfence();
    return l;
}
__device__ __forceinline__ bool rc_ticket_fenced(unsigned* ticket, unsigned n) {
    __threadfence();
    return rc_fenced_ticket_(ticket, n);
}
__device__ __forceinline__ bool rc_hand_off_fenced(unsigned* ticket, unsigned n, int* last) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) *last = rc_fenced_ticket_(ticket, n);
    __syncthreads();
    return *last != 0;
}

// The closings without a fence (pv_arrive in planview_kernels.hip, wv_arrive in waves_kernels.hip) are protocols of their own and
// stay with their kernels; the argument they rest on is this.  A release at agent scope writes the L2's dirty lines back, and a
// launch that has just dirtied all of its output pays for that in every block: 1024 blocks ending in __threadfence took 90 to 180 us
// whatever the plan's size.  Where nothing but atomics passes between blocks, a fence orders what needs no order.  What is needed:
// the block that draws the last ticket finds every block's sums.  An atomic that RETURNS its old value has been performed, where
// agent scope performs atomics, once the wave's vmcnt has counted it.  So either the ticket's operand is made from the values the
// block's other atomics returned (planview: a data dependency, always zero), or every add asks for its old value and the wave
// waits (rc_wait_performed) before the barrier and the ticket (waves).  The last block's exchanges are issued after its ticket
// returned, through the branch on it.  This is an argument about gfx950, not one the HIP memory model makes: relaxed atomics order
// nothing there.  A port to another architecture, or a compiler that no longer waits for an atomic's returned value as for a
// load's, needs rc_ticket_release in the ticket's place.

// ---------------------------------------------------------------------------------------------------- small shared pieces
__device__ __forceinline__ long long rc_floor_div(long long a, long long b) {   // b > 0
    const long long q = a / b;
    return q - (a % b != 0 && a < 0);
}

// the 768-byte colour table into LDS, by a block of RC_BLOCK threads; the caller's barrier follows
__device__ __forceinline__ void rc_stage_jet(uint8_t* lut, const uint8_t* src) {
    for (int i = threadIdx.x; i < 768; i += RC_BLOCK) lut[i] = src[i];
}
