// gs_radix.h -- the steps of a stable radix pass over a 4096-key chunk, each written once (device code of gs_sort.hip, gs_bin2.hip and
// gs_bin3.hip; nothing here is exported).  A scatter kernel is: rank every key among its wave's earlier same-digit keys (rank_round /
// rank_round_atomic), turn the per-wave counts into offsets (digit_prefixes), PLACE the keys digit-contiguously in LDS (radix_slot)
// and WRITE them out in digit runs (radix_dest).  The block scans the other kernels of these units need are here as well.
#pragma once
#include "gs_common.h"

#define RS_THREADS 256
#define RS_ITEMS 16
#define RS_CHUNK (RS_THREADS * RS_ITEMS)   // 4096 keys per workgroup
#define RS_RADIX 256
#define RS_WAVES (RS_THREADS / GS_WAVE)

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < GS_WAVE; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive prefix of one value per thread over the NT threads of the block.  sm: NT / 64 words, read until the caller's next barrier.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_prefix(uint32_t v, uint32_t *sm) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v, lane);
    if (lane == 63) sm[w] = incl;
    __syncthreads();
    uint32_t pre = incl - v;
    for (int k = 0; k < w; ++k) pre += sm[k];
    return pre;
}

// ---------------------------------------------------------------- stable rank of a key among its wave's earlier same-digit keys
// A wave takes its keys in rounds of 64 (one per lane); the stable order is (round, lane).  wc: the wave's own row of RS_RADIX
// running counters in LDS, zero before the first round.  Two forms:
//  * ballots (portable): 8 wave64 ballots build the set of same-digit lanes, the counter adds the earlier rounds, the set's lowest
//    lane (its leader) stores the new count;
//  * LDS atomic (gs_config.rank_mode = 0): ONE ds_add_rtn_u32 on the counter.  When several lanes of one wave instruction hit the
//    same LDS address, gfx950 hands out the pre-values in ascending lane order (tools/lds_atomic_order.hip: 0 mismatches in 1.7e8
//    lane-ops) -- exactly the stable rank.  Measured behaviour, not an architectural guarantee: gs_create probes it
//    (lds_atomic_order_probe_kernel compares these two functions) and the GPU tests compare every list bit for bit with both.
//
// What keeps the ballot form's counter read and store in order (DESIGN 5.2 has the argument in full).  The row is a plain LDS
// pointer -- a volatile generic one turns ds_read_b32 / ds_write_b32 into flat operations -- and the code relies on three things: the
// stored value is computed from the read; both go through one pointer with a run-time index, so the next round's read may alias the
// store and stays behind it, and no counter is carried in a register; the LDS unit serves a wave's DS instructions in issue order.
// The two wave barriers emit no instruction: they pin the same order for the instruction scheduler.
__device__ __forceinline__ uint32_t rank_round(uint32_t dg, bool valid, int lane, uint32_t *wc) {
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned long long bal = __ballot((dg >> b) & 1u);
        peers &= ((dg >> b) & 1u) ? bal : ~bal;
    }
    const uint32_t before = wc[dg];                                     // same-digit keys of earlier rounds
    const uint32_t rank = before + (uint32_t)__popcll(peers & lt_mask);
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers & lt_mask) == 0ull) wc[dg] = before + (uint32_t)__popcll(peers);   // group leader
    __builtin_amdgcn_wave_barrier();
    return rank;
}
__device__ __forceinline__ uint32_t rank_round_atomic(uint32_t dg, bool valid, uint32_t *wc) {
    return valid ? atomicAdd(&wc[dg], 1u) : 0u;
}

// Exclusive prefix of one value per DIGIT in a block of 256 or more threads (thread d < 256 holds digit d's value, the others take part
// in the barrier only): use(prefix) runs in the digit's thread.  sm: 4 words, read until the caller's next barrier.  (The consumer is
// a callback because a value returned out of the `tid < 256` region changed the vector code of the depth sort's kernels.)
template <typename Use>
__device__ __forceinline__ void digits_excl_prefix(uint32_t v, uint32_t *sm, Use use) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t incl = wave_incl_scan(v, lane);
    if (tid < RS_RADIX && lane == 63) sm[w] = incl;
    __syncthreads();
    if (tid < RS_RADIX) { uint32_t woff = 0; for (int k = 0; k < w; ++k) woff += sm[k]; use(woff + incl - v); }
}

// After the ranking (and a barrier), with all NW * 64 >= 256 threads, thread `tid` == digit: wcnt[k][d] becomes the exclusive offset
// of wave k among the chunk's keys of digit d, lpre[d] the first slot of digit d in the digit-ordered chunk.  Returns the digit's key
// count (threads beyond 255: 0).  The caller's barrier comes before lpre / wcnt are read.
template <int NW>
__device__ __forceinline__ uint32_t digit_prefixes(uint32_t (*wcnt)[RS_RADIX], uint32_t *lpre, uint32_t *sm) {
    const int tid = threadIdx.x;
    uint32_t tot = 0;
    if (tid < RS_RADIX) {
#pragma unroll
        for (int k = 0; k < NW; ++k) { const uint32_t c = wcnt[k][tid]; wcnt[k][tid] = tot; tot += c; }
    }
    digits_excl_prefix(tot, sm, [=](uint32_t pre) { lpre[tid] = pre; });
    return tot;
}
// the chunk's ranked keys, in every thread: the sum over the digits, from the sm digit_prefixes left (before the caller's next barrier)
__device__ __forceinline__ uint32_t ranked_keys(const uint32_t *sm) { return sm[0] + sm[1] + sm[2] + sm[3]; }
// place: the slot of a key of digit dg and rank `rank` of the wave whose offsets row is wc
__device__ __forceinline__ uint32_t radix_slot(const uint32_t *lpre, const uint32_t *wc, uint32_t dg, uint32_t rank) { return lpre[dg] + wc[dg] + rank; }
// write runs: where the key in slot li (digit dg) goes, gbase[d] = first output position of this chunk's keys of digit d
__device__ __forceinline__ size_t radix_dest(const uint32_t *gbase, const uint32_t *lpre, uint32_t dg, int li) {
    return (size_t)gbase[dg] + (uint32_t)(li - (int)lpre[dg]);
}

// Elements a workgroup holds in registers, wave-striped: wave w owns the `per` consecutive elements from w * per on, round r of the
// wave the 64 from r * 64 on.  (wave, round, lane) ascending == element ascending: the stable order.
#define RS_LI(w, r, lane, per) ((w) * (per) + (r) * GS_WAVE + (lane))
// The stable scatter of one chunk whose cnt keys the NT threads hold that way (per = 64 * ITEMS), stored by store(position, key) in
// digit runs.  wcnt is zero and gbase is set on entry, with a barrier behind both.
template <int NT, bool ATOMIC_RANK, typename K, typename DigitOf, typename Store>
__device__ __forceinline__ void radix_scatter_chunk(const K (&key)[RS_CHUNK / NT], int cnt, DigitOf digit_of, Store store, K *skeys,
                                                    uint32_t (*wcnt)[RS_RADIX], uint32_t *lpre, const uint32_t *gbase, uint32_t *sm) {
    constexpr int NW = NT / GS_WAVE, ITEMS = RS_CHUNK / NT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t rank[ITEMS];
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const bool valid = RS_LI(w, r, lane, GS_WAVE * ITEMS) < cnt;
        const uint32_t dg = valid ? digit_of(key[r]) : (RS_RADIX - 1);
        rank[r] = ATOMIC_RANK ? rank_round_atomic(dg, valid, wcnt[w]) : rank_round(dg, valid, lane, wcnt[w]);
    }
    __syncthreads();
    digit_prefixes<NW>(wcnt, lpre, sm);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ITEMS; ++r)
        if (RS_LI(w, r, lane, GS_WAVE * ITEMS) < cnt) skeys[radix_slot(lpre, wcnt[w], digit_of(key[r]), rank[r])] = key[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
        const int li = r * NT + tid;
        if (li < cnt) { const K k = skeys[li]; store(radix_dest(gbase, lpre, digit_of(k), li), k); }
    }
}

// host: the rank-mode choice of a scatter launch, made in one place, between the kernel's two instantiations
template <typename... P, typename... A>
inline void rs_launch_ranked(bool ballot_ranks, void (*ballot)(P...), void (*atomic)(P...), dim3 grid, dim3 block, hipStream_t s, A... args) {
    hipLaunchKernelGGL(ballot_ranks ? ballot : atomic, grid, block, 0, s, args...);
}
