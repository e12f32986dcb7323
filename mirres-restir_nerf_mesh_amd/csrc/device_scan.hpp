// device_scan.hpp — the wave64 / workgroup prefix sums and the radix sorts' digit matching, written once for every kernel of the library.
//
// INTEGERS ONLY.  An integer sum is the same bits in any order, so every caller gets what its own hand-written scan gave.  A floating-point sum has an order
// that is part of the result (passes.hip's k_env_rows / k_env_marginal fix theirs and keep it): it must not go through these scans.
//
// Barrier contract.  wave_incl_scan and wave_digit_rank contain no barrier and need the whole wave to arrive (they shuffle and ballot across its 64 lanes).
// block_excl_scan and block_append contain __syncthreads, so EVERY thread of the workgroup must call them, the same number of times, lanes with nothing to
// add passing zero (no early return before them); their LDS words are free again on return, so a kernel may call them in a loop or twice in a row.
#pragma once
#include "device_math.hpp"

namespace mr {

MR_DEV int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// inclusive prefix sum over the wave's 64 lanes; T = uint32_t or unsigned long long (the 64-bit shuffle moves both halves, the add carries between them)
template <typename T>
MR_DEV T wave_incl_scan(T v) {
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const T t = __shfl_up(v, off, 64); if (lane >= off) v += t; }
    return v;
}

// exclusive prefix sum of one value per thread over a BLOCK-thread workgroup (thread order): wave scans + the BLOCK / 64 wave totals through sh[BLOCK / 64].
// total = the workgroup's sum, in every thread.  Every thread of the workgroup must call it; sh is reusable on return (the trailing barrier is inside).
template <int BLOCK, typename T>
MR_DEV T block_excl_scan(T v, T* sh, T& total) {
    static_assert(BLOCK % 64 == 0 && BLOCK >= 64 && BLOCK <= 1024, "whole waves, one workgroup");
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const T inc = wave_incl_scan(v);
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) { const T t = sh[w]; if (w < wave) before += t; all += t; }
    __syncthreads();
    total = all;
    return before + inc - v;
}

// Block-level compacted append: ONE global atomic per workgroup (a single queue-head word saturates at ~88 atomics/us on MI355X, and the
// per-wave version made every ray-generating kernel atomic-bound: 17 k wave atomics = 195 us for a kernel that moves 150 MB).
// Every thread of the block must call it (three __syncthreads). `n` rays are reserved for lanes with `want`. The wave count is blockDim's, at run time.
MR_DEV uint32_t block_append(uint32_t* counter, bool want, uint32_t n = 1) {
    __shared__ uint32_t s_wave[17];
    const uint32_t mine = want ? n : 0u;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
    const uint32_t incl = wave_incl_scan(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < nwaves; w++) { uint32_t t = s_wave[w]; s_wave[w] = tot; tot += t; }
        s_wave[16] = tot ? atomicAdd(counter, tot) : 0u;
    }
    __syncthreads();
    const uint32_t r = s_wave[16] + s_wave[wave] + incl - mine;
    __syncthreads();   // s_wave may be reused by a second append in the same kernel
    return r;
}

// One round of a radix sort's stable scatter, for the wave's 64 keys: the lanes holding the same 8-bit digit d find each other with eight ballots (wave64
// match), the lowest of them bumps the wave's own counter of that digit in row[256] (LDS), and the key's rank among the wave's keys of that digit so far
// = the counter before the bump + the matching lower lanes.  Invalid lanes (past the end of the keys) count nowhere.  No barrier inside: the caller puts
// one between rounds (the next round's leaders read what this round's leaders wrote) and before it reads the counters.
MR_DEV uint32_t wave_digit_rank(uint32_t d, bool valid, uint32_t* row) {
    const int lane = lane_id();
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) { const bool bit = (d >> b) & 1u; const uint64_t bal = __ballot(bit); m &= bit ? bal : ~bal; }
    // m = the valid lanes of this round with the same digit (this lane included when it is valid)
    const int leader = valid ? __builtin_ctzll(m) : lane;
    uint32_t prev = 0u;
    if (valid && lane == leader) { prev = row[d]; row[d] = prev + (uint32_t)__popcll(m); }
    prev = (uint32_t)__shfl((int)prev, leader, 64);
    const uint64_t lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    return prev + (uint32_t)__popcll(m & lt_mask);
}

}  // namespace mr
