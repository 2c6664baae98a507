// The summary of a batched pass over gnark point arrays (OK, infinity, rejected, first rejected index): shared by the decoding
// kernels of gnark_points.hip and the encoding kernels of gnark_points_encode.hip.  Ballots per wave, the four waves of a workgroup
// meet through LDS, lane 0 adds with ordinary atomics (at most four per workgroup) into words a one-lane kernel has set.
// Internal to those two files (static: each is its own translation unit, no relocatable device code).
#pragma once
#include "gnark_points.cuh"

#define GK_LANES 256u
#define GK_WAVES (GK_LANES / 64u)
#define GK_MAX_POINTS (1ull << 31)

static __global__ void gk_summary_init_kernel(u64 *__restrict__ summary) {
    summary[0] = summary[1] = summary[2] = 0;
    summary[3] = ~0ull;
}

// every lane of the workgroup calls this once (live = 0: a lane behind the end of the array)
static __device__ __forceinline__ void gk_count(u32 st, u32 live, u64 idx, u64 *__restrict__ summary) {
    __shared__ u32 cnt[GK_WAVES][3];
    __shared__ u64 first[GK_WAVES];
    const u64 b_ok = __ballot(live && st == GK_OK), b_inf = __ballot(live && st == GK_INFINITY), b_rej = __ballot(live && st >= GK_BAD_ENCODING);
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) {
        cnt[wave][0] = (u32)__popcll(b_ok);
        cnt[wave][1] = (u32)__popcll(b_inf);
        cnt[wave][2] = (u32)__popcll(b_rej);
        first[wave] = b_rej ? idx + (u64)(__ffsll((unsigned long long)b_rej) - 1) : ~0ull;   // idx: this wave's first point
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 c[3] = {0, 0, 0}, f = ~0ull;
    for (u32 w = 0; w < GK_WAVES; w++) {
        for (int j = 0; j < 3; j++) c[j] += cnt[w][j];
        f = first[w] < f ? first[w] : f;
    }
    for (int j = 0; j < 3; j++)
        if (c[j]) atomicAdd((unsigned long long *)summary + j, (unsigned long long)c[j]);
    if (c[2]) atomicMin((unsigned long long *)summary + 3, (unsigned long long)f);
}
