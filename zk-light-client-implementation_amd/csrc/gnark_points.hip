// Batched decoding of gnark point arrays on gfx950 + C ABI (gnark_points.cuh): one lane per point over the bytes of a key file.
//   gk_decode_kernel<G2, COMPRESSED>   four instances.  Raw: two / four 32-byte coordinates in by 16-byte loads, a handful of field
//                                      multiplications, 64 / 128 bytes out by 16-byte stores -- a memory stream.  Compressed: an
//                                      instance of its own, so the square roots (calls of __noinline__ functions) are not in the
//                                      raw instances' register budget.
//   gk_g2_subgroup_kernel              the membership test as a second kernel over the decoded words: lanes whose status is not OK
//                                      skip, the others call the __noinline__ g16_g2_in_subgroup.
// Summary (OK, infinity, rejected, first rejected index): the LAST kernel of a call counts -- ballots per wave, the four waves of a
// workgroup meet through LDS, lane 0 adds with ordinary atomics (at most four per workgroup) into words a one-lane kernel has set.
#include "gnark_points_summary.cuh"   // gk_summary_init_kernel, gk_count: shared with the encoder
#include "groth16_verifier_host.h"
#include "zklc_internal.h"

template <u32 G2, u32 COMPRESSED>
__global__ void __launch_bounds__(GK_LANES)
gk_decode_kernel(const g16_key key, const uint8_t *__restrict__ bytes, u64 n, u32 *__restrict__ words, u32 *__restrict__ status,
                 u64 *__restrict__ summary, u32 count) {
    constexpr u32 STRIDE = (G2 ? 128u : 64u) >> COMPRESSED, QUADS = G2 ? 8u : 4u;
    const u64 i = (u64)blockIdx.x * GK_LANES + threadIdx.x;
    const u32 live = i < n;
    u32 st = GK_INFINITY;
    if (live) {
        u32 o[4 * QUADS];
        if (G2) st = gk_g2_decode<COMPRESSED>(key, bytes + i * STRIDE, o);
        else st = gk_g1_decode<COMPRESSED>(bytes + i * STRIDE, o);
        gk_store_words(words + i * (4 * QUADS), o, QUADS);
        status[i] = st;
    }
    if (count) gk_count(st, live, i, summary);
}

__global__ void __launch_bounds__(GK_LANES)
gk_g2_subgroup_kernel(u32 *__restrict__ words, u32 *__restrict__ status, u64 n, u64 *__restrict__ summary) {
    const u64 i = (u64)blockIdx.x * GK_LANES + threadIdx.x;
    const u32 live = i < n;
    u32 st = live ? status[i] : GK_INFINITY;
    if (live && st == GK_OK) {
        u32 o[32];
        gk_load_words(o, words + i * 32, 8);
        st = gk_g2_subgroup_lane(o);
        if (st != GK_OK) {
            gk_store_words(words + i * 32, o, 8);
            status[i] = st;
        }
    }
    gk_count(st, live, i, summary);
}

static int32_t gk_decode_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_bytes, uint64_t n, uint32_t flags, uint64_t *d_words,
                             uint32_t *d_status, uint64_t *d_summary, bool g2) {
    if (!ctx || !d_summary || (flags & ~(ZKLC_POINTS_COMPRESSED | ZKLC_POINTS_CHECK_SUBGROUP))) return ZKLC_ERR_INVALID_ARG;
    if (!g2 && (flags & ZKLC_POINTS_CHECK_SUBGROUP)) return ZKLC_ERR_INVALID_ARG;
    if (n > GK_MAX_POINTS || (n && (!d_bytes || !d_words || !d_status))) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)d_bytes | (uintptr_t)d_words) & 15 || (uintptr_t)d_status & 3 || (uintptr_t)d_summary & 7) return ZKLC_ERR_INVALID_ARG;
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = zklc_pick_stream(ctx, stream);
    hipLaunchKernelGGL(gk_summary_init_kernel, dim3(1), dim3(1), 0, st, (u64 *)d_summary);
    ZKLC_HIP(ctx, hipGetLastError());
    if (!n) return ZKLC_OK;
    const dim3 grid((unsigned)((n + GK_LANES - 1) / GK_LANES)), block(GK_LANES);
    const u32 compressed = flags & ZKLC_POINTS_COMPRESSED, subgroup = (flags & ZKLC_POINTS_CHECK_SUBGROUP) != 0;
    const g16_key &key = g16_key_constants();
    u32 *w = (u32 *)d_words;
    u64 *s = (u64 *)d_summary;
    if (!g2) {
        if (compressed) hipLaunchKernelGGL((gk_decode_kernel<0, 1>), grid, block, 0, st, key, d_bytes, (u64)n, w, d_status, s, 1u);
        else hipLaunchKernelGGL((gk_decode_kernel<0, 0>), grid, block, 0, st, key, d_bytes, (u64)n, w, d_status, s, 1u);
    } else {
        if (compressed) hipLaunchKernelGGL((gk_decode_kernel<1, 1>), grid, block, 0, st, key, d_bytes, (u64)n, w, d_status, s, !subgroup);
        else hipLaunchKernelGGL((gk_decode_kernel<1, 0>), grid, block, 0, st, key, d_bytes, (u64)n, w, d_status, s, !subgroup);
    }
    ZKLC_HIP(ctx, hipGetLastError());
    if (subgroup) {
        hipLaunchKernelGGL(gk_g2_subgroup_kernel, grid, block, 0, st, w, d_status, (u64)n, s);
        ZKLC_HIP(ctx, hipGetLastError());
    }
    return ZKLC_OK;
}

extern "C" int32_t zklc_bn254_g1_decode_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_bytes, uint64_t n, uint32_t flags,
                                            uint64_t *d_words, uint32_t *d_status, uint64_t *d_summary) {
    return gk_decode_dev(ctx, stream, d_bytes, n, flags, d_words, d_status, d_summary, false);
}
extern "C" int32_t zklc_bn254_g2_decode_dev(zklc_ctx *ctx, void *stream, const uint8_t *d_bytes, uint64_t n, uint32_t flags,
                                            uint64_t *d_words, uint32_t *d_status, uint64_t *d_summary) {
    return gk_decode_dev(ctx, stream, d_bytes, n, flags, d_words, d_status, d_summary, true);
}
