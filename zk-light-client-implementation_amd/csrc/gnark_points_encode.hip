// Batched encoding of gnark point arrays on gfx950 + C ABI (gnark_points_encode.cuh): one lane per point over the words of a key
// in HBM, the bytes of a key file's point array out.
//   gk_encode_kernel<G2, COMPRESSED>   four instances.  16 / 32 words in by 16-byte loads, two / four multiplications out of the
//                                      Montgomery domain, bytes swapped in registers, 64 / 128 bytes (raw) or 32 / 64 (compressed)
//                                      out by 16-byte stores -- a memory stream; the curve equation only when the caller validates
//                                      (a run-time argument, uniform over the grid).
// Summary (OK, infinity, rejected, first rejected index): gnark_points_summary.cuh, the decoder's own.
#include "gnark_points_encode.cuh"
#include "gnark_points_summary.cuh"
#include "groth16_verifier_host.h"
#include "zklc_internal.h"

template <u32 G2, u32 COMPRESSED>
__global__ void __launch_bounds__(GK_LANES)
gk_encode_kernel(const g16_key key, const u32 *__restrict__ words, u64 n, u32 validate, uint8_t *__restrict__ bytes,
                 u32 *__restrict__ status, u64 *__restrict__ summary) {
    constexpr u32 STRIDE = (G2 ? 128u : 64u) >> COMPRESSED, QUADS = G2 ? 8u : 4u;
    const u64 i = (u64)blockIdx.x * GK_LANES + threadIdx.x;
    const u32 live = i < n;
    u32 st = GK_INFINITY;
    if (live) {
        u32 w[4 * QUADS];
        gk_load_words(w, words + i * (4 * QUADS), QUADS);
        if (G2) st = gk_g2_encode<COMPRESSED>(key, w, validate, bytes + i * STRIDE);
        else st = gk_g1_encode<COMPRESSED>(w, validate, bytes + i * STRIDE);
        status[i] = st;
    }
    gk_count(st, live, i, summary);
}

static int32_t gk_encode_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_words, uint64_t n, uint32_t flags, uint8_t *d_bytes,
                             uint32_t *d_status, uint64_t *d_summary, bool g2) {
    if (!ctx || !d_summary || (flags & ~(ZKLC_POINTS_COMPRESSED | ZKLC_POINTS_VALIDATE))) return ZKLC_ERR_INVALID_ARG;
    if (n > GK_MAX_POINTS || (n && (!d_bytes || !d_words || !d_status))) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)d_bytes | (uintptr_t)d_words) & 15 || (uintptr_t)d_status & 3 || (uintptr_t)d_summary & 7) return ZKLC_ERR_INVALID_ARG;
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = zklc_pick_stream(ctx, stream);
    hipLaunchKernelGGL(gk_summary_init_kernel, dim3(1), dim3(1), 0, st, (u64 *)d_summary);
    ZKLC_HIP(ctx, hipGetLastError());
    if (!n) return ZKLC_OK;
    const dim3 grid((unsigned)((n + GK_LANES - 1) / GK_LANES)), block(GK_LANES);
    const u32 compressed = flags & ZKLC_POINTS_COMPRESSED, validate = (flags & ZKLC_POINTS_VALIDATE) != 0;
    const g16_key &key = g16_key_constants();
    const u32 *w = (const u32 *)d_words;
    u64 *s = (u64 *)d_summary;
    if (!g2) {
        if (compressed) hipLaunchKernelGGL((gk_encode_kernel<0, 1>), grid, block, 0, st, key, w, (u64)n, validate, d_bytes, d_status, s);
        else hipLaunchKernelGGL((gk_encode_kernel<0, 0>), grid, block, 0, st, key, w, (u64)n, validate, d_bytes, d_status, s);
    } else {
        if (compressed) hipLaunchKernelGGL((gk_encode_kernel<1, 1>), grid, block, 0, st, key, w, (u64)n, validate, d_bytes, d_status, s);
        else hipLaunchKernelGGL((gk_encode_kernel<1, 0>), grid, block, 0, st, key, w, (u64)n, validate, d_bytes, d_status, s);
    }
    ZKLC_HIP(ctx, hipGetLastError());
    return ZKLC_OK;
}

extern "C" int32_t zklc_bn254_g1_encode_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_words, uint64_t n, uint32_t flags,
                                            uint8_t *d_bytes, uint32_t *d_status, uint64_t *d_summary) {
    return gk_encode_dev(ctx, stream, d_words, n, flags, d_bytes, d_status, d_summary, false);
}
extern "C" int32_t zklc_bn254_g2_encode_dev(zklc_ctx *ctx, void *stream, const uint64_t *d_words, uint64_t n, uint32_t flags,
                                            uint8_t *d_bytes, uint32_t *d_status, uint64_t *d_summary) {
    return gk_encode_dev(ctx, stream, d_words, n, flags, d_bytes, d_status, d_summary, true);
}
