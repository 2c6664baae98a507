// Batched fixed-base scalar multiplication on gfx950 + C ABI (bn254_fixed_mul.cuh).  Per call, on one stream:
//   fbm_summary_init_kernel      one lane: (0, all-ones)
//   fbm_mul_kernel<F>            stage A, one lane per scalar: a table gather and a mixed addition per non-zero digit, X, Y, ZZ, ZZZ
//                                into the workspace.  256 lanes per workgroup = one wave per SIMD: the G2 accumulator (80 limbs) and
//                                a table entry (40) with the temporaries of a mixed addition do not fit the 256 registers of two.
//   fbm_affine_kernel<F, Emit>   stage B, one lane per inversion group: gnark's words out; a lane that met points at infinity adds to
//                                the summary with ordinary atomics (zero scalars are the exception).
// A table is built once by fbm_table_kernel<F> (stage A') and the same stage B with the packing emitter.
#include "bn254_fixed_mul.cuh"
#include "zklc_internal.h"

#define FBM_LANES 256u

__global__ void fbm_summary_init_kernel(u64 *__restrict__ summary) {
    summary[0] = 0;
    summary[1] = ~0ull;
}

template <class F>
__global__ void __launch_bounds__(FBM_LANES)
fbm_mul_kernel(const i32 *__restrict__ table, u32 c, const u64 *__restrict__ scalars, u64 n, i32 *__restrict__ ws) {
    const u64 i = (u64)blockIdx.x * FBM_LANES + threadIdx.x;
    if (i < n) fbm_mul_lane<F>(table, c, scalars, i, ws, n);
}

template <class F>
__global__ void __launch_bounds__(FBM_LANES)
fbm_table_kernel(const u32 *__restrict__ row_bases, u32 c, u64 lanes, i32 *__restrict__ ws, u64 total) {
    const u64 t = (u64)blockIdx.x * FBM_LANES + threadIdx.x;
    if (t < lanes) fbm_table_lane<F>(row_bases, c, t, ws, total);
}

template <class F, class Emit>
__global__ void __launch_bounds__(FBM_LANES)
fbm_affine_kernel(i32 *__restrict__ ws, u64 n, Emit emit, u64 *__restrict__ summary) {
    const u64 g = (u64)blockIdx.x * FBM_LANES + threadIdx.x;
    if (g >= fbm_groups(n)) return;
    u64 first;
    const u32 n_inf = fbm_affine_group<F>(ws, n, g, emit, first);
    if (n_inf && summary) {
        atomicAdd((unsigned long long *)summary, (unsigned long long)n_inf);
        atomicMin((unsigned long long *)summary + 1, (unsigned long long)first);
    }
}

static unsigned fbm_blocks(u64 lanes) { return (unsigned)((lanes + FBM_LANES - 1) / FBM_LANES); }

template <class F>
static int32_t fbm_build_device(zklc_ctx *ctx, const std::vector<u32> &row_bases, zklc_fixed_base *t) {
    const u32 c = t->c, cpr = (t->entries + FBM_CHUNK - 1) / FBM_CHUNK;
    const u64 total = (u64)t->rows * t->entries, lanes = (u64)t->rows * cpr;
    void *d_ws = nullptr, *d_bases = nullptr;
    ZKLC_HIP(ctx, hipMalloc(&t->d_table, total * 2 * F::PACKW * 4));
    auto release = [&] {
        if (d_ws) (void)hipFree(d_ws);
        if (d_bases) (void)hipFree(d_bases);
    };
    hipError_t e = hipMalloc(&d_ws, (size_t)FBM_SLOTS * F::LIMBS * 4 * total);
    if (e == hipSuccess) e = hipMalloc(&d_bases, row_bases.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_bases, row_bases.data(), row_bases.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((fbm_table_kernel<F>), dim3(fbm_blocks(lanes)), dim3(FBM_LANES), 0, ctx->stream, (const u32 *)d_bases, c, lanes,
                           (i32 *)d_ws, total);
        const fbm_emit_packed<F> emit = {(u32 *)t->d_table};
        hipLaunchKernelGGL((fbm_affine_kernel<F, fbm_emit_packed<F>>), dim3(fbm_blocks(fbm_groups(total))), dim3(FBM_LANES), 0, ctx->stream,
                           (i32 *)d_ws, total, emit, (u64 *)nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = zklc_stream_wait(ctx->stream);
    release();
    ZKLC_HIP(ctx, e);
    return ZKLC_OK;
}

extern "C" void zklc_bn254_fixed_base_destroy(zklc_fixed_base *t) {
    if (!t) return;
    if (t->device >= 0 && t->d_table) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(t->device);
        (void)hipFree(t->d_table);
        if (prev >= 0) (void)hipSetDevice(prev);
        (void)hipGetLastError();
    }
    delete t;
}

extern "C" int32_t zklc_bn254_fixed_base_create(zklc_ctx *ctx, uint32_t group, const uint64_t *base_words, uint32_t window_bits,
                                                zklc_fixed_base **out) {
    if (!ctx) return fbm_build_host(group, base_words, window_bits, out);
    if (!out) return ZKLC_ERR_INVALID_ARG;
    *out = nullptr;
    std::vector<u32> row_bases;
    int32_t rc = fbm_row_bases_host(group, base_words, window_bits, row_bases);
    if (rc != ZKLC_OK) return rc;
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    zklc_fixed_base *t = new (std::nothrow) zklc_fixed_base;
    if (!t) return ZKLC_ERR_OOM;
    t->group = group;
    t->c = window_bits;
    t->rows = fbm_rows(window_bits);
    t->entries = fbm_entries(window_bits);
    t->device = ctx->device;
    rc = group == ZKLC_GROUP_G2 ? fbm_build_device<Fp2Field>(ctx, row_bases, t) : fbm_build_device<FpField>(ctx, row_bases, t);
    if (rc != ZKLC_OK) {
        zklc_bn254_fixed_base_destroy(t);
        return rc;
    }
    *out = t;
    return ZKLC_OK;
}

template <class F>
static void fbm_launch(hipStream_t st, const zklc_fixed_base *t, const u64 *scalars, u64 n, u32 *words, u64 *summary, i32 *ws) {
    hipLaunchKernelGGL((fbm_mul_kernel<F>), dim3(fbm_blocks(n)), dim3(FBM_LANES), 0, st, (const i32 *)t->d_table, t->c, scalars, n, ws);
    const fbm_emit_gnark<F> emit = {words};
    hipLaunchKernelGGL((fbm_affine_kernel<F, fbm_emit_gnark<F>>), dim3(fbm_blocks(fbm_groups(n))), dim3(FBM_LANES), 0, st, ws, n, emit,
                       summary);
}

static int32_t fbm_mul_dev(zklc_ctx *ctx, void *stream, const zklc_fixed_base *t, u32 group, const uint64_t *d_scalars, uint64_t n,
                           uint64_t *d_words, uint64_t *d_summary, void *d_ws, uint64_t ws_bytes) {
    if (!ctx || !t || t->group != group || t->device != ctx->device || !t->d_table || !d_summary) return ZKLC_ERR_INVALID_ARG;
    if (n > FBM_MAX_POINTS || (n && (!d_scalars || !d_words || !d_ws))) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)d_scalars | (uintptr_t)d_words | (uintptr_t)d_ws) & 15 || (uintptr_t)d_summary & 7) return ZKLC_ERR_INVALID_ARG;
    if (n && ws_bytes < zklc_bn254_fixed_mul_workspace_bytes(group, n)) return ZKLC_ERR_INVALID_ARG;
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = zklc_pick_stream(ctx, stream);
    hipLaunchKernelGGL(fbm_summary_init_kernel, dim3(1), dim3(1), 0, st, (u64 *)d_summary);
    if (n) {
        if (group == ZKLC_GROUP_G2) fbm_launch<Fp2Field>(st, t, (const u64 *)d_scalars, n, (u32 *)d_words, (u64 *)d_summary, (i32 *)d_ws);
        else fbm_launch<FpField>(st, t, (const u64 *)d_scalars, n, (u32 *)d_words, (u64 *)d_summary, (i32 *)d_ws);
    }
    ZKLC_HIP(ctx, hipGetLastError());
    return ZKLC_OK;
}

extern "C" int32_t zklc_bn254_g1_fixed_mul_dev(zklc_ctx *ctx, void *stream, const zklc_fixed_base *tbl, const uint64_t *d_scalars_regular,
                                               uint64_t n, uint64_t *d_words, uint64_t *d_summary, void *d_workspace, uint64_t workspace_bytes) {
    return fbm_mul_dev(ctx, stream, tbl, ZKLC_GROUP_G1, d_scalars_regular, n, d_words, d_summary, d_workspace, workspace_bytes);
}
extern "C" int32_t zklc_bn254_g2_fixed_mul_dev(zklc_ctx *ctx, void *stream, const zklc_fixed_base *tbl, const uint64_t *d_scalars_regular,
                                               uint64_t n, uint64_t *d_words, uint64_t *d_summary, void *d_workspace, uint64_t workspace_bytes) {
    return fbm_mul_dev(ctx, stream, tbl, ZKLC_GROUP_G2, d_scalars_regular, n, d_words, d_summary, d_workspace, workspace_bytes);
}
