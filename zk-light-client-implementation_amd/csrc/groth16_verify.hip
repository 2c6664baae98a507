// Batched Groth16 verification on gfx950 + C ABI (groth16_verify.cuh): one kernel decodes and validates the proofs' points and
// folds the public inputs into kSum, leaving the g1 / g2 arrays of the pairing-product kernels of bn254_pairing.hip, which give the
// verdict.  One upload (proofs + inputs), two launches, one settled read-back (statuses + pairing verdicts).
#include "groth16_verifier_host.h"
#include "zklc_internal.h"
#include <chrono>
#include <string.h>

// One 128-lane workgroup per proof.  Wave 0: lane j folds the inputs j, j + 64, ... over the key's table; the partial sums meet
// through LDS (40 words per lane) and lane 0 leaves kSum.  Wave 1, lane 64: decoding, curve and subgroup tests of A, B, C.
// g1 per proof: A, C, kSum, alpha (8 u64 each); g2: B, -delta, -gamma, -beta (16 u64 each).  A rejected proof gets all-zero G1
// points: the pairing kernel skips those pairs, and the host ignores its verdict.
__global__ void __launch_bounds__(128)
g16_prepare_kernel(const g16_key *__restrict__ key, const g16_tab_entry *__restrict__ tab, const uint8_t *__restrict__ k_inf,
                   const uint8_t *__restrict__ proofs, const u64 *__restrict__ inputs, u32 compressed, u32 *__restrict__ status,
                   u64 *__restrict__ g1, u64 *__restrict__ g2) {
    __shared__ i32 lds[G16_FOLD_LANES * 40];
    __shared__ u32 st_sh;
    const u32 b = blockIdx.x, t = threadIdx.x;
    const u32 np = key->n_public;
    u32 *o1 = reinterpret_cast<u32 *>(g1 + (size_t)b * 32), *o2 = reinterpret_cast<u32 *>(g2 + (size_t)b * 64);
    g16_g1 acc = ec_infinity<FpField>();
    if (t < G16_FOLD_LANES) {
        acc = g16_fold_lane(tab, k_inf, inputs + (size_t)b * np * 4, np, t, G16_FOLD_LANES);
    } else if (t == G16_FOLD_LANES) {
        u32 wa[16], wc[16], wb[32];
        const u32 st = g16_validate_lane(*key, proofs + (size_t)b * (compressed ? 128 : 256), compressed, wa, wc, wb);
        for (int i = 0; i < 16; i++) {
            o1[i] = wa[i];
            o1[16 + i] = wc[i];
        }
        for (int i = 0; i < 32; i++) o2[i] = wb[i];
        st_sh = st;
        status[b] = st;
    }
    u32 width = 1;
    while (width < np && width < G16_FOLD_LANES) width <<= 1;
    for (u32 stride = width >> 1; stride >= 1; stride >>= 1) {
        if (t >= stride && t < 2 * stride) {
            i32 *d = lds + (t - stride) * 40;
            FpField::store(d, acc.X);
            FpField::store(d + 10, acc.Y);
            FpField::store(d + 20, acc.ZZ);
            FpField::store(d + 30, acc.ZZZ);
        }
        __syncthreads();
        if (t < stride) {
            const i32 *s = lds + t * 40;
            g16_g1 o;
            o.X = FpField::load(s);
            o.Y = FpField::load(s + 10);
            o.ZZ = FpField::load(s + 20);
            o.ZZZ = FpField::load(s + 30);
            acc = ec_add<FpField>(acc, o);
        }
        __syncthreads();
    }
    __syncthreads();                       // st_sh (also when the loop above ran no round)
    if (t != 0) return;
    u32 wk[16];
    if (st_sh == G16_OK) g16_fold_finish(*key, acc, wk);
    else
        for (int i = 0; i < 16; i++) wk[i] = 0;
    for (int i = 0; i < 16; i++) {
        o1[32 + i] = wk[i];
        o1[48 + i] = st_sh == G16_OK ? key->alpha[i] : 0u;
    }
    for (int i = 0; i < 96; i++) o2[32 + i] = key->neg_g2[i / 32][i % 32];
}

static int32_t g16_grow(zklc_ctx *ctx, void **buf, size_t *cap, size_t bytes) {
    if (*cap >= bytes) return ZKLC_OK;
    if (*buf) ZKLC_HIP(ctx, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    ZKLC_HIP(ctx, hipMalloc(buf, bytes));
    *cap = bytes;
    return ZKLC_OK;
}
static int32_t g16_grow_pinned(zklc_ctx *ctx, void **buf, size_t *cap, size_t bytes) {
    if (*cap >= bytes) return ZKLC_OK;
    if (*buf) ZKLC_HIP(ctx, hipHostFree(*buf));
    *buf = nullptr;
    *cap = 0;
    ZKLC_HIP(ctx, hipHostMalloc(buf, bytes, hipHostMallocDefault));
    *cap = bytes;
    return ZKLC_OK;
}
static double g16_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

extern "C" int32_t zklc_groth16_verify_batch(zklc_ctx *ctx, zklc_groth16_verifier *v, const uint8_t *proofs, const uint64_t *public_inputs,
                                             uint64_t n, uint32_t flags, int32_t *status_out) {
    if (!ctx || !v || (flags & ~ZKLC_G16_COMPRESSED)) return ZKLC_ERR_INVALID_ARG;
    if (v->device >= 0 && v->device != ctx->device) return ZKLC_ERR_INVALID_ARG;   // the buffers live on the first call's GPU
    if (!n) return ZKLC_OK;
    const uint32_t np = v->key.n_public, compressed = flags & ZKLC_G16_COMPRESSED;
    if (!proofs || !status_out || (np && !public_inputs) || n > G16_MAX_BATCH) return ZKLC_ERR_INVALID_ARG;
    const double t0 = g16_now_ms();
    // sizes: n <= 2^24 and n_public <= 4096 bound every product below 2^45; checked all the same
    uint64_t proof_bytes, input_bytes, g1_bytes, g2_bytes, out_bytes;
    if (!g16_mul_ok(n, compressed ? 128 : 256, &proof_bytes) || !g16_mul_ok(n, (uint64_t)np * 32, &input_bytes) ||
        !g16_mul_ok(n, 4 * 64, &g1_bytes) || !g16_mul_ok(n, 4 * 128, &g2_bytes) || !g16_mul_ok(n, 8, &out_bytes) ||
        proof_bytes + input_bytes < proof_bytes)
        return ZKLC_ERR_INVALID_ARG;
    const size_t in_bytes = (size_t)(proof_bytes + input_bytes);
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    v->device = ctx->device;
    hipStream_t st = ctx->stream;
    int32_t rc;
    if (!v->d_key) {                        // the key, its table and the infinity flags: once per verifier
        size_t c = 0;
        if ((rc = g16_grow(ctx, &v->d_key, &c, sizeof(g16_key)))) return rc;
        c = 0;
        if ((rc = g16_grow(ctx, &v->d_tab, &c, v->tab.size() * sizeof(g16_tab_entry) + 16))) return rc;
        c = 0;
        if ((rc = g16_grow(ctx, &v->d_kinf, &c, v->k_inf.size()))) return rc;
        ZKLC_HIP(ctx, hipMemcpyAsync(v->d_key, &v->key, sizeof(g16_key), hipMemcpyHostToDevice, st));
        if (!v->tab.empty())
            ZKLC_HIP(ctx, hipMemcpyAsync(v->d_tab, v->tab.data(), v->tab.size() * sizeof(g16_tab_entry), hipMemcpyHostToDevice, st));
        ZKLC_HIP(ctx, hipMemcpyAsync(v->d_kinf, v->k_inf.data(), v->k_inf.size(), hipMemcpyHostToDevice, st));
        ZKLC_HIP(ctx, zklc_stream_wait(st));   // the sources are pageable host memory of the verifier
    }
    if ((rc = g16_grow(ctx, &v->d_in, &v->cap_in, in_bytes)) || (rc = g16_grow(ctx, &v->d_g1, &v->cap_g1, (size_t)g1_bytes)) ||
        (rc = g16_grow(ctx, &v->d_g2, &v->cap_g2, (size_t)g2_bytes)) || (rc = g16_grow(ctx, &v->d_out, &v->cap_out, (size_t)out_bytes)) ||
        (rc = g16_grow_pinned(ctx, &v->h_in, &v->cap_h_in, in_bytes)) || (rc = g16_grow_pinned(ctx, &v->h_out, &v->cap_h_out, (size_t)out_bytes)))
        return rc;
    hipEvent_t *ev = (hipEvent_t *)v->events;
    for (int k = 0; k < 4; k++)
        if (!ev[k]) ZKLC_HIP(ctx, hipEventCreate(&ev[k]));
    // 1. one upload: inputs first (8-byte aligned), then the proof bytes
    if (input_bytes) memcpy(v->h_in, public_inputs, (size_t)input_bytes);
    memcpy((uint8_t *)v->h_in + input_bytes, proofs, (size_t)proof_bytes);
    ZKLC_HIP(ctx, hipEventRecord(ev[0], st));
    ZKLC_HIP(ctx, hipMemcpyAsync(v->d_in, v->h_in, in_bytes, hipMemcpyHostToDevice, st));
    ZKLC_HIP(ctx, hipEventRecord(ev[1], st));
    // 2. validation + kSum, then the pairing product over what it left
    u32 *d_status = (u32 *)v->d_out, *d_is_one = d_status + n;
    hipLaunchKernelGGL(g16_prepare_kernel, dim3((unsigned)n), dim3(128), 0, st, (const g16_key *)v->d_key, (const g16_tab_entry *)v->d_tab,
                       (const uint8_t *)v->d_kinf, (const uint8_t *)v->d_in + input_bytes, (const u64 *)v->d_in, compressed, d_status,
                       (u64 *)v->d_g1, (u64 *)v->d_g2);
    ZKLC_HIP(ctx, hipGetLastError());
    ZKLC_HIP(ctx, hipEventRecord(ev[2], st));
    if ((rc = zklc_bn254_pairing_check_dev(ctx, st, (const uint64_t *)v->d_g1, (const uint64_t *)v->d_g2, 4, (uint32_t)n, d_is_one, nullptr)))
        return rc;
    ZKLC_HIP(ctx, hipEventRecord(ev[3], st));
    // 3. one read-back after the stream has settled
    ZKLC_HIP(ctx, zklc_readback_async(v->h_out, v->d_out, (size_t)out_bytes, st));
    ZKLC_HIP(ctx, zklc_stream_wait(st));
    const u32 *h_status = (const u32 *)v->h_out, *h_is_one = h_status + n;
    for (uint64_t i = 0; i < n; i++)
        status_out[i] = h_status[i] ? (int32_t)h_status[i] : (h_is_one[i] ? ZKLC_G16_OK : ZKLC_G16_PAIRING);
    float up = 0, ka = 0, kb = 0;
    (void)hipEventElapsedTime(&up, ev[0], ev[1]);
    (void)hipEventElapsedTime(&ka, ev[1], ev[2]);
    (void)hipEventElapsedTime(&kb, ev[2], ev[3]);
    v->last_ms[0] = up;
    v->last_ms[1] = ka;
    v->last_ms[2] = kb;
    v->last_ms[3] = g16_now_ms() - t0;
    return ZKLC_OK;
}

extern "C" uint32_t zklc_groth16_verifier_last_timings(const zklc_groth16_verifier *v, double *out_ms, uint32_t cap) {
    if (!v || !out_ms) return 0;
    uint32_t k = cap < 4 ? cap : 4;
    for (uint32_t i = 0; i < k; i++) out_ms[i] = v->last_ms[i];
    return k;
}

extern "C" void zklc_groth16_verifier_destroy(zklc_groth16_verifier *v) {
    if (!v) return;
    if (v->device >= 0 && hipSetDevice(v->device) == hipSuccess) {
        for (void *p : {v->d_key, v->d_tab, v->d_kinf, v->d_in, v->d_g1, v->d_g2, v->d_out})
            if (p) (void)hipFree(p);
        for (void *e : v->events)
            if (e) (void)hipEventDestroy((hipEvent_t)e);
    }
    if (v->h_in) (void)hipHostFree(v->h_in);
    if (v->h_out) (void)hipHostFree(v->h_out);
    delete v;
}
