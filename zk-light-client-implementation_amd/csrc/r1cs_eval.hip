// A w, B w, C w of a resident constraint system on gfx950 + C ABI (r1cs_eval.cuh).  Per call, on one stream:
//   r1cs_witness_kernel        one lane per wire: the witness, regular form, into Montgomery form in the workspace (one multiplication)
//   r1cs_pad_kernel            rows n_constraints .. n - 1 of the three outputs: zero
//   r1cs_rows_kernel<1|8|64>   the rows of one length bin, 1 / 8 / 64 lanes per row.  A group strides over its row's terms (for 8 and
//                              64 lanes consecutive lanes read consecutive terms), every lane keeps a canonical partial sum, the group
//                              adds them by a butterfly of __shfl_xor (modular additions: exact, any order), its first lane stores
//                              32 bytes.  Rows come through the bin's list of row indices; the outputs stay in the caller's order.
//   r1cs_check_kernel          ZKLC_R1CS_CHECK: one lane per constraint, a b - c; ballots per wave, the waves of a workgroup meet
//                              through LDS, lane 0 adds with ordinary atomics (two per workgroup that has a violation) into the two
//                              words a one-lane kernel has set.
#include "r1cs_eval.cuh"
#include "zklc_internal.h"

#define R1CS_LANES 256u
#define R1CS_WAVES (R1CS_LANES / 64u)
#define R1CS_MAX_GRID 0x7fffffffull

__global__ void r1cs_summary_init_kernel(u64 *__restrict__ summary) {
    summary[0] = 0;
    summary[1] = ~0ull;
}

__global__ void __launch_bounds__(R1CS_LANES)
r1cs_witness_kernel(const u32 *__restrict__ regular, u64 n_wires, u32 *__restrict__ mont) {
    const u64 i = (u64)blockIdx.x * R1CS_LANES + threadIdx.x;
    if (i < n_wires) r1cs_store(mont + 8 * i, r1cs_witness_to_mont(regular + 8 * i));
}

// i < 3 pad: row n_constraints + i % pad of output i / pad
__global__ void __launch_bounds__(R1CS_LANES)
r1cs_pad_kernel(u64 nc, u64 pad, u32 *__restrict__ a, u32 *__restrict__ b, u32 *__restrict__ c) {
    const u64 i = (u64)blockIdx.x * R1CS_LANES + threadIdx.x;
    if (i >= 3 * pad) return;
    const u64 m = i / pad, j = nc + i % pad;
    r1cs_store((m == 0 ? a : m == 1 ? b : c) + 8 * j, r1cs_zero());
}

template <u32 G>
__global__ void __launch_bounds__(R1CS_LANES)
r1cs_rows_kernel(const u64 *__restrict__ terms, const u64 *__restrict__ row_ptr, const u32 *__restrict__ perm, u64 n_rows,
                 const u32 *__restrict__ coeffs, const u32 *__restrict__ witness, u64 nc, u32 *__restrict__ a, u32 *__restrict__ b,
                 u32 *__restrict__ c) {
    const u64 slot = ((u64)blockIdx.x * R1CS_LANES + threadIdx.x) / G;
    const u32 sub = threadIdx.x % G;
    const bool live = slot < n_rows;            // a group is live or not as a whole: G divides the workgroup
    u64 row = 0, begin = 0, end = 0;
    if (live) {
        row = perm[slot];
        begin = row_ptr[row];
        end = row_ptr[row + 1];
    }
    r1cs_el s = r1cs_row_sum(terms, begin, end, sub, G, witness, coeffs);
    // every lane of the wave takes part in the butterfly (a group that is not live adds zeros)
    for (u32 off = G >> 1; off; off >>= 1) {
        r1cs_el o;
        for (int i = 0; i < 8; i++) o.w[i] = (u32)__shfl_xor((int)s.w[i], (int)off, 64);
        s = r1cs_add(s, o);
    }
    if (live && sub == 0) {
        const u64 m = row / nc, j = row % nc;
        r1cs_store((m == 0 ? a : m == 1 ? b : c) + 8 * j, s);
    }
}

__global__ void __launch_bounds__(R1CS_LANES)
r1cs_check_kernel(const u32 *__restrict__ a, const u32 *__restrict__ b, const u32 *__restrict__ c, u64 nc, u64 *__restrict__ summary) {
    __shared__ u32 cnt[R1CS_WAVES];
    __shared__ u64 first[R1CS_WAVES];
    const u64 j = (u64)blockIdx.x * R1CS_LANES + threadIdx.x;
    const bool bad = j < nc && !r1cs_satisfied(a + 8 * j, b + 8 * j, c + 8 * j);
    const u64 ballot = __ballot(bad);
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) {
        cnt[wave] = (u32)__popcll(ballot);
        first[wave] = ballot ? j + (u64)(__ffsll((unsigned long long)ballot) - 1) : ~0ull;   // j: this wave's first constraint
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    u64 n_bad = 0, f = ~0ull;
    for (u32 w = 0; w < R1CS_WAVES; w++) {
        n_bad += cnt[w];
        f = first[w] < f ? first[w] : f;
    }
    if (n_bad) {
        atomicAdd((unsigned long long *)summary, (unsigned long long)n_bad);
        atomicMin((unsigned long long *)summary + 1, (unsigned long long)f);
    }
}

static void r1cs_free_device(zklc_r1cs *s) {
    if (s->device < 0) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(s->device);
    for (void *p : {s->d_row_ptr, s->d_terms, s->d_coeffs, s->d_perm})
        if (p) (void)hipFree(p);
    s->d_row_ptr = s->d_terms = s->d_coeffs = s->d_perm = nullptr;
    s->device = -1;
    if (prev >= 0) (void)hipSetDevice(prev);
    (void)hipGetLastError();
}

static int32_t r1cs_upload(zklc_ctx *ctx, zklc_r1cs *s) {
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    s->device = ctx->device;
    struct {
        void **d;
        const void *h;
        size_t bytes;
    } parts[4] = {{&s->d_row_ptr, s->row_ptr.data(), s->row_ptr.size() * 8},
                  {&s->d_terms, s->terms.data(), s->terms.size() * 8},
                  {&s->d_coeffs, s->coeffs.data(), s->coeffs.size() * 4},
                  {&s->d_perm, s->perm.data(), s->perm.size() * 4}};
    for (auto &p : parts) {
        ZKLC_HIP(ctx, hipMalloc(p.d, p.bytes ? p.bytes : 16));      // never a null device pointer in a kernel's arguments
        if (p.bytes) ZKLC_HIP(ctx, hipMemcpy(*p.d, p.h, p.bytes, hipMemcpyHostToDevice));
    }
    return ZKLC_OK;
}

extern "C" int32_t zklc_r1cs_create(zklc_ctx *ctx, uint64_t n_constraints, uint64_t n_wires, const uint64_t *row_ptr,
                                    const uint32_t *term_wire, const uint32_t *term_coeff, uint64_t nnz, const uint64_t *coeffs,
                                    uint32_t n_coeff, zklc_r1cs **out) {
    int32_t rc = r1cs_build_host(n_constraints, n_wires, row_ptr, term_wire, term_coeff, nnz, coeffs, n_coeff, out);
    if (rc != ZKLC_OK || !ctx) return rc;
    rc = r1cs_upload(ctx, *out);
    if (rc != ZKLC_OK) {
        zklc_r1cs_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

extern "C" void zklc_r1cs_destroy(zklc_r1cs *s) {
    if (!s) return;
    r1cs_free_device(s);
    r1cs_free_host(s);
}

extern "C" int32_t zklc_r1cs_abc_dev(zklc_ctx *ctx, void *stream, const zklc_r1cs *s, const uint64_t *d_witness_regular, uint64_t n,
                                     uint64_t *d_a, uint64_t *d_b, uint64_t *d_c, uint32_t flags, uint64_t *d_summary,
                                     void *d_workspace, uint64_t workspace_bytes) {
    if (!ctx || !s || s->device != ctx->device || (flags & ~ZKLC_R1CS_CHECK)) return ZKLC_ERR_INVALID_ARG;
    if (n < s->n_constraints || n > R1CS_MAX_CONSTRAINTS) return ZKLC_ERR_INVALID_ARG;
    if (!d_witness_regular || !d_workspace || (n && (!d_a || !d_b || !d_c)) || ((flags & ZKLC_R1CS_CHECK) && !d_summary))
        return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)d_witness_regular | (uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_c | (uintptr_t)d_workspace) & 15 ||
        (uintptr_t)d_summary & 7)
        return ZKLC_ERR_INVALID_ARG;
    if (workspace_bytes < zklc_r1cs_workspace_bytes(s)) return ZKLC_ERR_INVALID_ARG;
    const u64 nc = s->n_constraints, pad = n - nc;
    auto blocks = [](u64 lanes) { return (lanes + R1CS_LANES - 1) / R1CS_LANES; };
    if (blocks(s->n_wires) > R1CS_MAX_GRID || blocks(3 * pad) > R1CS_MAX_GRID || blocks(s->bin_rows[0]) > R1CS_MAX_GRID ||
        blocks(s->bin_rows[1] * 8) > R1CS_MAX_GRID || blocks(s->bin_rows[2] * 64) > R1CS_MAX_GRID)
        return ZKLC_ERR_INVALID_ARG;
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = zklc_pick_stream(ctx, stream);
    const dim3 block(R1CS_LANES);
    u32 *a = (u32 *)d_a, *b = (u32 *)d_b, *c = (u32 *)d_c, *wm = (u32 *)d_workspace;
    if (flags & ZKLC_R1CS_CHECK) hipLaunchKernelGGL(r1cs_summary_init_kernel, dim3(1), dim3(1), 0, st, (u64 *)d_summary);
    hipLaunchKernelGGL(r1cs_witness_kernel, dim3((unsigned)blocks(s->n_wires)), block, 0, st, (const u32 *)d_witness_regular,
                       (u64)s->n_wires, wm);
    if (pad) hipLaunchKernelGGL(r1cs_pad_kernel, dim3((unsigned)blocks(3 * pad)), block, 0, st, nc, pad, a, b, c);
    const u64 *terms = (const u64 *)s->d_terms, *row_ptr = (const u64 *)s->d_row_ptr;
    const u32 *perm = (const u32 *)s->d_perm, *coeffs = (const u32 *)s->d_coeffs;
    const u64 r0 = s->bin_rows[0], r1 = s->bin_rows[1], r2 = s->bin_rows[2];
    if (r0) hipLaunchKernelGGL((r1cs_rows_kernel<1>), dim3((unsigned)blocks(r0)), block, 0, st, terms, row_ptr, perm, r0, coeffs,
                               (const u32 *)wm, nc, a, b, c);
    if (r1) hipLaunchKernelGGL((r1cs_rows_kernel<8>), dim3((unsigned)blocks(r1 * 8)), block, 0, st, terms, row_ptr, perm + r0, r1,
                               coeffs, (const u32 *)wm, nc, a, b, c);
    if (r2) hipLaunchKernelGGL((r1cs_rows_kernel<64>), dim3((unsigned)blocks(r2 * 64)), block, 0, st, terms, row_ptr, perm + r0 + r1,
                               r2, coeffs, (const u32 *)wm, nc, a, b, c);
    if ((flags & ZKLC_R1CS_CHECK) && nc)
        hipLaunchKernelGGL(r1cs_check_kernel, dim3((unsigned)blocks(nc)), block, 0, st, (const u32 *)a, (const u32 *)b, (const u32 *)c,
                           nc, (u64 *)d_summary);
    ZKLC_HIP(ctx, hipGetLastError());
    return ZKLC_OK;
}
