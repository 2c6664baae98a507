// plonky2 verifier, device part: the FRI query phase of a batch of proofs on the GPU (the once-per-proof work -- parse, transcript,
// vanishing identity, reduced openings -- stays on the host: csrc/plonky2_verifier_host.cpp).
//   kernel A (p2v_merkle_kernel)  one lane per (tree, proof, query round), tree-major and every tree's segment padded to whole
//                                 waves: the lanes of a wave hash leaves of one width, walk paths of one length, with one hasher
//   kernel B (p2v_fri_kernel)     one lane per (proof, query round): initial combination, fold chain, final polynomial
// Both read leaves, siblings and evaluations straight from the batch's proof bytes in HBM; one byte of result per lane.
// The Poseidon-Goldilocks permutation is the plain C++ form of poseidon_gl.cuh (no inline assembly in this unit).
#define ZKLC_PGL_NO_ASM 1
#include <chrono>
#include <vector>
#include "zklc_internal.h"
#include "plonky2_verifier_host.h"

#define P2V_WAVE 64

// Goldilocks openings, one lane per item (the Poseidon-BN254 ones: p2v_merkle_bn254_coop_kernel)
template <u32 HASHER>
__global__ void __launch_bounds__(P2V_WAVE) p2v_merkle_kernel(p2v_layout L, const uint8_t *__restrict__ proofs,
                                                              const uint8_t *__restrict__ cap0, const u32 *__restrict__ x_index,
                                                              u64 items, u64 seg, uint8_t *__restrict__ out) {
    const u64 gid = (u64)blockIdx.x * P2V_WAVE + threadIdx.x;
    const u32 t = (u32)(gid / seg);
    const u64 j = gid - (u64)t * seg;     // (proof, round) of this lane
    if (t >= L.num_trees || j >= items) return;
    const u64 p = j / L.rounds;
    const u32 r = (u32)(j - p * L.rounds);
    out[(u64)t * items + j] = p2v_merkle_lane<HASHER>(L, proofs + p * L.bytes, cap0, r, t, x_index[j]) ? 1 : 0;
}

// Poseidon-BN254 openings on FOUR lanes per item (poseidon_bn254_permute_coop, as the small Merkle levels of the prover): the
// one-lane permutation does not fit in the register file (256 VGPRs + 336 bytes of scratch in every one-lane kernel of
// poseidon_bn254.hip).  Lane q of a quad holds state word q.  Leaf: lanes 1..3 absorb three elements each per permutation
// (hash_no_pad, rate 3 Fr); path level: lanes 2 / 3 take (digest, sibling) in the order of the index bit (two_to_one = permute
// [0, 0, l, r]).  The running digest is state word 0, broadcast to the quad after every permutation.  Same result as
// p2v_merkle_lane<1> (the host path), which the tests compare on every BN128 batch.
__global__ void __launch_bounds__(P2V_WAVE) p2v_merkle_bn254_coop_kernel(p2v_layout L, const uint8_t *__restrict__ proofs,
                                                                         const uint8_t *__restrict__ cap0,
                                                                         const u32 *__restrict__ x_index, u64 items, u64 seg,
                                                                         uint8_t *__restrict__ out) {
    const u64 gid = (u64)blockIdx.x * P2V_WAVE + threadIdx.x;
    const u64 item = gid >> 2;
    const u32 q = (u32)(gid & 3);
    const u32 t = (u32)(item / seg);
    u64 j = item - (u64)t * seg;
    if (t >= L.num_trees) return;        // whole waves: seg is a multiple of 16 items
    const bool live = j < items;
    if (!live) j = items - 1;            // the quad broadcast needs all four lanes: idle quads redo the last item, without storing
    const u64 p = j / L.rounds;
    const u32 r = (u32)(j - p * L.rounds);
    const uint8_t *proof = proofs + p * L.bytes;
    const uint8_t *leaf = proof + L.rounds_off + (u64)r * L.round_bytes + L.tree_off[t];
    const u32 len = L.leaf_words[t], depth = L.depth[t];
    const uint8_t *sib = leaf + 8 * (size_t)len + 1;
    u32 index = x_index[j];
    const uint8_t *cap;
    if (t == 0) {
        cap = cap0;
    } else if (t < 4) {
        cap = proof + L.cap_off[t - 1];
    } else {
        cap = proof + L.commit_cap_off[t - 4];
        for (u32 i = 0; i <= t - 4; i++) index >>= L.arity_bits[i];
    }
    fr v[4];
    fr h = p2v_bn_pack3(leaf, len < 3 ? len : 3);     // hash_or_noop of <= 3 elements: the elements themselves
    if (len > 3) {
        fr s = fr_zero();
#pragma unroll 1
        for (u32 off = 0; off < len; off += 9) {
            const u32 o = off + 3 * (q - 1);
            if (q != 0 && o < len) s = p2v_bn_pack3(leaf + 8 * (size_t)o, len - o < 3 ? len - o : 3);
            poseidon_bn254_permute_coop(s, q);
        }
        pbn_quad_gather(v, s);
        h = v[0];
    }
#pragma unroll 1
    for (u32 d = 0; d < depth; d++) {
        fr s = fr_zero();
        if (q >= 2) {
            u32 w[8];
            for (int i = 0; i < 8; i++) w[i] = p2v_ld32(sib + 32 * (size_t)d + 4 * i);
            const fr sb = fr_from_regular(w);
            s = (q == 2) == (bool)(index & 1) ? sb : h;     // lane 2 = left, lane 3 = right
        }
        index >>= 1;
        poseidon_bn254_permute_coop(s, q);
        pbn_quad_gather(v, s);
        h = v[0];
    }
    if (live && q == 0) {
        u32 o8[8];
        fr_to_regular(o8, h);
        bool eq = true;
        const uint8_t *c = cap + 32 * (size_t)index;
        for (int i = 0; i < 8; i++) eq = eq && o8[i] == p2v_ld32(c + 4 * i);
        out[(u64)t * items + j] = eq ? 1 : 0;
    }
}

__global__ void __launch_bounds__(P2V_WAVE) p2v_fri_kernel(p2v_layout L, const uint8_t *__restrict__ proofs,
                                                           const p2v_proof_tab *__restrict__ tabs, const u32 *__restrict__ x_index,
                                                           u64 items, uint8_t *__restrict__ out) {
    const u64 j = (u64)blockIdx.x * P2V_WAVE + threadIdx.x;
    if (j >= items) return;
    const u64 p = j / L.rounds;
    const u32 r = (u32)(j - p * L.rounds);
    out[j] = (uint8_t)p2v_fri_lane(L, proofs + p * L.bytes, tabs[p], r, x_index[j]);
}

static int32_t p2v_grow(zklc_ctx *ctx, void **buf, size_t *cap, size_t bytes) {
    if (*cap >= bytes) return ZKLC_OK;
    if (*buf) ZKLC_HIP(ctx, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    ZKLC_HIP(ctx, hipMalloc(buf, bytes));
    *cap = bytes;
    return ZKLC_OK;
}

static double p2v_now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

extern "C" int32_t zklc_plonky2_verify_batch(zklc_ctx *ctx, zklc_plonky2_verifier *v, const uint8_t *proofs, uint64_t n,
                                             int32_t *status_out) {
    if (!ctx || !v || (n && (!proofs || !status_out))) return ZKLC_ERR_INVALID_ARG;
    if (v->device >= 0 && v->device != ctx->device) return ZKLC_ERR_INVALID_ARG;   // the buffers live on the first call's GPU
    if (!n) return ZKLC_OK;
    const double t0 = p2v_now_ms();
    const p2v_layout &L = v->L;
    const u64 R = L.rounds, items = n * R;
    // 1. the host stage of every proof (parse, transcript, PoW, vanishing, reduced openings) on the host threads
    const size_t tab_bytes = ((n * sizeof(p2v_proof_tab) + 255) & ~(size_t)255), idx_bytes = items * 4;
    std::vector<uint8_t> table(tab_bytes + idx_bytes, 0);
    p2v_proof_tab *tabs = (p2v_proof_tab *)table.data();
    u32 *idx = (u32 *)(table.data() + tab_bytes);
    p2v_parallel_for(n, 16, [&](uint64_t i) { status_out[i] = p2v_host_stage(v, proofs + i * L.bytes, &tabs[i], idx + i * R); });
    const double t1 = p2v_now_ms();
    // 2. buffers (grow-only, owned by the verifier), one copy of the proof bytes, one of the table
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    v->device = ctx->device;
    hipStream_t st = ctx->stream;
    const u64 seg = (items + P2V_WAVE - 1) / P2V_WAVE * P2V_WAVE;
    const size_t out_bytes = (size_t)(L.num_trees + 1) * items;
    int32_t rc;
    if ((rc = p2v_grow(ctx, &v->d_proofs, &v->cap_proofs, n * L.bytes)) || (rc = p2v_grow(ctx, &v->d_tab, &v->cap_tab, table.size())) ||
        (rc = p2v_grow(ctx, &v->d_out, &v->cap_out, out_bytes)))
        return rc;
    if (!v->d_cap) {
        size_t c = 0;
        if ((rc = p2v_grow(ctx, &v->d_cap, &c, v->cap.size()))) return rc;
        ZKLC_HIP(ctx, hipMemcpyAsync(v->d_cap, v->cap.data(), v->cap.size(), hipMemcpyHostToDevice, st));
    }
    if (v->cap_pinned < out_bytes) {
        if (v->h_pinned) ZKLC_HIP(ctx, hipHostFree(v->h_pinned));
        v->h_pinned = nullptr;
        v->cap_pinned = 0;
        ZKLC_HIP(ctx, hipHostMalloc(&v->h_pinned, out_bytes, hipHostMallocDefault));
        v->cap_pinned = out_bytes;
    }
    ZKLC_HIP(ctx, hipMemcpyAsync(v->d_proofs, proofs, n * L.bytes, hipMemcpyHostToDevice, st));
    ZKLC_HIP(ctx, hipMemcpyAsync(v->d_tab, table.data(), table.size(), hipMemcpyHostToDevice, st));
    // 3. the two kernels
    const uint8_t *d_pr = (const uint8_t *)v->d_proofs;
    const u32 *d_idx = (const u32 *)((const uint8_t *)v->d_tab + tab_bytes);
    uint8_t *d_out = (uint8_t *)v->d_out;
    hipEvent_t *ev = (hipEvent_t *)v->events;      // made once per verifier, destroyed with it
    for (int k = 0; k < 3; k++)
        if (!ev[k]) ZKLC_HIP(ctx, hipEventCreate(&ev[k]));
    ZKLC_HIP(ctx, hipEventRecord(ev[0], st));
    const dim3 gb((unsigned)((items + P2V_WAVE - 1) / P2V_WAVE));
    if (L.hasher == 0)
        hipLaunchKernelGGL(p2v_merkle_kernel<0>, dim3((unsigned)(seg * L.num_trees / P2V_WAVE)), dim3(P2V_WAVE), 0, st, L, d_pr,
                           (const uint8_t *)v->d_cap, d_idx, items, seg, d_out);
    else     // four lanes per item
        hipLaunchKernelGGL(p2v_merkle_bn254_coop_kernel, dim3((unsigned)(4 * seg * L.num_trees / P2V_WAVE)), dim3(P2V_WAVE), 0, st, L,
                           d_pr, (const uint8_t *)v->d_cap, d_idx, items, seg, d_out);
    ZKLC_HIP(ctx, hipGetLastError());
    ZKLC_HIP(ctx, hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(p2v_fri_kernel, gb, dim3(P2V_WAVE), 0, st, L, d_pr, (const p2v_proof_tab *)v->d_tab, d_idx, items,
                       d_out + (size_t)L.num_trees * items);
    ZKLC_HIP(ctx, hipGetLastError());
    ZKLC_HIP(ctx, hipEventRecord(ev[2], st));
    // 4. read-back after the stream has settled (zklc_internal.h zklc_readback_async), then wait for the copy
    ZKLC_HIP(ctx, zklc_readback_async(v->h_pinned, d_out, out_bytes, st));
    ZKLC_HIP(ctx, zklc_stream_wait(st));
    float ka = 0, kb = 0;
    (void)hipEventElapsedTime(&ka, ev[0], ev[1]);
    (void)hipEventElapsedTime(&kb, ev[1], ev[2]);
    // 5. per-item results -> per-proof statuses in the documented order: per round the initial trees, then per reduction the
    // consistency check and that layer's opening, then the final polynomial
    const uint8_t *res = (const uint8_t *)v->h_pinned, *fri = res + (size_t)L.num_trees * items;
    for (u64 p = 0; p < n; p++) {
        if (status_out[p] != ZKLC_PROOF_OK) continue;
        int32_t s = ZKLC_PROOF_OK;
        for (u64 r = 0; r < R && s == ZKLC_PROOF_OK; r++) {
            const u64 j = p * R + r;
            for (u32 t = 0; t < 4 && s == ZKLC_PROOF_OK; t++)
                if (!res[(u64)t * items + j]) s = ZKLC_PROOF_BAD_MERKLE;
            for (u32 i = 0; i < L.num_arities && s == ZKLC_PROOF_OK; i++) {
                if (fri[j] == 1 + i) s = ZKLC_PROOF_BAD_FRI;
                else if (!res[(u64)(4 + i) * items + j]) s = ZKLC_PROOF_BAD_MERKLE;
            }
            if (s == ZKLC_PROOF_OK && fri[j]) s = ZKLC_PROOF_BAD_FRI;
        }
        status_out[p] = s;
    }
    v->last_ms[0] = t1 - t0;
    v->last_ms[1] = ka;
    v->last_ms[2] = kb;
    v->last_ms[3] = p2v_now_ms() - t0;
    return ZKLC_OK;
}

extern "C" uint32_t zklc_plonky2_verifier_last_timings(const zklc_plonky2_verifier *v, double *out_ms, uint32_t cap) {
    if (!v || !out_ms) return 0;
    uint32_t k = cap < 4 ? cap : 4;
    for (uint32_t i = 0; i < k; i++) out_ms[i] = v->last_ms[i];
    return k;
}

extern "C" void zklc_plonky2_verifier_destroy(zklc_plonky2_verifier *v) {
    if (!v) return;
    if (v->device >= 0 && hipSetDevice(v->device) == hipSuccess) {
        for (void *p : {v->d_proofs, v->d_tab, v->d_out, v->d_cap})
            if (p) (void)hipFree(p);
        for (void *e : v->events)
            if (e) (void)hipEventDestroy((hipEvent_t)e);
    }
    if (v->h_pinned) (void)hipHostFree(v->h_pinned);
    delete v;
}
