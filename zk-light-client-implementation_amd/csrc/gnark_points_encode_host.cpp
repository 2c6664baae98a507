// Encoding of gnark point arrays, host path (plain C++): the lane functions of gnark_points_encode.cuh compiled with the host
// compiler, 256 points per task.  Same classes, bytes and summary as the kernels of gnark_points_encode.hip; no GPU, no context.
#include "gnark_points_encode.cuh"
#include "groth16_verifier_host.h"
#include "plonky2_verifier_host.h"   // p2v_parallel_for
#include <string.h>

#define GK_HOST_TASK 256u

static int32_t gk_encode_host(const uint64_t *words, uint64_t n, uint32_t flags, uint32_t nthreads, uint8_t *bytes, uint32_t *status,
                              uint64_t *summary, bool g2) {
    if (!summary || (flags & ~(ZKLC_POINTS_COMPRESSED | ZKLC_POINTS_VALIDATE))) return ZKLC_ERR_INVALID_ARG;
    if (n > (1ull << 31) || (n && (!bytes || !words || !status))) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)bytes | (uintptr_t)words) & 15 || (uintptr_t)status & 3 || (uintptr_t)summary & 7) return ZKLC_ERR_INVALID_ARG;
    const g16_key &key = g16_key_constants();
    const uint32_t compressed = flags & ZKLC_POINTS_COMPRESSED, validate = (flags & ZKLC_POINTS_VALIDATE) != 0;
    const uint64_t stride = (g2 ? 128u : 64u) >> compressed, width = g2 ? 32 : 16;
    const u32 *src = (const u32 *)words;
    p2v_parallel_for((n + GK_HOST_TASK - 1) / GK_HOST_TASK, nthreads, [&](uint64_t task) {
        const uint64_t end = (task + 1) * GK_HOST_TASK < n ? (task + 1) * GK_HOST_TASK : n;
        for (uint64_t i = task * GK_HOST_TASK; i < end; i++) {
            u32 w[32], st;
            uint8_t *slot = bytes + i * stride;
            gk_load_words(w, src + i * width, (int)(width / 4));
            if (g2) st = compressed ? gk_g2_encode<1>(key, w, validate, slot) : gk_g2_encode<0>(key, w, validate, slot);
            else st = compressed ? gk_g1_encode<1>(w, validate, slot) : gk_g1_encode<0>(w, validate, slot);
            status[i] = st;
        }
    });
    summary[0] = summary[1] = summary[2] = 0;
    summary[3] = ~0ull;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t st = status[i];
        summary[st == GK_OK ? 0 : st == GK_INFINITY ? 1 : 2]++;
        if (st >= GK_BAD_ENCODING && summary[3] == ~0ull) summary[3] = i;
    }
    return ZKLC_OK;
}

extern "C" int32_t zklc_bn254_g1_encode_host(const uint64_t *words, uint64_t n, uint32_t flags, uint32_t nthreads, uint8_t *bytes,
                                             uint32_t *status, uint64_t *summary) {
    return gk_encode_host(words, n, flags, nthreads, bytes, status, summary, false);
}
extern "C" int32_t zklc_bn254_g2_encode_host(const uint64_t *words, uint64_t n, uint32_t flags, uint32_t nthreads, uint8_t *bytes,
                                             uint32_t *status, uint64_t *summary) {
    return gk_encode_host(words, n, flags, nthreads, bytes, status, summary, true);
}
