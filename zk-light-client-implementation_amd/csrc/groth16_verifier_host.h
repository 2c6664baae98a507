// Groth16 verifier, state shared by the host path (groth16_verifier_host.cpp, plain C++) and the GPU path (groth16_verify.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/zklc.h"
#include "groth16_verify.cuh"

#define G16_MAX_PUBLIC 4096u          // 4096 x 64 x 15 table entries of 80 bytes = 315 MB; a larger key is refused
#define G16_MAX_BATCH (1u << 24)

struct zklc_groth16_verifier {
    g16_key key;
    std::vector<g16_tab_entry> tab;   // [n_public][64 windows][15]
    std::vector<uint8_t> k_inf;       // [n_public + 1] (padded to a multiple of 4)
    // device side (groth16_verify.hip): grow-only buffers owned by the verifier; one call at a time per verifier
    int device = -1;
    void *d_key = nullptr, *d_tab = nullptr, *d_kinf = nullptr;
    void *d_in = nullptr, *d_g1 = nullptr, *d_g2 = nullptr, *d_out = nullptr;
    size_t cap_in = 0, cap_g1 = 0, cap_g2 = 0, cap_out = 0;
    void *h_in = nullptr, *h_out = nullptr;   // page-locked staging: proofs + inputs up, statuses + pairing verdicts down
    size_t cap_h_in = 0, cap_h_out = 0;
    void *events[4] = {};
    double last_ms[4] = {};           // upload, validation / kSum kernel, pairing kernel, total (last GPU call)
};

// a * b without wrapping; false when the product does not fit
inline bool g16_mul_ok(uint64_t a, uint64_t b, uint64_t *out) { return !__builtin_mul_overflow(a, b, out); }
// a key that holds only the constants of the twist equation and of the Fp2 square root: twist_b = 3 / (9 + u), half = 1 / 2, the
// rest zero (groth16_verifier_host.cpp: host code, computed once with the field functions)
const g16_key &g16_key_constants();
