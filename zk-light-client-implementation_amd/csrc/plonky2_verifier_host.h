// plonky2 verifier, host part (plain C++; csrc/plonky2_verifier_host.cpp): proof parser, transcript replay, the gate evaluators at
// zeta in the quadratic extension, the vanishing identity and the reduced openings -- the once-per-proof work.  The query phase
// is in csrc/plonky2_verifier.cuh (lane functions shared by the host path and the kernels of csrc/plonky2_verifier.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include <vector>
#include "../../include/zklc.h"
#include "plonky2_verifier.cuh"

struct zklc_plonky2_verifier {
    zklc_plonky2_params P;
    std::vector<zklc_plonky2_gate> gates;
    std::vector<uint64_t> extra, k_is;
    std::vector<uint8_t> cap, digest;       // 2^cap_h0 x 32 bytes, 32 bytes
    p2v_layout L;
    // device side (csrc/plonky2_verifier.hip): grow-only buffers owned by the verifier
    int device = -1;
    // (one call at a time per verifier: the buffers are shared state, zklc.h)
    void *d_proofs = nullptr, *d_tab = nullptr, *d_out = nullptr, *d_cap = nullptr;   // d_tab: per-proof tables, then query indices
    size_t cap_proofs = 0, cap_tab = 0, cap_out = 0;
    void *h_pinned = nullptr;               // page-locked result bytes
    size_t cap_pinned = 0;
    void *events[3] = {};                   // hipEvent_t around the two kernels
    double last_ms[4] = {};                 // host stage, kernel A, kernel B, total (last GPU call)
};

// the once-per-proof host stage: FORMAT, POW and VANISHING checks; on ZKLC_PROOF_OK fills `tab` and the query indices
// (num_query_rounds values, the low lde_bits bits of each challenge)
int32_t p2v_host_stage(const zklc_plonky2_verifier *v, const uint8_t *proof, p2v_proof_tab *tab, uint32_t *x_index);
// the query phase of one proof on the host, in the documented order
int32_t p2v_query_host(const zklc_plonky2_verifier *v, const uint8_t *proof, const p2v_proof_tab &tab, const uint32_t *x_index);
// csrc/plonky2_prover.hip: the creation arguments of a circuit (gate_extra and k_is read back from the GPU)
int32_t p2_circuit_verifier_args(zklc_plonky2_circuit *c, zklc_plonky2_params *params, std::vector<zklc_plonky2_gate> *gates,
                                 std::vector<uint64_t> *extra, std::vector<uint64_t> *k_is);
// runs fn(i) for i < n on min(n, nthreads) std::threads (nthreads 0 = 16; never more than 256)
void p2v_parallel_for(uint64_t n, uint32_t nthreads, const std::function<void(uint64_t)> &fn);
