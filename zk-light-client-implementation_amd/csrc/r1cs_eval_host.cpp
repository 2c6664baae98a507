// The constraint system on the host (plain C++): validation of the caller's CSR, the library's own form of it (classified, packed,
// binned), and A w, B w, C w with the lane functions of r1cs_eval.cuh compiled by the host compiler.  Same words and summary as the
// kernels of r1cs_eval.hip.  No GPU call, no context, nothing of the library but the Fr header: this file links on its own.
#include "r1cs_eval.cuh"
#include "../../include/zklc.h"
#include <atomic>
#include <new>
#include <thread>

#define R1CS_HOST_TASK 256u

// fn(task) for every task < n on min(n, nthreads) threads (0 = 16)
template <class Fn>
static void r1cs_parallel_for(uint64_t n, uint32_t nthreads, const Fn &fn) {
    if (!nthreads) nthreads = 16;
    if (nthreads > n) nthreads = (uint32_t)n;
    if (nthreads <= 1) {
        for (uint64_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::atomic<uint64_t> next(0);
    auto work = [&] {
        for (uint64_t i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i);
    };
    std::vector<std::thread> pool;
    pool.reserve(nthreads);
    for (uint32_t t = 1; t < nthreads; t++) {
        try {
            pool.emplace_back(work);
        } catch (...) {                                            // no further thread to be had: the ones running share the tasks
            break;
        }
    }
    work();
    for (auto &t : pool) t.join();
}

static int32_t r1cs_build(uint64_t nc, uint64_t n_wires, const uint64_t *row_ptr, const uint32_t *term_wire, const uint32_t *term_coeff,
                          uint64_t nnz, const uint64_t *coeffs, uint32_t n_coeff, zklc_r1cs **out) {
    // sizes first, each against an explicit bound: nothing below multiplies two of the caller's numbers, and nothing is read
    // before the bounds hold
    if (!out) return ZKLC_ERR_INVALID_ARG;
    *out = nullptr;
    if (nc > R1CS_MAX_CONSTRAINTS || n_wires < 1 || n_wires > R1CS_MAX_WIRES || nnz > R1CS_MAX_TERMS || n_coeff > R1CS_MAX_COEFFS)
        return ZKLC_ERR_INVALID_ARG;
    if (!row_ptr || (nnz && (!term_wire || !term_coeff)) || (n_coeff && !coeffs)) return ZKLC_ERR_INVALID_ARG;
    const uint64_t rows = 3 * nc;                                  // <= 3 2^30
    if (row_ptr[0] != 0 || row_ptr[rows] != nnz) return ZKLC_ERR_INVALID_ARG;
    for (uint64_t i = 0; i < rows; i++)
        if (row_ptr[i] > row_ptr[i + 1]) return ZKLC_ERR_INVALID_ARG;   // with the two ends fixed: every entry is within [0, nnz]
    for (uint32_t i = 0; i < n_coeff; i++)
        if (r1cs_ge_r((const u32 *)(coeffs + 4 * (uint64_t)i))) return ZKLC_ERR_INVALID_ARG;
    for (uint64_t t = 0; t < nnz; t++)
        if (term_wire[t] >= n_wires || term_coeff[t] >= n_coeff) return ZKLC_ERR_INVALID_ARG;

    zklc_r1cs *s = new zklc_r1cs();
    *out = s;
    s->n_constraints = nc;
    s->n_wires = n_wires;
    s->nnz = nnz;
    s->n_coeff = n_coeff;
    s->row_ptr.assign(row_ptr, row_ptr + rows + 1);
    s->coeffs.assign((const u32 *)coeffs, (const u32 *)coeffs + 8 * (uint64_t)n_coeff);
    std::vector<uint8_t> cls(n_coeff);
    for (uint32_t i = 0; i < n_coeff; i++) cls[i] = (uint8_t)r1cs_classify(s->coeffs.data() + 8 * (uint64_t)i);
    s->terms.resize(nnz);
    for (uint64_t t = 0; t < nnz; t++) s->terms[t] = r1cs_pack_term(term_wire[t], term_coeff[t], cls[term_coeff[t]]);
    // bins by row length; within a bin the rows keep their order, the outputs are never reordered
    auto bin_of = [](uint64_t len) { return len <= R1CS_BIN0_MAX ? 0 : len <= R1CS_BIN1_MAX ? 1 : 2; };
    for (uint64_t i = 0; i < rows; i++) {
        const uint64_t len = row_ptr[i + 1] - row_ptr[i];
        s->bin_rows[bin_of(len)]++;
        s->bin_terms[bin_of(len)] += len;
    }
    s->perm.resize(rows);
    uint64_t at[3] = {0, s->bin_rows[0], s->bin_rows[0] + s->bin_rows[1]};
    for (uint64_t i = 0; i < rows; i++) s->perm[at[bin_of(row_ptr[i + 1] - row_ptr[i])]++] = (u32)i;
    return ZKLC_OK;
}

int32_t r1cs_build_host(uint64_t n_constraints, uint64_t n_wires, const uint64_t *row_ptr, const uint32_t *term_wire,
                        const uint32_t *term_coeff, uint64_t nnz, const uint64_t *coeffs, uint32_t n_coeff, zklc_r1cs **out) {
    try {
        return r1cs_build(n_constraints, n_wires, row_ptr, term_wire, term_coeff, nnz, coeffs, n_coeff, out);
    } catch (const std::bad_alloc &) {
        if (out && *out) {
            delete *out;
            *out = nullptr;
        }
        return ZKLC_ERR_OOM;
    }
}

void r1cs_free_host(zklc_r1cs *s) { delete s; }

extern "C" uint64_t zklc_r1cs_workspace_bytes(const zklc_r1cs *s) { return s ? s->n_wires * 32 : 0; }   // n_wires <= 2^32

static int32_t r1cs_abc_host(const zklc_r1cs *s, const uint64_t *witness, uint64_t n, uint64_t *a, uint64_t *b, uint64_t *c,
                             uint32_t flags, uint32_t nthreads, uint64_t *summary) {
    if (!s || (flags & ~ZKLC_R1CS_CHECK) || n < s->n_constraints || n > R1CS_MAX_CONSTRAINTS) return ZKLC_ERR_INVALID_ARG;
    if (!witness || (n && (!a || !b || !c)) || ((flags & ZKLC_R1CS_CHECK) && !summary)) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)witness | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15 || (uintptr_t)summary & 7) return ZKLC_ERR_INVALID_ARG;
    const uint64_t nc = s->n_constraints;
    std::vector<r1cs_q> mont(2 * s->n_wires);                      // 16-byte aligned by its element type
    u32 *wm = (u32 *)mont.data();
    const u32 *wr = (const u32 *)witness;
    r1cs_parallel_for((s->n_wires + R1CS_HOST_TASK - 1) / R1CS_HOST_TASK, nthreads, [&](uint64_t task) {
        const uint64_t end = (task + 1) * R1CS_HOST_TASK < s->n_wires ? (task + 1) * R1CS_HOST_TASK : s->n_wires;
        for (uint64_t i = task * R1CS_HOST_TASK; i < end; i++) r1cs_store(wm + 8 * i, r1cs_witness_to_mont(wr + 8 * i));
    });
    u32 *o[3] = {(u32 *)a, (u32 *)b, (u32 *)c};
    const uint64_t total = 3 * n;                                  // output rows, the padding included
    r1cs_parallel_for((total + R1CS_HOST_TASK - 1) / R1CS_HOST_TASK, nthreads, [&](uint64_t task) {
        const uint64_t end = (task + 1) * R1CS_HOST_TASK < total ? (task + 1) * R1CS_HOST_TASK : total;
        for (uint64_t i = task * R1CS_HOST_TASK; i < end; i++) {
            const uint64_t m = i / n, j = i % n;
            r1cs_el v = r1cs_zero();
            if (j < nc) {
                const uint64_t row = m * nc + j;
                v = r1cs_row_sum(s->terms.data(), s->row_ptr[row], s->row_ptr[row + 1], 0, 1, wm, s->coeffs.data());
            }
            r1cs_store(o[m] + 8 * j, v);
        }
    });
    if (flags & ZKLC_R1CS_CHECK) {
        const uint64_t tasks = (nc + R1CS_HOST_TASK - 1) / R1CS_HOST_TASK;
        std::vector<uint64_t> bad(tasks, 0), first(tasks, ~0ull);
        r1cs_parallel_for(tasks, nthreads, [&](uint64_t task) {
            const uint64_t end = (task + 1) * R1CS_HOST_TASK < nc ? (task + 1) * R1CS_HOST_TASK : nc;
            for (uint64_t j = task * R1CS_HOST_TASK; j < end; j++)
                if (!r1cs_satisfied(o[0] + 8 * j, o[1] + 8 * j, o[2] + 8 * j)) {
                    if (!bad[task]++) first[task] = j;
                }
        });
        summary[0] = 0;
        summary[1] = ~0ull;
        for (uint64_t t = 0; t < tasks; t++) {
            summary[0] += bad[t];
            if (first[t] < summary[1]) summary[1] = first[t];
        }
    }
    return ZKLC_OK;
}

extern "C" int32_t zklc_r1cs_abc_host(const zklc_r1cs *s, const uint64_t *witness_regular, uint64_t n, uint64_t *a, uint64_t *b,
                                      uint64_t *c, uint32_t flags, uint32_t nthreads, uint64_t *summary) {
    try {
        return r1cs_abc_host(s, witness_regular, n, a, b, c, flags, nthreads, summary);
    } catch (const std::bad_alloc &) {
        return ZKLC_ERR_OOM;
    }
}
