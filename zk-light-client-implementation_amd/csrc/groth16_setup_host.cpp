// The scalar stage of groth16.Setup on the host (plain C++): the lane functions of groth16_setup.cuh compiled with the host compiler
// and walked by threads, 256 lanes per task.  Same words as the kernels of groth16_setup.hip; no GPU, no context.  Also what every
// entry does on the host before anything else: the size checks and the constants made from the toxic waste.  Links with
// r1cs_eval_host.cpp (the system's handle) and nothing else.
//
// Where the kernels take the inverse transform of (1, tau, .., tau^(n-1)), this file takes the quotient formula
// L_j = (tau^n - 1) w^j / (n (tau - w^j)) with one inversion per task of 256 (prefix products), and the indicator of tau when tau
// is a point of the domain: both are the exact value made canonical, so the words are the same.  The transposition is a counting
// sort by one thread.  Every buffer and every named temporary that held a function of the toxic waste is overwritten before the call
// returns.
#include "groth16_setup.cuh"
#include "../../include/zklc.h"
#include <atomic>
#include <new>
#include <thread>

#define SETUP_HOST_TASK 256u
// gnark-crypto's rootOfUnity (order 2^28; = 5^((r - 1) / 2^28)) in Montgomery form
#define SETUP_ROOT28_MONT {0x80d13d9cu, 0x636e7355u, 0x2445ffd6u, 0xa22bf374u, 0x1eb203d8u, 0x56452ac0u, 0x2963f9e7u, 0x1860ef94u}

// fn(task) for every task < n on min(n, nthreads) threads (0 = 16)
template <class Fn>
static void setup_parallel_for(uint64_t n, uint32_t nthreads, const Fn &fn) {
    if (!nthreads) nthreads = 16;
    if (nthreads > n) nthreads = (uint32_t)n;
    std::atomic<uint64_t> next{0};
    auto work = [&] {
        for (uint64_t t = next.fetch_add(1); t < n; t = next.fetch_add(1)) fn(t);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nthreads; t++) {
        try {
            pool.emplace_back(work);
        } catch (...) {                                            // no further thread to be had: the ones running share the tasks
            break;
        }
    }
    work();
    for (auto &th : pool) th.join();
}

void setup_wipe(void *p, size_t bytes) {
    volatile unsigned char *v = (volatile unsigned char *)p;
    for (size_t i = 0; i < bytes; i++) v[i] = 0;
}

int32_t setup_check_sizes(const zklc_r1cs *s, uint32_t n_public, uint64_t n, uint32_t *log_n) {
    if (!s || !log_n) return ZKLC_ERR_INVALID_ARG;
    if (n < 2 || n < s->n_constraints || n > (1ull << SETUP_MAX_LOG) || (n & (n - 1))) return ZKLC_ERR_INVALID_ARG;
    if ((uint64_t)n_public + 1 > s->n_wires || s->n_wires > SETUP_MAX_WIRES) return ZKLC_ERR_INVALID_ARG;
    uint32_t l = 0;
    while ((1ull << l) < n) l++;
    *log_n = l;
    return ZKLC_OK;
}

bool setup_prepare(const uint64_t *toxic, uint32_t log_n, setup_consts *c) {
    // toxic is 8-byte aligned and no more: its words are read one by one (setup_to_mont), never 16 bytes at a time
    r1cs_el t[5];                                                   // tau, alpha, beta, gamma, delta: reduced, Montgomery
    for (int i = 0; i < 5; i++) t[i] = setup_to_mont((const u32 *)(toxic + 4 * i));
    const bool ok = !setup_is_zero(t[3].w) && !setup_is_zero(t[4].w);
    if (ok) {
        r1cs_el v[8];                                               // every intermediate lives here and is wiped below
        r1cs_el &p = v[0], &zm = v[1], &dinv = v[2], &ginv = v[3], &zt = v[4], &dr = v[5], &gr = v[6], &zd = v[7];
        p = t[0];
        for (u32 k = 0; k <= SETUP_MAX_LOG; k++) {
            for (int i = 0; i < 8; i++) c->tau_pow[k][i] = p.w[i];
            p = setup_mul(p.w, p.w);
        }
        zm = r1cs_sub(setup_load(c->tau_pow[log_n]), setup_one());
        dinv = setup_inv(t[4].w);
        ginv = setup_inv(t[3].w);
        zd = setup_mul(zm.w, dinv.w);
        zt = setup_to_regular(zd.w);
        dr = setup_to_regular(dinv.w);
        gr = setup_to_regular(ginv.w);
        for (int i = 0; i < 8; i++) {
            c->zt[i] = zt.w[i];
            c->beta[i] = t[2].w[i];
            c->alpha[i] = t[1].w[i];
            c->ginv[i] = gr.w[i];
            c->dinv[i] = dr.w[i];
        }
        setup_wipe(v, sizeof v);
    }
    setup_wipe(t, sizeof t);
    return ok;
}

// columns per bin (4) and the segments of the last bin, as the kernels count them
static void setup_plan(const zklc_r1cs *s, const std::vector<uint64_t> &col_ptr, uint64_t *out5) {
    for (int i = 0; i < 5; i++) out5[i] = 0;
    for (uint64_t key = 0; key + 1 < col_ptr.size(); key++) {
        const uint64_t len = col_ptr[key + 1] - col_ptr[key];
        out5[setup_bin_of(len)]++;
        if (setup_bin_of(len) == 3) out5[4] += setup_segments(len);
    }
}

// col_ptr [3 n_wires + 1]; with tterms: the transposed terms as well
static void setup_transpose(const zklc_r1cs *s, std::vector<uint64_t> &col_ptr, std::vector<uint64_t> *tterms) {
    const uint64_t nc = s->n_constraints, nw = s->n_wires;
    col_ptr.assign(3 * nw + 1, 0);
    for (uint64_t row = 0; row < 3 * nc; row++)
        for (uint64_t t = s->row_ptr[row]; t < s->row_ptr[row + 1]; t++) col_ptr[setup_key(row / nc, nw, s->terms[t]) + 1]++;
    for (uint64_t key = 0; key < 3 * nw; key++) col_ptr[key + 1] += col_ptr[key];
    if (!tterms) return;
    std::vector<uint64_t> at(col_ptr.begin(), col_ptr.end() - 1);
    tterms->resize(s->nnz);
    for (uint64_t row = 0; row < 3 * nc; row++)
        for (uint64_t t = s->row_ptr[row]; t < s->row_ptr[row + 1]; t++)
            (*tterms)[at[setup_key(row / nc, nw, s->terms[t])]++] = setup_transposed_term(s->terms[t], (u32)(row % nc));
}

extern "C" int32_t zklc_groth16_setup_plan(const zklc_r1cs *s, uint64_t *out5) {
    if (!s || !out5 || s->n_wires > SETUP_MAX_WIRES) return ZKLC_ERR_INVALID_ARG;
    try {
        std::vector<uint64_t> col_ptr;
        setup_transpose(s, col_ptr, nullptr);
        setup_plan(s, col_ptr, out5);
    } catch (const std::bad_alloc &) {
        return ZKLC_ERR_OOM;
    }
    return ZKLC_OK;
}

// L_j(tau) for the task's j, Montgomery
static void setup_lagrange_task(const setup_consts &c, uint32_t log_n, const r1cs_el *w_pow, const r1cs_el &zn, bool in_domain,
                                uint64_t task, u32 *L) {
    const uint64_t n = 1ull << log_n, j0 = task * SETUP_HOST_TASK, end = j0 + SETUP_HOST_TASK < n ? j0 + SETUP_HOST_TASK : n;
    r1cs_el tau = setup_load(c.tau_pow[0]);
    r1cs_el wj = setup_one();
    for (uint32_t k = 0; k < log_n; k++)
        if ((j0 >> k) & 1) wj = setup_mul(wj.w, w_pow[k].w);
    r1cs_el num[SETUP_HOST_TASK], den[SETUP_HOST_TASK], pre[SETUP_HOST_TASK];
    r1cs_el acc = setup_one();
    for (uint64_t j = j0; j < end; j++) {
        num[j - j0] = wj;
        den[j - j0] = r1cs_sub(tau, wj);
        pre[j - j0] = acc;
        if (!in_domain) acc = setup_mul(acc.w, den[j - j0].w);
        wj = setup_mul(wj.w, w_pow[0].w);
    }
    if (in_domain) {                                               // tau is a point of the domain: 1 there, 0 elsewhere
        for (uint64_t j = j0; j < end; j++) r1cs_store(L + 8 * j, setup_is_zero(den[j - j0].w) ? setup_one() : r1cs_zero());
    } else {
        r1cs_el ainv = setup_inv(acc.w);
        r1cs_el inv = setup_mul(ainv.w, zn.w);                      // (tau^n - 1) / n over the product of the denominators
        setup_wipe(&ainv, sizeof ainv);
        for (uint64_t j = end; j-- > j0;) {
            r1cs_store(L + 8 * j, setup_mul(setup_mul(num[j - j0].w, inv.w).w, pre[j - j0].w));
            inv = setup_mul(inv.w, den[j - j0].w);
        }
        setup_wipe(&inv, sizeof inv);
    }
    setup_wipe(den, sizeof den);
    setup_wipe(pre, sizeof pre);
    setup_wipe(&acc, sizeof acc);
    setup_wipe(&tau, sizeof tau);
}

static int32_t setup_scalars_host(const zklc_r1cs *s, const uint64_t *toxic, uint32_t n_public, uint64_t n, uint32_t nthreads,
                                  uint64_t *a_t, uint64_t *b_t, uint64_t *k, uint64_t *z) {
    uint32_t log_n = 0;
    if (setup_check_sizes(s, n_public, n, &log_n) != ZKLC_OK) return ZKLC_ERR_INVALID_ARG;
    if (!toxic || !a_t || !b_t || !k || !z) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)a_t | (uintptr_t)b_t | (uintptr_t)k | (uintptr_t)z) & 15 || (uintptr_t)toxic & 7) return ZKLC_ERR_INVALID_ARG;
    // every allocation comes before the first value made from the toxic waste: nothing of it is left behind by a failed one
    const uint64_t nw = s->n_wires;
    std::vector<uint64_t> col_ptr, tterms;
    setup_transpose(s, col_ptr, &tterms);
    std::vector<r1cs_q> pw(2 * n), abc_t(2 * 3 * nw);              // 16-byte aligned by their element type
    u32 *L = (u32 *)pw.data(), *abc = (u32 *)abc_t.data();
    setup_consts c;
    if (!setup_prepare(toxic, log_n, &c)) {
        setup_wipe(&c, sizeof c);
        return ZKLC_ERR_INVALID_ARG;
    }
    const uint64_t runs = (n + SETUP_RUN - 1) / SETUP_RUN;
    setup_parallel_for((runs + SETUP_HOST_TASK - 1) / SETUP_HOST_TASK, nthreads, [&](uint64_t task) {
        const uint64_t end = (task + 1) * SETUP_HOST_TASK < runs ? (task + 1) * SETUP_HOST_TASK : runs;
        for (uint64_t r = task * SETUP_HOST_TASK; r < end; r++) setup_powers_lane(c, n, r, L, (u32 *)z);
    });
    // the powers have given z; the Lagrange values take their place
    const u32 root28[8] = SETUP_ROOT28_MONT;
    r1cs_el w_pow[SETUP_MAX_LOG + 1];                               // w^(2^k), w of order n
    w_pow[0] = setup_load(root28);
    for (uint32_t i = log_n; i < SETUP_MAX_LOG; i++) w_pow[0] = setup_mul(w_pow[0].w, w_pow[0].w);
    for (uint32_t i = 1; i <= log_n; i++) w_pow[i] = setup_mul(w_pow[i - 1].w, w_pow[i - 1].w);
    const u32 n_words[8] = {(u32)n, (u32)(n >> 32), 0, 0, 0, 0, 0, 0};
    r1cs_el zm = r1cs_sub(setup_load(c.tau_pow[log_n]), setup_one());
    const bool in_domain = setup_is_zero(zm.w);
    const r1cs_el n_inv = setup_inv(setup_to_mont(n_words).w);      // 1 / n: nothing of the toxic waste
    r1cs_el zn = setup_mul(zm.w, n_inv.w);
    setup_parallel_for((n + SETUP_HOST_TASK - 1) / SETUP_HOST_TASK, nthreads,
                       [&](uint64_t task) { setup_lagrange_task(c, log_n, w_pow, zn, in_domain, task, L); });
    setup_parallel_for((3 * nw + SETUP_HOST_TASK - 1) / SETUP_HOST_TASK, nthreads, [&](uint64_t task) {
        const uint64_t end = (task + 1) * SETUP_HOST_TASK < 3 * nw ? (task + 1) * SETUP_HOST_TASK : 3 * nw;
        for (uint64_t key = task * SETUP_HOST_TASK; key < end; key++)
            r1cs_store(abc + 8 * key, r1cs_row_sum(tterms.data(), col_ptr[key], col_ptr[key + 1], 0, 1, L, s->coeffs.data()));
    });
    setup_parallel_for((nw + SETUP_HOST_TASK - 1) / SETUP_HOST_TASK, nthreads, [&](uint64_t task) {
        const uint64_t end = (task + 1) * SETUP_HOST_TASK < nw ? (task + 1) * SETUP_HOST_TASK : nw;
        for (uint64_t i = task * SETUP_HOST_TASK; i < end; i++) setup_combine_lane(c, i, nw, n_public, abc, (u32 *)a_t, (u32 *)b_t, (u32 *)k);
    });
    setup_wipe(pw.data(), pw.size() * sizeof(r1cs_q));
    setup_wipe(abc_t.data(), abc_t.size() * sizeof(r1cs_q));
    setup_wipe(&c, sizeof c);
    setup_wipe(&zm, sizeof zm);
    setup_wipe(&zn, sizeof zn);
    return ZKLC_OK;
}

extern "C" int32_t zklc_groth16_setup_scalars_host(const zklc_r1cs *s, const uint64_t *toxic, uint32_t n_public, uint64_t n,
                                                   uint32_t nthreads, uint64_t *a_t, uint64_t *b_t, uint64_t *k, uint64_t *z) {
    try {
        return setup_scalars_host(s, toxic, n_public, n, nthreads, a_t, b_t, k, z);
    } catch (const std::bad_alloc &) {
        return ZKLC_ERR_OOM;
    }
}
