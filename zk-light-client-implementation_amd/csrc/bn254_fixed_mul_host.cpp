// Batched fixed-base scalar multiplication, host path (plain C++): the lane functions of bn254_fixed_mul.cuh compiled with the host
// compiler and walked by threads, 256 lanes per task.  Same table, words and summary as the kernels of bn254_fixed_mul.hip; no GPU,
// no context.  Also the part of a table's creation that is the same with and without a GPU: the validation and the rows' bases
// (254 doublings and one inversion per row -- nothing to spread over lanes).
#include "bn254_fixed_mul.cuh"
#include "../../include/zklc.h"
#include <atomic>
#include <new>
#include <thread>

#define FBM_HOST_TASK 256u

// fn(task) for every task < n on min(n, nthreads) threads (0 = 16)
template <class Fn>
static void fbm_parallel_for(uint64_t n, uint32_t nthreads, const Fn &fn) {
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

// the generators of G1, (1, 2), and of G2 (gnark-crypto's, the precompile's), in gnark-crypto's memory layout
static const uint64_t FBM_GENERATOR_G1[8] = {0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full,
                                       0xa6ba871b8b1e1b3aull, 0x14f1d651eb8e167bull, 0xccdd46def0f28c58ull, 0x1c14ef83340fbe5eull};
static const uint64_t FBM_GENERATOR_G2[16] = {0x8e83b5d102bc2026ull, 0xdceb1935497b0172ull, 0xfbb8264797811adfull, 0x19573841af96503bull,
                                        0xafb4737da84c6140ull, 0x6043dd5a5802d8c4ull, 0x09e950fc52a02f86ull, 0x14fef0833aea7b6bull,
                                        0x619dfa9d886be9f6ull, 0xfe7fd297f59e9b78ull, 0xff9e1a62231b7dfeull, 0x28fd7eebae9e4206ull,
                                        0x64095b56c71856eeull, 0xdc57f922327d3cbbull, 0x55f935be33351076ull, 0x0da4a0e693fd6482ull};

static u64 fbm_record_words(u32 group) { return group == ZKLC_GROUP_G2 ? 2 * Fp2Field::PACKW : 2 * FpField::PACKW; }

template <class F>
static void fbm_row_bases(const uint64_t *base, u32 c, std::vector<u32> &out) {
    typedef typename F::T T;
    const int W = 8 * F::LIMBS / 10;
    const u32 rows = fbm_rows(c);
    out.assign((size_t)rows * 2 * F::PACKW, 0);
    const u32 *bw = reinterpret_cast<const u32 *>(base);
    T x = F::reduce(F::from_gnark(bw)), y = F::reduce(F::from_gnark(bw + W));
    for (u32 k = 0; k < rows; k++) {
        F::pack(out.data() + (size_t)k * 2 * F::PACKW, x);
        F::pack(out.data() + (size_t)k * 2 * F::PACKW + F::PACKW, y);
        if (k + 1 == rows) break;
        ec_xyzz<F> p = ec_double_affine<F>(x, y);
        for (u32 b = 1; b < c; b++) p = ec_double<F>(p);
        const T inv = F::inv(F::mul(p.ZZ, p.ZZZ));
        x = F::mul(p.X, F::mul(inv, p.ZZZ));
        y = F::mul(p.Y, F::mul(inv, p.ZZ));
    }
}

int32_t fbm_row_bases_host(u32 group, const uint64_t *base_words, u32 c, std::vector<u32> &row_bases) {
    if (group > ZKLC_GROUP_G2 || c < FBM_MIN_WINDOW || c > FBM_MAX_WINDOW || (uintptr_t)base_words & 7) return ZKLC_ERR_INVALID_ARG;
    const uint64_t *base = base_words ? base_words : group == ZKLC_GROUP_G2 ? FBM_GENERATOR_G2 : FBM_GENERATOR_G1;
    uint64_t any = 0;
    for (u32 i = 0; i < (group == ZKLC_GROUP_G2 ? 16u : 8u); i++) any |= base[i];
    if (!any) return ZKLC_ERR_INVALID_ARG;                          // the point at infinity has no table
    if (group == ZKLC_GROUP_G2) fbm_row_bases<Fp2Field>(base, c, row_bases);
    else fbm_row_bases<FpField>(base, c, row_bases);
    return ZKLC_OK;
}

template <class F>
static void fbm_build_table(const std::vector<u32> &row_bases, u32 c, std::vector<u32> &table) {
    const u32 E = fbm_entries(c), cpr = (E + FBM_CHUNK - 1) / FBM_CHUNK;
    const u64 total = (u64)fbm_rows(c) * E, lanes = (u64)fbm_rows(c) * cpr;
    std::vector<i32> ws((size_t)FBM_SLOTS * F::LIMBS * total);
    table.assign((size_t)total * 2 * F::PACKW, 0);
    fbm_parallel_for((lanes + FBM_HOST_TASK - 1) / FBM_HOST_TASK, 0, [&](uint64_t task) {
        const u64 end = (task + 1) * FBM_HOST_TASK < lanes ? (task + 1) * FBM_HOST_TASK : lanes;
        for (u64 t = task * FBM_HOST_TASK; t < end; t++) fbm_table_lane<F>(row_bases.data(), c, t, ws.data(), total);
    });
    const u64 groups = fbm_groups(total);
    const fbm_emit_packed<F> emit = {table.data()};
    fbm_parallel_for((groups + FBM_HOST_TASK - 1) / FBM_HOST_TASK, 0, [&](uint64_t task) {
        const u64 end = (task + 1) * FBM_HOST_TASK < groups ? (task + 1) * FBM_HOST_TASK : groups;
        for (u64 g = task * FBM_HOST_TASK; g < end; g++) {
            u64 first;
            (void)fbm_affine_group<F>(ws.data(), total, g, emit, first);
        }
    });
}

int32_t fbm_build_host(u32 group, const uint64_t *base_words, u32 c, zklc_fixed_base **out) {
    if (!out) return ZKLC_ERR_INVALID_ARG;
    *out = nullptr;
    std::vector<u32> row_bases;
    const int32_t rc = fbm_row_bases_host(group, base_words, c, row_bases);
    if (rc != ZKLC_OK) return rc;
    zklc_fixed_base *t = new (std::nothrow) zklc_fixed_base;
    if (!t) return ZKLC_ERR_OOM;
    t->group = group;
    t->c = c;
    t->rows = fbm_rows(c);
    t->entries = fbm_entries(c);
    try {
        if (group == ZKLC_GROUP_G2) fbm_build_table<Fp2Field>(row_bases, c, t->host);
        else fbm_build_table<FpField>(row_bases, c, t->host);
    } catch (const std::bad_alloc &) {
        delete t;
        return ZKLC_ERR_OOM;
    }
    *out = t;
    return ZKLC_OK;
}

extern "C" uint64_t zklc_bn254_fixed_base_table_bytes(uint32_t group, uint32_t window_bits) {
    if (group > ZKLC_GROUP_G2 || window_bits < FBM_MIN_WINDOW || window_bits > FBM_MAX_WINDOW) return 0;
    return (uint64_t)fbm_rows(window_bits) * fbm_entries(window_bits) * fbm_record_words(group) * 4;
}

extern "C" uint64_t zklc_bn254_fixed_mul_workspace_bytes(uint32_t group, uint64_t n) {
    if (group > ZKLC_GROUP_G2 || n > FBM_MAX_POINTS) return 0;
    const uint64_t limbs = group == ZKLC_GROUP_G2 ? Fp2Field::LIMBS : FpField::LIMBS;
    return FBM_SLOTS * limbs * 4 * (n ? n : 1);
}

template <class F>
static void fbm_mul_all(const zklc_fixed_base *t, const uint64_t *scalars, uint64_t n, uint32_t nthreads, u32 *words) {
    std::vector<i32> ws((size_t)FBM_SLOTS * F::LIMBS * n);
    const i32 *table = reinterpret_cast<const i32 *>(t->host.data());
    fbm_parallel_for((n + FBM_HOST_TASK - 1) / FBM_HOST_TASK, nthreads, [&](uint64_t task) {
        const u64 end = (task + 1) * FBM_HOST_TASK < n ? (task + 1) * FBM_HOST_TASK : n;
        for (u64 i = task * FBM_HOST_TASK; i < end; i++) fbm_mul_lane<F>(table, t->c, scalars, i, ws.data(), n);
    });
    const u64 groups = fbm_groups(n);
    const fbm_emit_gnark<F> emit = {words};
    fbm_parallel_for((groups + FBM_HOST_TASK - 1) / FBM_HOST_TASK, nthreads, [&](uint64_t task) {
        const u64 end = (task + 1) * FBM_HOST_TASK < groups ? (task + 1) * FBM_HOST_TASK : groups;
        for (u64 g = task * FBM_HOST_TASK; g < end; g++) {
            u64 first;
            (void)fbm_affine_group<F>(ws.data(), n, g, emit, first);
        }
    });
    // the scalars' multiples as limbs: nothing of them stays behind in freed memory
    volatile i32 *v = ws.data();
    for (size_t i = 0; i < ws.size(); i++) v[i] = 0;
}

static int32_t fbm_mul_host(const zklc_fixed_base *t, u32 group, const uint64_t *scalars, uint64_t n, uint32_t nthreads, uint64_t *words,
                            uint64_t *summary) {
    if (!t || t->group != group || t->host.empty() || !summary || n > FBM_MAX_POINTS || (n && (!scalars || !words)))
        return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)scalars | (uintptr_t)words) & 15 || (uintptr_t)summary & 7) return ZKLC_ERR_INVALID_ARG;
    summary[0] = 0;
    summary[1] = ~0ull;
    if (!n) return ZKLC_OK;
    try {
        if (group == ZKLC_GROUP_G2) fbm_mul_all<Fp2Field>(t, scalars, n, nthreads, (u32 *)words);
        else fbm_mul_all<FpField>(t, scalars, n, nthreads, (u32 *)words);
    } catch (const std::bad_alloc &) {
        return ZKLC_ERR_OOM;
    }
    const u64 width = group == ZKLC_GROUP_G2 ? 16 : 8;
    for (u64 i = 0; i < n; i++) {
        uint64_t o = 0;
        for (u64 j = 0; j < width; j++) o |= words[i * width + j];
        if (o) continue;
        if (!summary[0]++) summary[1] = i;
    }
    return ZKLC_OK;
}

extern "C" int32_t zklc_bn254_g1_fixed_mul_host(const zklc_fixed_base *tbl, const uint64_t *scalars_regular, uint64_t n, uint32_t nthreads,
                                                uint64_t *words, uint64_t *summary) {
    return fbm_mul_host(tbl, ZKLC_GROUP_G1, scalars_regular, n, nthreads, words, summary);
}
extern "C" int32_t zklc_bn254_g2_fixed_mul_host(const zklc_fixed_base *tbl, const uint64_t *scalars_regular, uint64_t n, uint32_t nthreads,
                                                uint64_t *words, uint64_t *summary) {
    return fbm_mul_host(tbl, ZKLC_GROUP_G2, scalars_regular, n, nthreads, words, summary);
}
