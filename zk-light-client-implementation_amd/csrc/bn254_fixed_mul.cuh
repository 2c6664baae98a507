// Batched fixed-base scalar multiplication in BN254 G1 and G2, the lane functions: out[i] = scalars[i] * P for ONE base P and n
// scalars -- what `groth16.Setup(r1cs)` (gnark-plonky2-verifier/cmd/compile.go:40; gnark v0.9.1 backend/groth16/bn254/setup.go,
// un-vendored) does through gnark-crypto's `bn254.BatchScalarMultiplicationG1` / `G2` to turn the key's scalars into its point
// arrays.  Shared by the kernels of bn254_fixed_mul.hip and by the host path of bn254_fixed_mul_host.cpp (g++), so both compute every
// word alike by construction; the output is canonical, so it is also what Python integers give.  DESIGN.md 3.11.
//
// Table.  rows = ceil(254 / c) rows of E = 2^c - 1 affine points: entry (k, d - 1) = d 2^(c k) P, in the packed record form of the
// multi-exponentiation (bn254_msm_lane.cuh: x then y, canonical values of the internal domain, 64 bytes in G1, 128 in G2).  A
// scalar below r has rows digits of c bits; its multiple is the sum of one entry per non-zero digit: at most `rows` mixed additions
// (ec_add_affine, accumulator in XYZZ) and no doubling.  P must be a finite point of order r: no multiple d 2^(c k) P below r is
// then the point at infinity, which a packed record cannot hold.
//
// From XYZZ to affine.  x = X / ZZ, y = Y / ZZZ costs one inversion (a Fermat chain of ~380 multiplications against ~11 per mixed
// addition), so it is shared by Montgomery's trick over FBM_INV_GROUP points that meet through the workspace:
//   stage A  one lane per point: the sum above, X, Y, ZZ, ZZZ stored as limbs (slots 0-3 of the workspace);
//   stage B  one lane per group g of the points g, g + n_groups, g + 2 n_groups, ...: forward, the running product of the ZZ ZZZ that
//            are not zero (slot 4); one inversion; backward, 1 / (ZZ ZZZ) of each point from the running products, x and y out.
// A point at infinity (ZZ = 0: a zero scalar) leaves the running product as it is -- it neither poisons its group nor is inverted --
// and gives all-zero words; a group of nothing but such points inverts nothing.  The workspace is one array per limb
// (word ((slot LIMBS + limb) n + point)): consecutive lanes touch consecutive words in both stages.
//
// The table is built the same way: stage A' gives every lane FBM_CHUNK consecutive multiples of one row's base -- the first by
// double-and-add, the others by one mixed addition each -- and stage B packs instead of writing gnark's words.
#pragma once
#include "bn254_msm_lane.cuh"

#define FBM_MIN_WINDOW 4u
#define FBM_MAX_WINDOW 16u
#define FBM_SCALAR_BITS 254u
#define FBM_INV_GROUP 16u          // points that share one inversion
#define FBM_CHUNK 16u              // consecutive table entries of one lane of the table build
#define FBM_SLOTS 5u               // X, Y, ZZ, ZZZ, running product
#define FBM_MAX_POINTS (1ull << 30)

// the table's and the groups' sizes: also asked for by the host code that launches the kernels
#if defined(__HIPCC__)
#define FBM_BOTH __host__ __device__ __forceinline__
#else
#define FBM_BOTH static inline
#endif
FBM_BOTH u32 fbm_rows(u32 c) { return (FBM_SCALAR_BITS + c - 1) / c; }
FBM_BOTH u32 fbm_entries(u32 c) { return (1u << c) - 1; }
FBM_BOTH u64 fbm_groups(u64 n) { return (n + FBM_INV_GROUP - 1) / FBM_INV_GROUP; }

// 16 bytes moved by one access
struct __attribute__((aligned(16), may_alias)) fbm_q {
    u32 w[4];
};
// nq x 16 bytes of words to a 16-byte aligned address
ZKLC_HD void fbm_store_words(u32 *dst, const u32 *w, int nq) {
    for (int i = 0; i < nq; i++) {
        fbm_q q;
        for (int j = 0; j < 4; j++) q.w[j] = w[4 * i + j];
        reinterpret_cast<fbm_q *>(dst)[i] = q;
    }
}

template <class F>
ZKLC_HD typename F::T fbm_ws_load(const i32 *ws, u64 n, u32 slot, u64 p) {
    i32 t[F::LIMBS];
    for (int l = 0; l < F::LIMBS; l++) t[l] = ws[((u64)slot * F::LIMBS + l) * n + p];
    return F::load(t);
}
template <class F>
ZKLC_HD void fbm_ws_store(i32 *ws, u64 n, u32 slot, u64 p, const typename F::T &a) {
    i32 t[F::LIMBS];
    F::store(t, a);
    for (int l = 0; l < F::LIMBS; l++) ws[((u64)slot * F::LIMBS + l) * n + p] = t[l];
}
template <class F>
ZKLC_HD void fbm_ws_store_point(i32 *ws, u64 n, u64 p, const ec_xyzz<F> &a) {
    fbm_ws_store<F>(ws, n, 0, p, a.X);
    fbm_ws_store<F>(ws, n, 1, p, a.Y);
    fbm_ws_store<F>(ws, n, 2, p, a.ZZ);
    fbm_ws_store<F>(ws, n, 3, p, a.ZZZ);
}

// digit k (c bits) of a scalar of eight words
ZKLC_HD u32 fbm_digit(const u32 *sw, u32 k, u32 c) {
    const u32 bit = k * c, wi = bit >> 5, sh = bit & 31;
    u64 x = (u64)sw[wi] >> sh;
    if (wi + 1 < 8) x |= (u64)sw[wi + 1] << (32 - sh);
    return (u32)x & ((1u << c) - 1);
}

// stage A: scalar i (regular form, reduced here when it is not below r) times the table's base, into the workspace
template <class F>
ZKLC_HD void fbm_mul_lane(const i32 *table, u32 c, const u64 *scalars, u64 i, i32 *ws, u64 n) {
    u32 sw[8];
    msm_load_scalar(scalars, (u32)i, sw);
    const u32 rows = fbm_rows(c), E = fbm_entries(c);
    ec_xyzz<F> acc = ec_infinity<F>();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 k = 0; k < rows; k++) {
        const u32 d = fbm_digit(sw, k, c);
        if (!d) continue;
        msm_cpoint<F> rec;
        msm_fetch_cpoint<F, true>(rec, table, k * E + d - 1);
        typename F::T x, y;
        msm_cpoint_xy<F, true>(rec, x, y);
        acc = ec_add_affine<F>(acc, x, y, 0);
    }
    fbm_ws_store_point<F>(ws, n, i, acc);
}

// stage A': lane t of the table build: entries d0 .. d0 + FBM_CHUNK - 1 (as far as the row goes) of row k = t / chunks-per-row;
// row_bases: rows packed records 2^(c k) P.  total = rows E
template <class F>
ZKLC_HD void fbm_table_lane(const u32 *row_bases, u32 c, u64 t, i32 *ws, u64 total) {
    const u32 E = fbm_entries(c), cpr = (E + FBM_CHUNK - 1) / FBM_CHUNK;
    const u32 k = (u32)(t / cpr), d0 = 1 + (u32)(t % cpr) * FBM_CHUNK;
    const u32 cnt = E - d0 + 1 < FBM_CHUNK ? E - d0 + 1 : FBM_CHUNK;
    const typename F::T x = F::unpack(row_bases + (size_t)k * 2 * F::PACKW), y = F::unpack(row_bases + (size_t)k * 2 * F::PACKW + F::PACKW);
    ec_xyzz<F> acc = ec_infinity<F>();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int b = (int)c - 1; b >= 0; b--) {
        acc = ec_double<F>(acc);
        if ((d0 >> b) & 1) acc = ec_add_affine<F>(acc, x, y, 0);
    }
    const u64 p0 = (u64)k * E + d0 - 1;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 j = 0; j < cnt; j++) {
        fbm_ws_store_point<F>(ws, total, p0 + j, acc);
        if (j + 1 < cnt) acc = ec_add_affine<F>(acc, x, y, 0);
    }
}

// what stage B does with a point: gnark's words (the multiplication) ...
template <class F>
struct fbm_emit_gnark {
    u32 *out;                      // n x 2 W words
    static constexpr int W = 8 * F::LIMBS / 10;
    ZKLC_M void point(u64 p, const typename F::T &x, const typename F::T &y) const {
        u32 w[2 * W];
        F::to_gnark(w, x);
        F::to_gnark(w + W, y);
        put(p, w);
    }
    ZKLC_M void infinity(u64 p) const {
        u32 w[2 * W];
        for (int i = 0; i < 2 * W; i++) w[i] = 0;
        put(p, w);
    }
    ZKLC_M void put(u64 p, const u32 *w) const { fbm_store_words(out + p * (2 * W), w, 2 * W / 4); }
};
// ... or a packed record (the table build; no entry of a table is the point at infinity)
template <class F>
struct fbm_emit_packed {
    u32 *out;                      // n x 2 PACKW words
    ZKLC_M void point(u64 p, const typename F::T &x, const typename F::T &y) const {
        u32 w[2 * F::PACKW];
        F::pack(w, x);
        F::pack(w + F::PACKW, y);
        put(p, w);
    }
    ZKLC_M void infinity(u64 p) const {
        u32 w[2 * F::PACKW];
        for (int i = 0; i < 2 * F::PACKW; i++) w[i] = 0;
        put(p, w);
    }
    ZKLC_M void put(u64 p, const u32 *w) const { fbm_store_words(out + p * (2 * F::PACKW), w, 2 * F::PACKW / 4); }
};

// stage B: group g < fbm_groups(n).  Returns the number of its points at infinity; first_inf = the smallest index among them
template <class F, class Emit>
ZKLC_HD u32 fbm_affine_group(i32 *ws, u64 n, u64 g, const Emit &emit, u64 &first_inf) {
    typedef typename F::T T;
    const u64 n_groups = fbm_groups(n);
    T acc = F::one();
    u32 finite = 0, n_inf = 0;
    u64 last = g;
    first_inf = ~0ull;
    for (u64 p = g; p < n; p += n_groups) {
        const T zz = fbm_ws_load<F>(ws, n, 2, p);
        if (!F::is_zero(zz)) {
            acc = F::mul(acc, F::mul(zz, fbm_ws_load<F>(ws, n, 3, p)));
            finite = 1;
        }
        fbm_ws_store<F>(ws, n, 4, p, acc);
        last = p;
    }
    T inv = F::one();
    if (finite) inv = F::inv(acc);                  // of a product of non-zero values
    for (u64 p = last;; p -= n_groups) {
        const T zz = fbm_ws_load<F>(ws, n, 2, p);
        if (F::is_zero(zz)) {
            emit.infinity(p);
            n_inf++;
            first_inf = p;                          // the walk goes down: the last one written is the smallest
        } else {
            const T zzz = fbm_ws_load<F>(ws, n, 3, p);
            const T before = p == g ? F::one() : fbm_ws_load<F>(ws, n, 4, p - n_groups);
            const T zi = F::mul(inv, before);       // 1 / (ZZ ZZZ) of this point
            inv = F::mul(inv, F::mul(zz, zzz));
            emit.point(p, F::mul(fbm_ws_load<F>(ws, n, 0, p), F::mul(zi, zzz)), F::mul(fbm_ws_load<F>(ws, n, 1, p), F::mul(zi, zz)));
        }
        if (p == g) break;
    }
    return n_inf;
}

// ---- the table as the library keeps it (host side; the device array is bn254_fixed_mul.hip's) ----
#include <vector>
struct zklc_fixed_base {
    u32 group = 0, c = 0, rows = 0, entries = 0;      // entries per row
    std::vector<u32> host;                            // rows x entries packed records (no context at create)
    int device = -1;
    void *d_table = nullptr;
};
// bn254_fixed_mul_host.cpp (no GPU call)
// validates group, window and base (NULL: the generator); the rows' bases 2^(c k) P as packed records.  ZKLC_OK or INVALID_ARG
int32_t fbm_row_bases_host(u32 group, const uint64_t *base_words, u32 c, std::vector<u32> &row_bases);
int32_t fbm_build_host(u32 group, const uint64_t *base_words, u32 c, zklc_fixed_base **out);
