/* Poseidon over BN254 Fr (t = 4, 8 full + 56 partial rounds, x^5) and the plonky2 hasher on it, in plain C -- TEST
 * INFRASTRUCTURE (see oracle/__init__.py).  Written from oracle/poseidon_bn254.py, which stays the definition: the same order
 * of operations, line by line.  The round constants and matrices are NOT compiled in: oracle/cport.py hands them over from
 * tests/golden/poseidon_bn254.json with one call of zklc_oracle_pbn_init, before any OpenMP region, so that nothing here
 * depends on the library's generated tables.  Fr elements cross the interface as 4 little-endian u64 words of the regular
 * (non-Montgomery) value; inside, the arithmetic is word-by-word Montgomery multiplication with `unsigned __int128`.
 */
#include <stdint.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef uint64_t u64;
typedef uint32_t u32;
typedef unsigned __int128 u128;

#define N_C 88       /* 4 + 3*4 + 4 | 56 | 3*4 */
#define N_S 392      /* 7 * 56 */
#define FULL 8
#define PARTIAL 56

/* r = 21888242871839275222246405745257275088548364400416034343698204186575808495617 */
static const u64 RMOD[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
static u64 N0INV;             /* -r^-1 mod 2^64 */
static u64 R2[4];             /* 2^512 mod r */
static u64 gC[N_C][4], gS[N_S][4], gM[16][4], gP[16][4];      /* Montgomery form */
static int g_ready;

static inline int fr_ge(const u64 *a, const u64 *b) {
    for (int i = 3; i >= 0; i--) { if (a[i] > b[i]) return 1; if (a[i] < b[i]) return 0; }
    return 1;
}
/* t (with the carry word hi) < 2 r -> r = t mod r, without a branch: the subtraction is kept when it does not borrow */
static inline void fr_reduce_once(u64 *r, const u64 *t, u64 hi) {
    u64 d[4], borrow = 0;
    for (int i = 0; i < 4; i++) {
        u128 x = (u128)t[i] - RMOD[i] - borrow;
        d[i] = (u64)x;
        borrow = (u64)(x >> 64) & 1;
    }
    const u64 keep = (u64)0 - (u64)(hi >= borrow);       /* t >= r  <=>  no borrow out of hi:t - r */
    for (int i = 0; i < 4; i++) r[i] = (d[i] & keep) | (t[i] & ~keep);
}
/* a, b < r -> a + b mod r (r < 2^254: the sum has no carry out) */
static inline void fr_add(u64 *r, const u64 *a, const u64 *b) {
    u128 c = 0;
    u64 t[4];
    for (int i = 0; i < 4; i++) { c += (u128)a[i] + b[i]; t[i] = (u64)c; c >>= 64; }
    fr_reduce_once(r, t, 0);
}
/* a * b / 2^256 mod r, a < 2^256 and b < r -> < r */
static inline void fr_mul(u64 *r, const u64 *a, const u64 *b) {
    u64 t[6] = {0, 0, 0, 0, 0, 0};
#pragma GCC unroll 4
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
#pragma GCC unroll 4
        for (int j = 0; j < 4; j++) { c += (u128)a[j] * b[i] + t[j]; t[j] = (u64)c; c >>= 64; }
        c += t[4];
        t[4] = (u64)c;
        t[5] = (u64)(c >> 64);
        const u64 m = t[0] * N0INV;
        c = ((u128)m * RMOD[0] + t[0]) >> 64;
#pragma GCC unroll 3
        for (int j = 1; j < 4; j++) { c += (u128)m * RMOD[j] + t[j]; t[j - 1] = (u64)c; c >>= 64; }
        c += t[4];
        t[3] = (u64)c;
        t[4] = t[5] + (u64)(c >> 64);
    }
    fr_reduce_once(r, t, t[4]);
}
static inline void fr_to_mont(u64 *r, const u64 *a) { fr_mul(r, a, R2); }           /* any a < 2^256 */
static inline void fr_from_mont(u64 *r, const u64 *a) { const u64 one[4] = {1, 0, 0, 0}; fr_mul(r, a, one); }
static inline void fr_exp5(u64 *x) {
    u64 x2[4], x4[4];
    fr_mul(x2, x, x);
    fr_mul(x4, x2, x2);
    fr_mul(x, x4, x);
}
/* out[i] = sum_j m[j][i] * s[j] */
static inline void fr_mix(u64 s[4][4], u64 (*m)[4]) {
    u64 o[4][4], p[4];
    for (int i = 0; i < 4; i++) {
        fr_mul(o[i], m[0 * 4 + i], s[0]);
        for (int j = 1; j < 4; j++) { fr_mul(p, m[j * 4 + i], s[j]); fr_add(o[i], o[i], p); }
    }
    memcpy(s, o, sizeof o);
}
/* oracle/poseidon_bn254.py `permute`, on a state in Montgomery form */
static void permute_mont(u64 s[4][4]) {
    for (int k = 0; k < 4; k++) fr_add(s[k], s[k], gC[k]);
    for (int i = 0; i < FULL / 2 - 1; i++) {
        for (int k = 0; k < 4; k++) { fr_exp5(s[k]); fr_add(s[k], s[k], gC[(i + 1) * 4 + k]); }
        fr_mix(s, gM);
    }
    for (int k = 0; k < 4; k++) { fr_exp5(s[k]); fr_add(s[k], s[k], gC[(FULL / 2) * 4 + k]); }
    fr_mix(s, gP);
    for (int i = 0; i < PARTIAL; i++) {
        u64 new0[4], p[4];
        fr_exp5(s[0]);
        fr_add(s[0], s[0], gC[(FULL / 2 + 1) * 4 + i]);
        fr_mul(new0, gS[7 * i], s[0]);
        for (int j = 1; j < 4; j++) { fr_mul(p, gS[7 * i + j], s[j]); fr_add(new0, new0, p); }
        for (int k = 1; k < 4; k++) { fr_mul(p, s[0], gS[7 * i + 4 + k - 1]); fr_add(s[k], s[k], p); }
        memcpy(s[0], new0, 32);
    }
    for (int i = 0; i < FULL / 2 - 1; i++) {
        for (int k = 0; k < 4; k++) { fr_exp5(s[k]); fr_add(s[k], s[k], gC[(FULL / 2 + 1) * 4 + PARTIAL + i * 4 + k]); }
        fr_mix(s, gM);
    }
    for (int k = 0; k < 4; k++) fr_exp5(s[k]);
    fr_mix(s, gM);
}

/* C: 88, S: 392, M and P: 16 (row-major 4 x 4) elements of 4 little-endian u64 words, regular values < r.  -> 0, or -1 */
int zklc_oracle_pbn_init(const u64 *C, u32 n_c, const u64 *S, u32 n_s, const u64 *M, const u64 *Pm) {
    if (!C || !S || !M || !Pm || n_c != N_C || n_s != N_S) return -1;
    u64 inv = 1;                                       /* Newton: inv = r^-1 mod 2^64 */
    for (int i = 0; i < 6; i++) inv *= 2 - RMOD[0] * inv;
    N0INV = (u64)0 - inv;
    u64 x[4] = {1, 0, 0, 0};                           /* 2^k mod r by doubling */
    for (int k = 0; k < 512; k++) fr_add(x, x, x);
    memcpy(R2, x, 32);
    for (u32 i = 0; i < N_C; i++) { if (fr_ge(C + 4 * i, RMOD)) return -1; fr_to_mont(gC[i], C + 4 * i); }
    for (u32 i = 0; i < N_S; i++) { if (fr_ge(S + 4 * i, RMOD)) return -1; fr_to_mont(gS[i], S + 4 * i); }
    for (u32 i = 0; i < 16; i++) {
        if (fr_ge(M + 4 * i, RMOD) || fr_ge(Pm + 4 * i, RMOD)) return -1;
        fr_to_mont(gM[i], M + 4 * i);
        fr_to_mont(gP[i], Pm + 4 * i);
    }
    g_ready = 1;
    return 0;
}
int zklc_oracle_pbn_ready(void) { return g_ready; }
void zklc_oracle_pbn_modulus(u64 *out4) { memcpy(out4, RMOD, 32); }

/* state: 4 elements of 4 words, any value below 2^256 (reduced mod r on the way in, as the Python does) */
void zklc_oracle_pbn_permute(u64 *state) {
    u64 s[4][4];
    for (int k = 0; k < 4; k++) fr_to_mont(s[k], state + 4 * k);
    permute_mont(s);
    for (int k = 0; k < 4; k++) fr_from_mont(state + 4 * k, s[k]);
}
void zklc_oracle_pbn_permute_many(u64 *states, u64 n) {
    for (u64 i = 0; i < n; i++) zklc_oracle_pbn_permute(states + 16 * i);
}

/* hash_no_pad: three Goldilocks elements per limb (little-endian u64 words), three limbs into state[1..4] per permutation; a
 * short last chunk overwrites only the limbs it reaches.  `in` is read with a stride (1 for a contiguous row). */
void zklc_oracle_pbn_hash_no_pad(const u64 *in, u64 stride, u64 len, u64 *out4) {
    u64 s[4][4];
    memset(s, 0, sizeof s);
    for (u64 off = 0; off < len; off += 9) {
        const u64 m = len - off < 9 ? len - off : 9;
        for (u64 j = 0; j < m; j += 3) {
            u64 limb[4] = {0, 0, 0, 0};
            for (u64 k = 0; k < 3 && j + k < m; k++) limb[k] = in[(off + j + k) * stride];
            fr_to_mont(s[j / 3 + 1], limb);
        }
        permute_mont(s);
    }
    fr_from_mont(out4, s[0]);
}
void zklc_oracle_pbn_hash_or_noop(const u64 *in, u64 stride, u64 len, u64 *out4) {
    if (len <= 3) {
        for (u64 k = 0; k < 4; k++) out4[k] = k < len ? in[k * stride] : 0;
        return;
    }
    zklc_oracle_pbn_hash_no_pad(in, stride, len, out4);
}
void zklc_oracle_pbn_two_to_one(const u64 *l, const u64 *r, u64 *out4) {
    u64 s[4][4];
    memset(s, 0, sizeof s);
    fr_to_mont(s[2], l);
    fr_to_mont(s[3], r);
    permute_mont(s);
    fr_from_mont(out4, s[0]);
}
/* to_vec: the 32 little-endian bytes in chunks of 7 -> five Goldilocks elements (the last one holds 4 bytes) */
void zklc_oracle_pbn_to_vec(const u64 *h4, u64 *out5) {
    for (int k = 0; k < 5; k++) {
        const int bit = 56 * k, w = bit >> 6, sh = bit & 63;
        u64 v = h4[w] >> sh;
        if (sh && w + 1 < 4) v |= h4[w + 1] << (64 - sh);
        out5[k] = v & ((1ULL << 56) - 1);
    }
}

/* mat: [width] columns, column c at mat + c * stride, leaf i = (mat[c * stride + i])_c.  Tree layout as
 * zklc_oracle_gl_merkle_commit: levels concatenated, leaves first, cap last, 4 words per digest.  -> threads used, -1 */
int zklc_oracle_bn254_merkle_commit(const u64 *mat, u64 stride, int log_leaves, u32 width, int cap_height, u64 *tree, int nthreads) {
    if (!g_ready || !mat || !tree || log_leaves < 0 || cap_height < 0 || cap_height > log_leaves) return -1;
    const u64 n = 1ULL << log_leaves;
    int used = 1;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
    used = nthreads > 0 ? nthreads : omp_get_max_threads();
#pragma omp parallel for schedule(static)
#endif
    for (int64_t i = 0; i < (int64_t)n; i++) zklc_oracle_pbn_hash_or_noop(mat + i, stride, width, tree + 4 * i);
    u64 *level = tree;
    for (int l = 0; l < log_leaves - cap_height; l++) {
        const u64 parents = n >> (l + 1);
        u64 *next = level + (4ULL << (log_leaves - l));
#ifdef _OPENMP
#pragma omp parallel for schedule(static)
#endif
        for (int64_t i = 0; i < (int64_t)parents; i++) zklc_oracle_pbn_two_to_one(level + 8 * i, level + 8 * i + 4, next + 4 * i);
        level = next;
    }
    return used;
}
