// The scalar stage of `groth16.Setup(r1cs)` (gnark-plonky2-verifier/cmd/compile.go:40; gnark backend/groth16/bn254/setup.go,
// un-vendored): from the constraint system and the toxic waste (tau, alpha, beta, gamma, delta) to the discrete logarithms of the
// key's points -- a_t[i] = sum_j A_ji L_j(tau), b_t, k[i] = (beta a_t[i] + alpha b_t[i] + c_t[i]) / (gamma | delta),
// z[i] = tau^i (tau^n - 1) / delta -- which the batched fixed-base multiplication (bn254_fixed_mul.cuh) turns into points.  The lane
// functions: one run of powers, one column key, one wire.  Shared by the kernels of groth16_setup.hip and by the host path of
// groth16_setup_host.cpp (g++), so both compute every word alike by construction.  DESIGN.md 3.12.
//
// Number forms.  Inside, every value is kept as r1cs_eval.cuh keeps a witness word: gnark's Montgomery form (x 2^256 mod r), eight
// words, CANONICAL -- what the Fr transform reads and writes and what r1cs_acc_term takes in the witness's place.  What leaves is
// in REGULAR form, canonical: the scalars zklc_bn254_g{1,2}_fixed_mul_dev reads.  One multiplier serves both: fr_mul divides by
// 2^260, so (16 a 2^256) (b 2^256) / 2^260 = a b 2^256 (Montgomery x Montgomery -> Montgomery) and (16 a 2^256) b / 2^260 = a b
// (Montgomery x regular -> regular: the conversion on the way out costs no multiplication of its own where a constant is due
// anyway).  Every stored value is exact and canonical, so the order of a column's terms and the split over lanes are invisible.
#pragma once
#include "r1cs_eval.cuh"

// a column of more terms is cut into segments of this many, one wave each (the constant wire can occur in every constraint)
#define SETUP_SEG_TERMS 2048u
// consecutive exponents per lane of the powers kernel
#define SETUP_RUN 32u
#define SETUP_MAX_LOG 28u                    // the 2-adicity of Fr
#define SETUP_MAX_WIRES (1ull << 30)         // a column key (3 n_wires of them) fits u32; the point stage takes at most 2^30 scalars
// rounds in which the lanes of a wave that share the first open lane's column are counted by one atomic
#define SETUP_AGG_ROUNDS 4u

// what the host prepares from the toxic waste, once per call (passed to the kernels by value)
struct alignas(16) setup_consts {
    u32 tau_pow[SETUP_MAX_LOG + 1][8];   // tau^(2^k), Montgomery (k = log2 n: tau^n)
    u32 zt[8];                       // (tau^n - 1) / delta, REGULAR
    u32 beta[8], alpha[8];           // Montgomery
    u32 ginv[8], dinv[8];            // 1 / gamma, 1 / delta, REGULAR
};

// a b: Montgomery x Montgomery -> Montgomery, or Montgomery x regular -> regular; canonical
ZKLC_HD r1cs_el setup_mul(const u32 *a, const u32 *b) {
    r1cs_el r;
    fr_freeze_words(r.w, fr_mul(fr_from_gnark(a), fr_from_words_raw(b)));
    return r;
}
// eight words from a place that is only word-aligned (the caller's toxic words, a field of setup_consts, a constant on the stack):
// r1cs_load moves 16 bytes at a time and is for the 16-byte aligned arrays alone
ZKLC_HD r1cs_el setup_load(const u32 *p) {
    r1cs_el r;
    for (int i = 0; i < 8; i++) r.w[i] = p[i];
    return r;
}
// regular form (any value below 2^256: reduced) -> Montgomery, canonical; r1cs_witness_to_mont for a word-aligned source
ZKLC_HD r1cs_el setup_to_mont(const u32 *regular) {
    const fr k = R1CS_2P516;
    r1cs_el r;
    fr_freeze_words(r.w, fr_mul(fr_from_words_raw(regular), k));
    return r;
}
ZKLC_HD r1cs_el setup_one() {
    const u32 one[8] = R1CS_ONE_WORDS;
    r1cs_el r;
    for (int i = 0; i < 8; i++) r.w[i] = one[i];
    return r;
}
ZKLC_HD r1cs_el setup_to_regular(const u32 *a) {
    const u32 one_raw[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    return setup_mul(a, one_raw);
}
ZKLC_HD u32 setup_is_zero(const u32 *a) {
    u32 o = 0;
    for (int i = 0; i < 8; i++) o |= a[i];
    return o == 0;
}
// 1 / a, Montgomery -> Montgomery (a != 0)
ZKLC_HD r1cs_el setup_inv(const u32 *a) {
    r1cs_el r;
    fr_to_gnark(r.w, fr_inv(fr_reduce(fr_from_gnark(a))));
    return r;
}

// exponents [run SETUP_RUN, (run + 1) SETUP_RUN) below n: the first power from the table of tau^(2^k), the rest by one
// multiplication each.  pw[e] = tau^e (Montgomery: the input of the inverse transform); z[e] = tau^e (tau^n - 1) / delta for
// e < n - 1, regular form
ZKLC_HD void setup_powers_lane(const setup_consts &c, u64 n, u64 run, u32 *pw, u32 *z) {
    const u64 e0 = run * SETUP_RUN;
    if (e0 >= n) return;
    const u64 end = e0 + SETUP_RUN < n ? e0 + SETUP_RUN : n;
    r1cs_el p = setup_one();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 k = 0; k < SETUP_MAX_LOG; k++)
        if ((e0 >> k) & 1) p = setup_mul(p.w, c.tau_pow[k]);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u64 e = e0; e < end; e++) {
        r1cs_store(pw + 8 * e, p);
        if (e + 1 < n) r1cs_store(z + 8 * e, setup_mul(p.w, c.zt));
        if (e + 1 < end) p = setup_mul(p.w, c.tau_pow[0]);
    }
}

// the transposed index: a column is (matrix, wire), key = matrix n_wires + wire; its terms keep coefficient id and class and carry
// the constraint index where the wire was (it fits: n_constraints <= 2^30)
ZKLC_HD u64 setup_key(u64 matrix, u64 n_wires, u64 term) { return matrix * n_wires + (u32)term; }
ZKLC_HD u64 setup_transposed_term(u64 term, u32 constraint) { return (term & 0xffffffff00000000ull) | constraint; }
// columns of at most R1CS_BIN0_MAX terms: one lane; of at most R1CS_BIN1_MAX: eight; of at most SETUP_SEG_TERMS: a wave; longer
// ones: a wave per segment and a second pass over the partial sums
ZKLC_HD u32 setup_bin_of(u64 len) { return len <= R1CS_BIN0_MAX ? 0u : len <= R1CS_BIN1_MAX ? 1u : len <= SETUP_SEG_TERMS ? 2u : 3u; }
ZKLC_HD u64 setup_segments(u64 len) { return (len + SETUP_SEG_TERMS - 1) / SETUP_SEG_TERMS; }

// one wire: abc_t = a_t, b_t, c_t (n_wires x 8 words each, Montgomery) -> a_t, b_t, k in regular form
ZKLC_HD void setup_combine_lane(const setup_consts &c, u64 i, u64 n_wires, u32 n_public, const u32 *abc_t, u32 *a_t, u32 *b_t, u32 *k) {
    const r1cs_el a = r1cs_load(abc_t + 8 * i), b = r1cs_load(abc_t + 8 * (n_wires + i)), cc = r1cs_load(abc_t + 8 * (2 * n_wires + i));
    // beta a + alpha b + c: two products below 1.2 r and a canonical word, made canonical together
    const fr g = fr_add(fr_add(fr_mul(fr_from_gnark(c.beta), fr_from_words_raw(a.w)), fr_mul(fr_from_gnark(c.alpha), fr_from_words_raw(b.w))),
                        fr_from_words_raw(cc.w));
    r1cs_el s;
    fr_freeze_words(s.w, g);
    r1cs_store(k + 8 * i, setup_mul(s.w, i <= n_public ? c.ginv : c.dinv));
    r1cs_store(a_t + 8 * i, setup_to_regular(a.w));
    r1cs_store(b_t + 8 * i, setup_to_regular(b.w));
}

// ---- host side (groth16_setup_host.cpp, g++; the kernels' file calls them too: its own host code cannot run the lane functions) ----
// the arguments every entry shares: ZKLC_OK or ZKLC_ERR_INVALID_ARG; *log_n = log2 n
int32_t setup_check_sizes(const zklc_r1cs *s, uint32_t n_public, uint64_t n, uint32_t *log_n);
// toxic: 5 x 4 u64, regular form, 8-byte aligned (read word by word), any value below 2^256 (reduced here).  false: gamma or delta
// is 0 mod r
bool setup_prepare(const uint64_t *toxic, uint32_t log_n, setup_consts *c);
// overwrites a buffer that held a function of the toxic waste (not optimised away)
void setup_wipe(void *p, size_t bytes);
