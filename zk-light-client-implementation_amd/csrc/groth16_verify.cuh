// Groth16 verification over BN254, the lane functions: decoding and validation of a proof's points, the public-input fold over
// a fixed-base table of the key, and the pairing product.  Shared by the kernels of groth16_verify.hip and by the host path of
// groth16_verifier_host.cpp (g++), so both give the same status for every proof by construction.
//
// Replaces `groth16.Verify` (gnark-plonky2-verifier/cmd/web-api.go:84; gnark v0.9.1 backend/groth16/bn254/verify.go, un-vendored)
// together with the decoding in front of it (`proof.ReadFrom` / the head of `verifyCompressedProof`,
// contracts/hardhat/contracts/Verifier.sol:427-449).  Oracle: oracle/bn254.py, oracle/groth16.py, zklc_amd/formats.py.
//
// Work per proof and where it runs (kernel g16_prepare_kernel: one 128-lane workgroup per proof):
//   lane 64       decode (big-endian words, `>= p` on the bytes; compressed form: an Fp square root for A and C, an Fp2 square
//                 root for B), A / C / B on their curves, B in the r-torsion subgroup (g16_g2_in_subgroup)
//   lanes 0..63   kSum = K[0] + sum_i x_i K[i + 1]: lane j folds the inputs j, j + 64, ... with 64 table additions each (4-bit
//                 windows of the 256-bit scalar, table rows d 16^w K[i + 1], d = 1..15: no doublings), partial sums are added
//                 through LDS, lane 0 adds K[0] and leaves the affine point
// The pairing product runs on the g1 / g2 arrays this leaves (bn254_pairing.hip; g16_pairing_is_one on the host).
#pragma once
#include "bn254_ec.cuh"
#include "bn254_pairing.cuh"

#if defined(__HIPCC__)
#define G16_FN __device__ __noinline__
#else
#define G16_FN static
#endif

#define G16_OK 0u
#define G16_BAD_ENCODING 1u
#define G16_INFINITY 2u
#define G16_NOT_ON_CURVE 3u
#define G16_NOT_IN_SUBGROUP 4u
#define G16_PAIRING 5u

#define G16_WINDOWS 64u       // 4-bit windows of a 256-bit scalar (no reduction modulo r needed: the bases have order r)
#define G16_ROW 15u           // d = 1..15
#define G16_FOLD_LANES 64u

typedef ec_xyzz<FpField> g16_g1;
typedef ec_xyzz<Fp2Field> g16_g2;

struct g16_tab_entry {        // d 16^w K[i + 1], affine, internal Montgomery limbs (reduced)
    fp x, y;
};
struct g16_key {
    u32 n_public, k0_inf;
    fp k0x, k0y;              // K[0]
    fp2 twist_b;              // 3 / (9 + u)
    fp half;                  // 1 / 2
    u32 alpha[16];            // gnark words, as the pairing kernel reads them
    u32 neg_g2[3][32];        // -delta, -gamma, -beta
};

// ---------------------------------------------------------------- decoding
// 32 big-endian bytes -> 8 little-endian words
ZKLC_HD void g16_be_words(u32 *w, const uint8_t *b) {
    for (int i = 0; i < 8; i++) {
        const uint8_t *q = b + 28 - 4 * i;
        w[i] = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | (u32)q[3];
    }
}
ZKLC_HD u32 g16_words_zero(const u32 *w) {
    u32 o = 0;
    for (int i = 0; i < 8; i++) o |= w[i];
    return o == 0;
}
// value >= p
ZKLC_HD u32 g16_words_ge_p(const u32 *w) {
    const u32 Pw[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    for (int i = 7; i >= 0; i--) {
        if (w[i] > Pw[i]) return 1;
        if (w[i] < Pw[i]) return 0;
    }
    return 1;
}
ZKLC_HD void g16_words_shr(u32 *w, int s) {   // s = 1 or 2
    for (int i = 0; i < 8; i++) w[i] = (w[i] >> s) | (i < 7 ? w[i + 1] << (32 - s) : 0u);
}
// the integer of 8 words (< 2^256) -> the element, |value| < 1.5 p
ZKLC_HD fp g16_fp_from_words(const u32 *w) {
    const fp r2 = FP_R2;      // 2^520 mod p: raw * 2^520 / 2^260 = raw * 2^260
    return fp_mul(fp_from_words_raw(w), r2);
}
ZKLC_HD u32 g16_fp_eq(const fp &a, const fp &b) { return fp_is_zero(fp_sub(a, b)); }

// a^((p + 1) / 4): the square root of a square (p = 3 mod 4), the root `pow(a, (p + 1) / 4, p)` of zklc_amd/formats.py
G16_FN fp g16_fp_sqrt_candidate(const fp &a) {
    const u32 E[8] = {0xb61f3f52u, 0x4f082305u, 0x5a1c72a3u, 0x65e05aa4u, 0xa0605617u, 0x6e14116du, 0xb84c680au, 0x0c19139cu};
    const fp one = FP_ONE;
    fp r = one, x = a;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 0; i < 252; i++) {
        if ((E[i >> 5] >> (i & 31)) & 1) r = fp_mul(r, x);
        x = fp_sqr(x);
    }
    return r;
}
G16_FN fp g16_fp_inv(const fp &a) { return fp_inv(a); }

ZKLC_HD u32 g16_g1_on_curve(const fp &x, const fp &y) {
    const fp three = FP_THREE;
    return fp_is_zero(fp_sub(fp_sub(fp_sqr(y), fp_mul(fp_sqr(x), x)), three));
}
ZKLC_HD fp2 g16_g2_rhs(const g16_key &k, const fp2 &x) { return fp2_add(fp2_mul(fp2_sqr(x), x), k.twist_b); }
ZKLC_HD u32 g16_g2_on_curve(const g16_key &k, const fp2 &x, const fp2 &y) { return fp2_is_zero(fp2_sub(fp2_sqr(y), g16_g2_rhs(k, x))); }

// compressed G1 word (x << 1 | sign of y): formats.decompress_g1.  Returns the class of the first defect (G16_OK: x, y set)
ZKLC_HD u32 g16_decompress_g1(u32 *w, fp &x, fp &y) {
    if (g16_words_zero(w)) return G16_INFINITY;
    const u32 sign = w[0] & 1;
    g16_words_shr(w, 1);
    if (g16_words_ge_p(w)) return G16_BAD_ENCODING;
    const fp three = FP_THREE;
    x = g16_fp_from_words(w);
    fp rhs = fp_reduce(fp_add(fp_mul(fp_sqr(x), x), three));
    y = g16_fp_sqrt_candidate(rhs);
    if (!g16_fp_eq(fp_sqr(y), rhs)) return G16_NOT_ON_CURVE;   // x has no y
    if (sign) y = fp_neg(y);
    return G16_OK;
}
// compressed G2 words c0 = x0 << 2 | hint << 1 | sign, c1 = x1: formats.decompress_g2 / _sqrt_fp2.  x^3 + b' not a square of Fp2
// (its norm is not a square of Fp): G16_NOT_ON_CURVE.  The norm is a square but the root the hint bit selects does not exist, or
// the root's real part is zero (no inverse): the word is malformed, G16_BAD_ENCODING.
ZKLC_HD u32 g16_decompress_g2(const g16_key &k, u32 *c0, const u32 *c1, fp2 &x, fp2 &y) {
    if (g16_words_zero(c0) && g16_words_zero(c1)) return G16_INFINITY;
    const u32 sign = c0[0] & 1, hint = (c0[0] >> 1) & 1;
    g16_words_shr(c0, 2);
    if (g16_words_ge_p(c0) || g16_words_ge_p(c1)) return G16_BAD_ENCODING;
    x.c0 = g16_fp_from_words(c0);
    x.c1 = g16_fp_from_words(c1);
    fp2 a = fp2_reduce(g16_g2_rhs(k, x));
    fp n = fp_reduce(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
    fp d = g16_fp_sqrt_candidate(n);
    if (!g16_fp_eq(fp_sqr(d), n)) return G16_NOT_ON_CURVE;
    if (hint) d = fp_neg(d);
    fp t = fp_mul(fp_add(a.c0, d), k.half);
    fp y0 = g16_fp_sqrt_candidate(t);
    if (!g16_fp_eq(fp_sqr(y0), t) || fp_is_zero(y0)) return G16_BAD_ENCODING;
    fp y1 = fp_mul(a.c1, g16_fp_inv(fp_dbl(y0)));
    y.c0 = y0;
    y.c1 = y1;
    if (!fp2_is_zero(fp2_sub(fp2_sqr(y), a))) return G16_NOT_ON_CURVE;
    if (sign) y = fp2_neg(y);
    return G16_OK;
}

// ---------------------------------------------------------------- G2 membership
// psi = twist o Frobenius o untwist on extended Jacobian coordinates: (x, y) -> (conj(x) gamma_1,2, conj(y) gamma_1,3), the pi(Q)
// of the Miller loop; x = X / ZZ, y = Y / ZZZ, so the denominators are conjugated only
ZKLC_HD g16_g2 g16_psi(const g16_g2 &p) {
    g16_g2 r;
    r.X = fp2_mul(fp2_conj(p.X), BN_GAMMA[1]);
    r.Y = fp2_mul(fp2_conj(p.Y), BN_GAMMA[2]);
    r.ZZ = fp2_conj(p.ZZ);
    r.ZZZ = fp2_conj(p.ZZZ);
    return r;
}
ZKLC_HD u32 g16_g2_eq(const g16_g2 &a, const g16_g2 &b) {
    u32 ai = ec_is_inf(a), bi = ec_is_inf(b);
    if (ai | bi) return ai & bi;
    return fp2_is_zero(fp2_sub(fp2_mul(a.X, b.ZZ), fp2_mul(b.X, a.ZZ))) & fp2_is_zero(fp2_sub(fp2_mul(a.Y, b.ZZZ), fp2_mul(b.Y, a.ZZZ)));
}
// Q = (x, y) on the twist (reduced): Q in G2  <=>  [x + 1] Q + psi([x] Q) + psi^2([x] Q) = psi^3([2 x] Q), x the BN parameter
// (Dai, Lin, Zhao, Zhou: "Fast subgroup membership testings for G1, G2 and GT on pairing-friendly curves", eprint 2022/348
// -- exact for BN curves): one 63-bit multiplication (61 doublings, 27 mixed additions) instead of the 254 doublings of
// [r] Q = O.
G16_FN u32 g16_g2_in_subgroup(const fp2 &x, const fp2 &y) {
    const u64 X = 0x44E992B44A6909F1ULL;
    g16_g2 q;
    q.X = x;
    q.Y = y;
    q.ZZ = fp2_one();
    q.ZZZ = fp2_one();
    g16_g2 xq = q;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 61; i >= 0; i--) {
        xq = ec_double<Fp2Field>(xq);
        if ((X >> i) & 1) xq = ec_add_affine<Fp2Field>(xq, x, y, 0);
    }
    g16_g2 p1 = g16_psi(xq), p2 = g16_psi(p1);
    g16_g2 lhs = ec_add<Fp2Field>(ec_add<Fp2Field>(ec_add_affine<Fp2Field>(xq, x, y, 0), p1), p2);
    g16_g2 rhs = g16_psi(g16_psi(g16_psi(ec_double<Fp2Field>(xq))));
    return g16_g2_eq(lhs, rhs);
}

// ---------------------------------------------------------------- one proof: decode + validate
// proof: 256 bytes (A.x, A.y, B.x1, B.x0, B.y1, B.y0, C.x, C.y) or, compressed, 128 bytes (A, B.c1, B.c0, C).  Returns the first
// failing class in the order BAD_ENCODING, INFINITY, NOT_ON_CURVE (A, C, B), NOT_IN_SUBGROUP; writes A, C (16 words each) and B
// (32 words) in gnark's layout, zeros for a rejected proof.
G16_FN u32 g16_validate_lane(const g16_key &k, const uint8_t *proof, u32 compressed, u32 *out_a, u32 *out_c, u32 *out_b) {
    fp ax, ay, cx, cy;
    fp2 bx, by;
    u32 st = G16_OK;
    ax = ay = cx = cy = fp_zero();
    bx = by = fp2_zero();
    if (compressed) {
        u32 wa[8], wb1[8], wb0[8], wc[8];
        g16_be_words(wa, proof);
        g16_be_words(wb1, proof + 32);
        g16_be_words(wb0, proof + 64);
        g16_be_words(wc, proof + 96);
        // the classes of the three points, then the first class in the documented order (a curve defect of A before one of C, of B)
        u32 sa = g16_decompress_g1(wa, ax, ay);
        u32 sc = g16_decompress_g1(wc, cx, cy);
        u32 sb = g16_decompress_g2(k, wb0, wb1, bx, by);
        for (u32 cls = G16_BAD_ENCODING; cls <= G16_NOT_ON_CURVE && st == G16_OK; cls++)
            if (sa == cls || sc == cls || sb == cls) st = cls;
    } else {
        u32 w[8][8], ge = 0, za = 1, zb = 1, zc = 1;
        for (int i = 0; i < 8; i++) {
            g16_be_words(w[i], proof + 32 * i);
            ge |= g16_words_ge_p(w[i]);
            u32 z = g16_words_zero(w[i]);
            if (i < 2) za &= z;
            else if (i < 6) zb &= z;
            else zc &= z;
        }
        if (ge) st = G16_BAD_ENCODING;
        else if (za | zb | zc) st = G16_INFINITY;
        else {
            ax = g16_fp_from_words(w[0]);
            ay = g16_fp_from_words(w[1]);
            bx.c1 = g16_fp_from_words(w[2]);
            bx.c0 = g16_fp_from_words(w[3]);
            by.c1 = g16_fp_from_words(w[4]);
            by.c0 = g16_fp_from_words(w[5]);
            cx = g16_fp_from_words(w[6]);
            cy = g16_fp_from_words(w[7]);
            if (!g16_g1_on_curve(ax, ay) || !g16_g1_on_curve(cx, cy) || !g16_g2_on_curve(k, bx, by)) st = G16_NOT_ON_CURVE;
        }
    }
    if (st == G16_OK && !g16_g2_in_subgroup(bx, by)) st = G16_NOT_IN_SUBGROUP;
    if (st != G16_OK) {
        for (int i = 0; i < 16; i++) out_a[i] = out_c[i] = 0;
        for (int i = 0; i < 32; i++) out_b[i] = 0;
        return st;
    }
    fp_to_gnark(out_a, ax);
    fp_to_gnark(out_a + 8, ay);
    fp_to_gnark(out_c, cx);
    fp_to_gnark(out_c + 8, cy);
    fp2_to_gnark(out_b, bx);
    fp2_to_gnark(out_b + 16, by);
    return G16_OK;
}

// ---------------------------------------------------------------- the public-input fold
// the partial sum of the inputs lane, lane + stride, ...: sum_i sum_w T[i][w][digit_w(x_i)], 64 mixed additions per input.
// inputs: n_public x 4 u64 (regular form, any 256-bit value: the bases have order r); k_inf[i + 1] = 1: K[i + 1] is the point at infinity
ZKLC_HD g16_g1 g16_fold_lane(const g16_tab_entry *tab, const uint8_t *k_inf, const u64 *inputs, u32 n_public, u32 lane, u32 stride) {
    g16_g1 acc = ec_infinity<FpField>();
    for (u32 i = lane; i < n_public; i += stride) {
        if (k_inf[i + 1]) continue;
        const g16_tab_entry *row = tab + (size_t)i * G16_WINDOWS * G16_ROW;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (u32 w = 0; w < G16_WINDOWS; w++) {
            const u32 d = (u32)(inputs[4 * (size_t)i + (w >> 4)] >> (4 * (w & 15))) & 15u;
            if (!d) continue;
            const g16_tab_entry &e = row[w * G16_ROW + d - 1];
            acc = ec_add_affine<FpField>(acc, e.x, e.y, 0);
        }
    }
    return acc;
}
// kSum = K[0] + sum -> 16 gnark words (zeros: the point at infinity)
ZKLC_HD void g16_fold_finish(const g16_key &k, const g16_g1 &sum, u32 *out) {
    g16_g1 t = sum;
    if (!k.k0_inf) t = ec_add_affine<FpField>(t, k.k0x, k.k0y, 0);
    (void)ec_to_affine_gnark<FpField>(out, t);
}

// ---------------------------------------------------------------- the pairing product (host path; the kernels of bn254_pairing.hip on the GPU)
// g1: 4 x 16 words, g2: 4 x 32 words as bn254_pairing_check_kernel reads them
ZKLC_HD u32 g16_pairing_is_one(const u32 *g1, const u32 *g2) {
    fp12 f = f12_one();
    for (u32 i = 0; i < 4; i++) {
        const u32 *p = g1 + 16 * i, *q = g2 + 32 * i;
        u32 z1 = 0, z2 = 0;
        for (int j = 0; j < 16; j++) z1 |= p[j];
        for (int j = 0; j < 32; j++) z2 |= q[j];
        if (!z1 || !z2) continue;
        fp xp = fp_reduce(fp_from_gnark(p)), yp = fp_reduce(fp_from_gnark(p + 8));
        fp2 xq = fp2_reduce(fp2_from_gnark(q)), yq = fp2_reduce(fp2_from_gnark(q + 16));
        bn_miller_loop(f, xp, yp, xq, yq);
    }
    return f12_is_one(bn_final_exponentiation(f));
}
