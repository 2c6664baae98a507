// gnark-crypto's own point encoding for BN254 (ecc/bn254/marshal.go, un-vendored: `G1Affine.SetBytes` / `G2Affine.SetBytes`, the
// decoders behind `pk.ReadFrom` of gnark-plonky2-verifier/verifier/util.go:337-389), the lane functions: one point of a key file's
// point array from its fixed-stride slot -> a class and the point in gnark-crypto's memory layout (the Montgomery words the
// multi-exponentiations read).  Shared by the kernels of gnark_points.hip and by the host path of gnark_points_host.cpp (g++), so
// both classify every point alike by construction.  Specification: zklc_amd/gnark_keys.py read_g1 / read_g2, down to their quirks.
//
//   raw (`WriteRawTo`)      G1 64 bytes: X | Y; G2 128 bytes: X.A1 | X.A0 | Y.A1 | Y.A0; 32-byte big-endian coordinates.  The two
//                           top bits of the first byte are 00, or 01 = infinity (the rest of the first coordinate zero; the
//                           padding behind it is not inspected).  An uncompressed (0, 0) is the point at infinity as well.
//   compressed (`WriteTo`)  G1 32 bytes: X; G2 64 bytes: X.A1 | X.A0; the flag is 10 (y is the lexicographically smaller root),
//                           11 (the larger one) or 01 (infinity).  Fp2 is ordered by A1, by A0 only when A1 = 0.
// This is NOT the contract's `compressProof` format of groth16_verify.cuh (sign and hint bits at the low end of the word).
//
// Serial chain per point in Fp multiplications, read from the code below (unit: one fp_mul / fp_sqr; fp2_mul counts 3, fp2_sqr 2;
// S = 361: a^((p + 1) / 4), 252 squarings + 109 set bits; I = 364: a^(p - 2), 254 + 110):
//   G1 raw          into the field 2, curve 3, out 2                                                                  =     7
//   G2 raw          into the field 4, curve 7 (y^2: 2, x^3: 2 + 3), out 4                                             =    15
//   G1 compressed   into the field 1, x^3 + 3 reduced 3, S, its check 1, order 1, out 2                               =   369
//   G2 compressed   into the field 2, x^3 + b' reduced 7, norm 3, S, check 1, h 1, S, I, t 1, checks 1 + 2, order 1,
//                   out 4                                                                                             = 1 109
//   G2 membership   reduce 4 + g16_g2_in_subgroup 2 418                                               = 2 422
#pragma once
#include "groth16_verify.cuh"

#define GK_OK 0u
#define GK_INFINITY 1u
#define GK_BAD_ENCODING 2u
#define GK_NOT_ON_CURVE 3u
#define GK_NOT_IN_SUBGROUP 4u

#define GK_FLAG_INFINITY 1u   // the two top bits of the first byte
#define GK_FLAG_LARGEST 3u

// 16 bytes of the file or of the output, moved by one access
struct __attribute__((aligned(16), may_alias)) gk_q {
    u32 w[4];
};

// one 32-byte big-endian coordinate at a 16-byte aligned address -> 8 little-endian words: two 16-byte loads, bytes swapped in registers
ZKLC_HD void gk_load_coord(u32 *w, const uint8_t *b) {
    const gk_q hi = *reinterpret_cast<const gk_q *>(b), lo = *reinterpret_cast<const gk_q *>(b + 16);
    for (int i = 0; i < 4; i++) {
        w[7 - i] = __builtin_bswap32(hi.w[i]);
        w[3 - i] = __builtin_bswap32(lo.w[i]);
    }
}
// nq x 16 bytes of words to a 16-byte aligned address
ZKLC_HD void gk_store_words(u32 *dst, const u32 *w, int nq) {
    for (int i = 0; i < nq; i++) {
        gk_q q;
        for (int j = 0; j < 4; j++) q.w[j] = w[4 * i + j];
        reinterpret_cast<gk_q *>(dst)[i] = q;
    }
}
ZKLC_HD void gk_load_words(u32 *w, const u32 *src, int nq) {
    for (int i = 0; i < nq; i++) {
        const gk_q q = reinterpret_cast<const gk_q *>(src)[i];
        for (int j = 0; j < 4; j++) w[4 * i + j] = q.w[j];
    }
}

// gnark-crypto fp.Element.LexicographicallyLargest: the canonical value is above (p - 1) / 2
// (on the canonical value's eight words: the encoder of gnark_points_encode.cuh has them already; then on an element)
ZKLC_HD u32 gk_words_lex_largest(const u32 *w) {
    const u32 H[8] = {0x6c3e7ea3u, 0x9e10460bu, 0xb438e546u, 0xcbc0b548u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
    for (int i = 7; i >= 0; i--) {
        if (w[i] > H[i]) return 1;
        if (w[i] < H[i]) return 0;
    }
    return 0;
}
ZKLC_HD u32 gk_fp_lex_largest(const fp &y) {
    const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    u32 w[8];
    fp_freeze_words(w, fp_mul(y, fp_from_words_raw(one)));   // out of the Montgomery domain
    return gk_words_lex_largest(w);
}
// E2.LexicographicallyLargest: A1 decides, A0 only when A1 = 0 (gnark_keys._g2_lex_largest)
ZKLC_HD u32 gk_fp2_lex_largest(const fp2 &y) { return fp_is_zero(y.c1) ? gk_fp_lex_largest(y.c0) : gk_fp_lex_largest(y.c1); }

// a square root of a (reduced) in Fp2 = Fp[u] / (u^2 + 1), without a hint bit: either root will do, the flag then chooses between y
// and -y.  Returns 0 when a is not a square.  a1 = 0: sqrt(a0), or u sqrt(-a0) when a0 is not a square (c = a0^((p + 1) / 4) squares
// to a0 or to -a0, p = 3 mod 4).  Otherwise d = sqrt(a0^2 + a1^2) and h = (a0 + d) / 2; h (a0 - d) / 2 = -a1^2 / 4 is not a square,
// so exactly one of the two is: with c = h^((p + 1) / 4) and t = a1 / (2 c) the root is c + t u when c^2 = h, and t + c u when
// c^2 = -h (then t^2 = (a0 - d) / 2) -- two exponentiations and one inversion whichever sign d has.
ZKLC_HD u32 gk_fp2_sqrt(const g16_key &k, const fp2 &a, fp2 &y) {
    if (fp_is_zero(a.c1)) {
        const fp c = g16_fp_sqrt_candidate(a.c0);
        const u32 real = g16_fp_eq(fp_sqr(c), a.c0);
        y.c0 = real ? c : fp_zero();
        y.c1 = real ? fp_zero() : c;
    } else {
        const fp n = fp_reduce(fp_add(fp_sqr(a.c0), fp_sqr(a.c1)));
        const fp d = g16_fp_sqrt_candidate(n);
        if (!g16_fp_eq(fp_sqr(d), n)) return 0;
        const fp h = fp_mul(fp_add(a.c0, d), k.half);
        const fp c = g16_fp_sqrt_candidate(h);
        const fp t = fp_mul(a.c1, g16_fp_inv(fp_dbl(c)));
        const u32 real = g16_fp_eq(fp_sqr(c), h);
        y.c0 = real ? c : t;
        y.c1 = real ? t : c;
    }
    return fp2_is_zero(fp2_sub(fp2_sqr(y), a));
}

// One G1 point.  slot: 64 bytes (raw) or 32 bytes (COMPRESSED), 16-byte aligned.  out: 16 words, gnark's layout; zeros unless the
// class is GK_OK.  Returns the first failing class in the order of include/zklc.h (ZKLC_POINT_*).
template <u32 COMPRESSED>
ZKLC_HD u32 gk_g1_decode(const uint8_t *slot, u32 *out) {
    for (int i = 0; i < 16; i++) out[i] = 0;
    u32 wx[8], wy[8];
    gk_load_coord(wx, slot);
    if (!COMPRESSED) gk_load_coord(wy, slot + 32);
    const u32 flag = wx[7] >> 30;
    wx[7] &= 0x3fffffffu;
    if (flag == GK_FLAG_INFINITY) return g16_words_zero(wx) ? GK_INFINITY : GK_BAD_ENCODING;
    if (COMPRESSED ? flag == 0 : flag != 0) return GK_BAD_ENCODING;          // a flag of the other encoding
    if (g16_words_ge_p(wx)) return GK_BAD_ENCODING;
    const fp x = g16_fp_from_words(wx);
    fp y;
    if (!COMPRESSED) {
        if (g16_words_ge_p(wy)) return GK_BAD_ENCODING;
        if (g16_words_zero(wx) && g16_words_zero(wy)) return GK_INFINITY;
        y = g16_fp_from_words(wy);
        if (!g16_g1_on_curve(x, y)) return GK_NOT_ON_CURVE;
    } else {
        const fp three = FP_THREE;
        const fp rhs = fp_reduce(fp_add(fp_mul(fp_sqr(x), x), three));
        y = g16_fp_sqrt_candidate(rhs);
        if (!g16_fp_eq(fp_sqr(y), rhs)) return GK_NOT_ON_CURVE;              // x has no y
        if (gk_fp_lex_largest(y) != (flag == GK_FLAG_LARGEST)) y = fp_neg(y);
    }
    fp_to_gnark(out, x);
    fp_to_gnark(out + 8, y);
    return GK_OK;
}

// One G2 point, membership in the r-torsion subgroup NOT tested (gk_g2_subgroup_lane).  slot: 128 bytes (raw) or 64 bytes
// (COMPRESSED); out: 32 words X.A0, X.A1, Y.A0, Y.A1.  k: twist_b and half are read.
template <u32 COMPRESSED>
ZKLC_HD u32 gk_g2_decode(const g16_key &k, const uint8_t *slot, u32 *out) {
    for (int i = 0; i < 32; i++) out[i] = 0;
    u32 wx1[8], wx0[8], wy1[8], wy0[8];
    gk_load_coord(wx1, slot);
    gk_load_coord(wx0, slot + 32);
    if (!COMPRESSED) {
        gk_load_coord(wy1, slot + 64);
        gk_load_coord(wy0, slot + 96);
    }
    const u32 flag = wx1[7] >> 30;
    wx1[7] &= 0x3fffffffu;
    if (flag == GK_FLAG_INFINITY) return g16_words_zero(wx1) && g16_words_zero(wx0) ? GK_INFINITY : GK_BAD_ENCODING;
    if (COMPRESSED ? flag == 0 : flag != 0) return GK_BAD_ENCODING;
    if (g16_words_ge_p(wx0) || g16_words_ge_p(wx1)) return GK_BAD_ENCODING;
    fp2 x, y;
    x.c0 = g16_fp_from_words(wx0);
    x.c1 = g16_fp_from_words(wx1);
    if (!COMPRESSED) {
        if (g16_words_ge_p(wy0) || g16_words_ge_p(wy1)) return GK_BAD_ENCODING;
        if (g16_words_zero(wx0) && g16_words_zero(wx1) && g16_words_zero(wy0) && g16_words_zero(wy1)) return GK_INFINITY;
        y.c0 = g16_fp_from_words(wy0);
        y.c1 = g16_fp_from_words(wy1);
        if (!g16_g2_on_curve(k, x, y)) return GK_NOT_ON_CURVE;
    } else {
        const fp2 rhs = fp2_reduce(g16_g2_rhs(k, x));
        if (!gk_fp2_sqrt(k, rhs, y)) return GK_NOT_ON_CURVE;                 // x has no y
        if (gk_fp2_lex_largest(y) != (flag == GK_FLAG_LARGEST)) y = fp2_neg(y);
    }
    fp2_to_gnark(out, x);
    fp2_to_gnark(out + 16, y);
    return GK_OK;
}

// The membership test of a decoded point (class GK_OK): words in / out, zeros when the point is on the twist but not of order r
ZKLC_HD u32 gk_g2_subgroup_lane(u32 *words) {
    const fp2 x = fp2_reduce(fp2_from_gnark(words)), y = fp2_reduce(fp2_from_gnark(words + 16));
    if (g16_g2_in_subgroup(x, y)) return GK_OK;
    for (int i = 0; i < 32; i++) words[i] = 0;
    return GK_NOT_IN_SUBGROUP;
}
