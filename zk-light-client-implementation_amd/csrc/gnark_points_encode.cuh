// gnark-crypto's own point encoding for BN254, the writing direction (ecc/bn254/marshal.go, un-vendored: `G1Affine.RawBytes` /
// `Bytes`, `G2Affine.RawBytes` / `Bytes`, the encoders behind `pk.WriteRawTo` / `pk.WriteTo` of
// gnark-plonky2-verifier/verifier/util.go:172-216), the lane functions: one point of a key in gnark-crypto's memory layout (the
// Montgomery words the multi-exponentiations read and groth16.Setup leaves) -> a class and its fixed-stride slot of a key file's
// point array.  The inverse of gnark_points.cuh, on the same field code; shared by the kernels of gnark_points_encode.hip and by
// the host path of gnark_points_encode_host.cpp (g++), so both write every slot alike by construction.  Specification:
// zklc_amd/gnark_keys.py write_g1 / write_g2 on words_to_points of the record.
//
//   in    16 (G1: X, Y) or 32 (G2: X.A0, X.A1, Y.A0, Y.A1) u32 words, each coordinate x 2^256 mod p as a canonical integer
//   out   the slot, 16-byte aligned, written by 16-byte stores:
//         raw G1 64 bytes X | Y, G2 128 bytes X.A1 | X.A0 | Y.A1 | Y.A0, flag 00; compressed G1 32 bytes X, G2 64 bytes X.A1 | X.A0,
//         flag 10 / 11 = y is the lexicographically smaller / larger root; 32-byte big-endian coordinates, the flag in the two top
//         bits of the first byte.  An all-zero record is the point at infinity: flag 01, zeros to the full stride.
// Classes (GK_*, the order of include/zklc.h): OK; INFINITY; BAD_ENCODING: a coordinate's eight words are >= p (gnark's memory form
// is canonical, so such a record is not a key's); NOT_ON_CURVE: only when the caller validates.  No subgroup test.  A rejected
// record's slot is all 0xFF: flag 11 in a raw array is a flag of the other encoding, and in a compressed one the x that follows it
// (2^254 - 1) is >= p, so every decoder of gnark_points.cuh classifies it BAD_ENCODING -- zeros would read back as infinity.
//
// Serial chain per point in Fp multiplications, read from the code below (unit as in gnark_points.cuh: one fp_mul / fp_sqr; fp2_mul
// counts 3, fp2_sqr 2).  A coordinate leaves the Montgomery domain by ONE multiplication (its lazy internal form, 16 w, times the
// integer 1: 16 w / 2^260 = w / 2^256), then fp_freeze_words; the compressed forms take the ordering of y from those frozen words.
//                   without validation                                with validation
//   G1 raw          x 1, y 1                                 = 2      + curve 3 (y^2, x^2, x^2 x: the lazy form is a legal operand)        = 5
//   G2 raw          x 2, y 2                                 = 4      + into reduced form 4 (fp2_sqr ADDS its operands: the lazy form
//                                                                       is not legal there) + curve 7 (y^2: 2, x^3: 2 + 3)            = 15
//   G1 compressed   x 1, y 1 (for the flag)                  = 2      + 3                                                             = 5
//   G2 compressed   x 2, y.A1 1, y.A0 1 only when y.A1 = 0   = 3 (4)  + 11                                                            = 14 (15)
// In G2 the curve equation comes AFTER the slot has been stored, and a failing record's slot is written a second time (0xFF): with
// the test in front, its Fp2 products and the words kept for the output held the kernels at 169 / 171 VGPRs, two waves per SIMD;
// this order needs 141 / 161, three waves, the occupancy of the decoder's raw G2 instance.
#pragma once
#include "gnark_points.cuh"

#define GK_FLAG_SMALLEST 2u

// a coordinate in its lazy internal form (fp_from_gnark) -> the canonical value's eight words: one multiplication
ZKLC_HD void gk_coord_out(u32 *cw, const fp &lazy) {
    const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    fp_freeze_words(cw, fp_mul(lazy, fp_from_words_raw(one)));
}
// eight canonical words -> 32 big-endian bytes at a 16-byte aligned address: bytes swapped in registers, two 16-byte stores.  flag:
// the two top bits of the first byte (the canonical value is below 2^254)
ZKLC_HD void gk_store_coord(uint8_t *b, const u32 *cw, u32 flag) {
    gk_q hi, lo;
    for (int i = 0; i < 4; i++) {
        hi.w[i] = __builtin_bswap32(cw[7 - i]);
        lo.w[i] = __builtin_bswap32(cw[3 - i]);
    }
    hi.w[0] |= flag << 6;
    reinterpret_cast<gk_q *>(b)[0] = hi;
    reinterpret_cast<gk_q *>(b)[1] = lo;
}
// nq x 16 bytes of one value; first: the first word (the flag byte of an infinity slot)
ZKLC_HD void gk_slot_fill(uint8_t *slot, int nq, u32 v, u32 first) {
    gk_q q;
    for (int j = 0; j < 4; j++) q.w[j] = v;
    for (int i = 1; i < nq; i++) reinterpret_cast<gk_q *>(slot)[i] = q;
    q.w[0] = first;
    reinterpret_cast<gk_q *>(slot)[0] = q;
}
ZKLC_HD u32 gk_record_zero(const u32 *w, int nw) {
    u32 o = 0;
    for (int i = 0; i < nw; i++) o |= w[i];
    return o == 0;
}

// One G1 point.  w: 16 words; slot: 64 bytes (raw) or 32 (COMPRESSED), 16-byte aligned, written in full whatever the class.
// Returns the first failing class.
template <u32 COMPRESSED>
ZKLC_HD u32 gk_g1_encode(const u32 *w, u32 validate, uint8_t *slot) {
    constexpr int NQ = COMPRESSED ? 2 : 4;
    u32 st = GK_OK;
    if (gk_record_zero(w, 16)) st = GK_INFINITY;
    else if (g16_words_ge_p(w) || g16_words_ge_p(w + 8)) st = GK_BAD_ENCODING;
    else if (validate && !g16_g1_on_curve(fp_from_gnark(w), fp_from_gnark(w + 8))) st = GK_NOT_ON_CURVE;
    if (st != GK_OK) {
        if (st == GK_INFINITY) gk_slot_fill(slot, NQ, 0, GK_FLAG_INFINITY << 6);
        else gk_slot_fill(slot, NQ, 0xffffffffu, 0xffffffffu);
        return st;
    }
    u32 c[8], flag = 0;
    gk_coord_out(c, fp_from_gnark(w + 8));
    if (COMPRESSED) flag = gk_words_lex_largest(c) ? GK_FLAG_LARGEST : GK_FLAG_SMALLEST;
    else gk_store_coord(slot + 32, c, 0);
    gk_coord_out(c, fp_from_gnark(w));
    gk_store_coord(slot, c, flag);
    return GK_OK;
}

// One G2 point, membership in the r-torsion subgroup not tested.  w: 32 words; slot: 128 bytes (raw) or 64 (COMPRESSED).  k: twist_b
// is read, and only when validate is set.
template <u32 COMPRESSED>
ZKLC_HD u32 gk_g2_encode(const g16_key &k, const u32 *w, u32 validate, uint8_t *slot) {
    constexpr int NQ = COMPRESSED ? 4 : 8;
    u32 st = GK_OK;
    if (gk_record_zero(w, 32)) st = GK_INFINITY;
    else if (g16_words_ge_p(w) || g16_words_ge_p(w + 8) || g16_words_ge_p(w + 16) || g16_words_ge_p(w + 24)) st = GK_BAD_ENCODING;
    if (st != GK_OK) {
        if (st == GK_INFINITY) gk_slot_fill(slot, NQ, 0, GK_FLAG_INFINITY << 6);
        else gk_slot_fill(slot, NQ, 0xffffffffu, 0xffffffffu);
        return st;
    }
    u32 c[8], flag = 0;
    gk_coord_out(c, fp_from_gnark(w + 24));                                  // Y.A1
    if (COMPRESSED) {
        if (g16_words_zero(c)) gk_coord_out(c, fp_from_gnark(w + 16));       // A1 = 0: A0 decides
        flag = gk_words_lex_largest(c) ? GK_FLAG_LARGEST : GK_FLAG_SMALLEST;
    } else {
        gk_store_coord(slot + 64, c, 0);
        gk_coord_out(c, fp_from_gnark(w + 16));
        gk_store_coord(slot + 96, c, 0);
    }
    gk_coord_out(c, fp_from_gnark(w + 8));                                   // X.A1 carries the flag
    gk_store_coord(slot, c, flag);
    gk_coord_out(c, fp_from_gnark(w));
    gk_store_coord(slot + 32, c, 0);
    // the curve equation LAST, the slot written over when it fails (a lane's stores to one address keep their order): the
    // products of an Fp2 multiplication (two accumulators of 20 columns) then do not meet the output words in the register file
    if (validate && !g16_g2_on_curve(k, fp2_reduce(fp2_from_gnark(w)), fp2_reduce(fp2_from_gnark(w + 16)))) {
        gk_slot_fill(slot, NQ, 0xffffffffu, 0xffffffffu);
        return GK_NOT_ON_CURVE;
    }
    return GK_OK;
}
