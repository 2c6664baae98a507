// Generic 254-bit Montgomery field on ten signed 26-bit limbs (R' = 2^260); included by
// bn254_fp.cuh (base field) and bn254_fr.cuh (scalar field) with these macros defined:
//   MONT_T            element type (struct { i32 v[10]; })
//   MONT_FN(name)     function-name prefixing macro
//   MONT_P26          modulus limbs, MONT_PINV26 = -m^-1 mod 2^26, MONT_PM2_WORDS = m - 2 (8 x u32)
//   MONT_ONE          1 and MONT_2P256 = 2^256 in the internal domain (x * 2^260 mod m)
// See bn254_fp.cuh for the representation and its bounds.
#define MONT_MASK26 0x3ffffff

ZKLC_HD MONT_T MONT_FN(zero)() {
    MONT_T r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = 0;
    return r;
}
// Limb additions are done on the UNSIGNED type (same bits, the lazy bounds keep the true values far from overflow): a signed
// `a + b` carries "no signed wrap", which lets the compiler turn sext(a + b) into sext(a) + sext(b) -- and a product
// (i64)(a + b) * c then stops being the sext(i32) x sext(i32) pattern of ONE v_mad_i64_i32: it is lowered as a generic 64 x 64-bit
// multiplication (v_mad_u64_u32 + 2 v_mul_lo_u32 + v_add3_u32, measured: 4 100 instead of ~3 000 instructions per mixed addition).
#define MONT_WRAP(expr) ((i32)(expr))
// The same for the multiplier's operands: the compiler tracks value ranges through the carry normalisation of a product and
// drops the i64 -> i32 -> i64 round trip of a limb it can prove small -- the operand of the next multiplication is then a genuine
// 64-bit value and the product is lowered as a generic 64 x 64-bit multiplication again.  An empty asm makes the 32-bit limb
// opaque, so that every partial product stays sext(i32) x sext(i32) = one v_mad_i64_i32.
#if defined(__HIP_DEVICE_COMPILE__)
#define MONT_OPAQUE(x) asm("" : "+v"(x))
#else
#define MONT_OPAQUE(x) (void)0
#endif
ZKLC_HD MONT_T MONT_FN(add)(const MONT_T &a, const MONT_T &b) {
    MONT_T r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = MONT_WRAP((u32)a.v[i] + (u32)b.v[i]);
    return r;
}
ZKLC_HD MONT_T MONT_FN(sub)(const MONT_T &a, const MONT_T &b) {
    MONT_T r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = MONT_WRAP((u32)a.v[i] - (u32)b.v[i]);
    return r;
}
ZKLC_HD MONT_T MONT_FN(neg)(const MONT_T &a) {
    MONT_T r;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = MONT_WRAP(0u - (u32)a.v[i]);
    return r;
}
ZKLC_HD MONT_T MONT_FN(dbl)(const MONT_T &a) { return MONT_FN(add)(a, a); }
ZKLC_HD MONT_T MONT_FN(select)(const MONT_T &a, const MONT_T &b, u32 cond) {
    MONT_T r;
    i32 m = -(i32)cond;
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] = (b.v[i] & m) | (a.v[i] & ~m);
    return r;
}

// Montgomery reduction of 19 signed columns (value = sum t[k] 2^(26k)) -> value / 2^260 mod p
ZKLC_HD MONT_T MONT_FN(mont_reduce)(i64 *t) {
    const i32 P[10] = MONT_P26;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        i32 m = (i32)(((u32)t[i] * (u32)MONT_PINV26) & MONT_MASK26);  // quotient digit in [0, 2^26)
#pragma unroll
        for (int j = 0; j < 10; j++) t[i + j] += (i64)m * P[j];
        t[i + 1] += t[i] >> 26;  // exact: t[i] is now a multiple of 2^26
    }
    // carry-normalise t[10..19] into ten limbs (centred, top limb takes the rest)
    MONT_T r;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        i64 c = (t[10 + j] + ((i64)1 << 25)) >> 26;
        t[11 + j] += c;
        r.v[j] = (i32)(t[10 + j] - (i64)((u64)c << 26));   // (shifted as unsigned: c may be negative)
    }
    r.v[9] = (i32)t[19];
    return r;
}

ZKLC_HD MONT_T MONT_FN(mul)(const MONT_T &a_in, const MONT_T &b_in) {
    MONT_T a = a_in, b = b_in;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        MONT_OPAQUE(a.v[i]);
        MONT_OPAQUE(b.v[i]);
    }
    i64 t[20];
#pragma unroll
    for (int k = 0; k < 19; k++) {
        i64 acc = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            int j = k - i;
            if (j >= 0 && j < 10) acc += (i64)a.v[i] * b.v[j];
        }
        t[k] = acc;
    }
    t[19] = 0;
    return MONT_FN(mont_reduce)(t);
}

ZKLC_HD MONT_T MONT_FN(sqr)(const MONT_T &a_in) {
    MONT_T a = a_in;
    i32 a2[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        MONT_OPAQUE(a.v[i]);
        a2[i] = MONT_WRAP((u32)a.v[i] << 1);
        MONT_OPAQUE(a2[i]);
    }
    i64 t[20];
#pragma unroll
    for (int k = 0; k < 19; k++) {
        i64 acc = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            int j = k - i;
            if (j < i || j >= 10) continue;
            acc += (i64)(i == j ? a.v[i] : a2[i]) * a.v[j];
        }
        t[k] = acc;
    }
    t[19] = 0;
    return MONT_FN(mont_reduce)(t);
}

// Sums of products with ONE reduction: t (19 columns + t[19]) accumulates the columns of several products a_k * b_k;
// acc_reduce = (sum a_k b_k) / 2^260.  For operands with limbs below 2^27 (outputs of mul / reduce, table constants, one lazy
// addition of them) a column holds four products (10 * 2^54 each) and the reduction's own 2^55 below 2^63; the result of four
// products is below 1.2 m.  A dot product of four terms costs 400 + ~195 instructions instead of 4 * 294 + a multiplication by one.
ZKLC_HD void MONT_FN(acc_zero)(i64 *t) {
#pragma unroll
    for (int k = 0; k < 20; k++) t[k] = 0;
}
ZKLC_HD void MONT_FN(acc_mul)(i64 *t, const MONT_T &a_in, const MONT_T &b_in) {
    MONT_T a = a_in, b = b_in;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        MONT_OPAQUE(a.v[i]);
        MONT_OPAQUE(b.v[i]);
    }
#pragma unroll
    for (int k = 0; k < 19; k++) {
        i64 acc = t[k];
#pragma unroll
        for (int i = 0; i < 10; i++) {
            int j = k - i;
            if (j >= 0 && j < 10) acc += (i64)a.v[i] * b.v[j];
        }
        t[k] = acc;
    }
}
ZKLC_HD MONT_T MONT_FN(acc_reduce)(i64 *t) { return MONT_FN(mont_reduce)(t); }

// canonical value in [0, p) as 8 little-endian u32 words (still in the internal Montgomery domain)
ZKLC_HD void MONT_FN(freeze_words)(u32 *out, const MONT_T &a) {
    const i32 P[10] = MONT_P26;
    // v + 16p is positive for every legal lazy element (|v| < 16p); propagate to limbs in [0, 2^26)
    i64 l[10];
    i64 c = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        c += (i64)a.v[i] + 16 * (i64)P[i];
        l[i] = c & MONT_MASK26;
        c >>= 26;
    }
    l[9] += c << 26;  // value < 32p < 2^259: the top limb absorbs what is left
    // subtract 16p, 8p, 4p, 2p, p while the value stays non-negative
#pragma unroll
    for (int k = 4; k >= 0; k--) {
        i64 d[10];
        i64 borrow = 0;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            i64 x = l[i] - ((i64)P[i] << k) + borrow;
            if (i < 9) {
                d[i] = x & MONT_MASK26;
                borrow = x >> 26;
            } else {
                d[i] = x;
            }
        }
        bool neg = d[9] < 0;
#pragma unroll
        for (int i = 0; i < 10; i++) l[i] = neg ? l[i] : d[i];
    }
    // pack 10 x 26 bits (value < p < 2^254) into 8 words
    u64 acc = 0;
    int bits = 0, w = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        acc |= (u64)l[i] << bits;
        bits += 26;
        if (bits >= 32) {
            out[w++] = (u32)acc;
            acc >>= 32;
            bits -= 32;
        }
    }
    if (w < 8) out[w] = (u32)acc;
}

// 8 little-endian words (any value < 2^256) -> limbs of that integer
ZKLC_HD MONT_T MONT_FN(from_words_raw)(const u32 *w) {
    MONT_T r;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        int bit = 26 * i, wi = bit >> 5, sh = bit & 31;
        u64 x = (u64)w[wi] >> sh;
        if (wi + 1 < 8) x |= (u64)w[wi + 1] << (32 - sh);
        r.v[i] = (i32)(x & MONT_MASK26);
    }
    return r;
}

// gnark-crypto Montgomery form (x * 2^256 mod p, 4 x u64 little-endian = 8 words) -> internal.
// The result is the LAZY integer 16 * (x * 2^256) (< 16p, limbs < 2^30): legal only as a direct
// operand of MONT_FN(mul) / MONT_FN(sqr); pass it through MONT_FN(reduce) before adding or freezing.
ZKLC_HD MONT_T MONT_FN(from_gnark)(const u32 *w) {
    MONT_T r = MONT_FN(from_words_raw)(w);
#pragma unroll
    for (int i = 0; i < 10; i++) r.v[i] <<= 4;  // x * 2^260 as the lazy integer 16 * (x * 2^256)
    return r;
}
// internal -> gnark-crypto Montgomery form, canonical
ZKLC_HD void MONT_FN(to_gnark)(u32 *out, const MONT_T &a) {
    const MONT_T c = MONT_2P256;
    MONT_FN(freeze_words)(out, MONT_FN(mul)(a, c));
}

// same element, |value| < 1.2 p, limbs <= 2^25
ZKLC_HD MONT_T MONT_FN(reduce)(const MONT_T &a) {
    const MONT_T one = MONT_ONE;
    return MONT_FN(mul)(a, one);
}

ZKLC_HD u32 MONT_FN(is_zero)(const MONT_T &a) {
    // a legal lazy element congruent to zero is the INTEGER k m with |k| <= 15, so k = a_0 * m^-1 mod 2^26 must be a small signed
    // number: four instructions reject all but 31 / 2^26 of the non-zero elements; the exact test runs only for the candidates
    // (the curve additions test a difference for zero on every call: the canonicalisation below was ~20 % of a mixed addition)
    const u32 minv = (0u - (u32)MONT_PINV26) & MONT_MASK26;
    u32 kk = ((u32)a.v[0] * minv) & MONT_MASK26;
    if (((kk + 15u) & MONT_MASK26) > 30u) return 0;
    u32 w[8];
    MONT_FN(freeze_words)(w, a);
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= w[i];
    return o == 0;
}

// a^(p-2) (used once per MSM for the affine output, never in the bucket loops)
ZKLC_HD MONT_T MONT_FN(inv)(const MONT_T &a) {
    // p - 2, little-endian 32-bit words
    const u32 E[8] = MONT_PM2_WORDS;
    const MONT_T one = MONT_ONE;
    MONT_T r = one, x = a;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 0; i < 254; i++) {
        if ((E[i >> 5] >> (i & 31)) & 1) r = MONT_FN(mul)(r, x);
        x = MONT_FN(sqr)(x);
    }
    return r;
}

#undef MONT_MASK26
#undef MONT_WRAP
#undef MONT_OPAQUE
