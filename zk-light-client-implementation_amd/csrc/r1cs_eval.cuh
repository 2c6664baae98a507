// The constraint system of `groth16.Prove(r1cs, pk, witness)` (gnark-plonky2-verifier/cmd/web-api.go:77): the per-constraint values
// a = A w, b = B w, c = C w that gnark's solver leaves behind (constraint/bn254/solver.go, un-vendored) and `computeH` transforms,
// from the solved witness.  The lane functions: one term, one row, one witness word.  Shared by the kernels of r1cs_eval.hip and by
// the host path of r1cs_eval_host.cpp (g++), so both compute every word alike by construction.  DESIGN.md 3.10.
//
// Number forms.  The witness arrives in REGULAR form (what the multi-exponentiations read) and is multiplied into gnark's Montgomery
// form (x 2^256 mod r, canonical) once per proof; coefficients arrive in that form.  A row's sum is kept CANONICAL (eight words below
// r, exact modular additions), so it does not depend on the order of its terms or on how lanes split them: kernels, host path and
// Python integers agree bit for bit.  Products go through the ten-limb multiplier of bn254_fr.cuh: fr_mul divides by 2^260, so
// (16 c 2^256) (w 2^256) / 2^260 = c w 2^256 -- fr_from_gnark on one operand, raw limbs on the other, no conversion afterwards.  Up
// to R1CS_LAZY_TERMS products are added as lazy limbs (each below 1.2 r with limbs below 2^25: the sum stays below 16 r and 2^28,
// the bounds fr_freeze_words takes) and made canonical together.
//
// A term is one u64: wire | coefficient id << 32 | class << 62.  The class of a dictionary entry is found once, at create time:
// 0 (the term is skipped), +1 / -1 (a modular addition / subtraction of the witness word, no coefficient load, no multiplication)
// or general.
#pragma once
#include "bn254_fr.cuh"

#define R1CS_ZERO 0u
#define R1CS_PLUS_ONE 1u
#define R1CS_MINUS_ONE 2u
#define R1CS_GENERAL 3u

// rows of at most R1CS_BIN0_MAX terms: one lane per row; of at most R1CS_BIN1_MAX: eight lanes; longer ones: a wave of 64
#define R1CS_BIN0_MAX 4u
#define R1CS_BIN1_MAX 64u
#define R1CS_LAZY_TERMS 8u

#define R1CS_MAX_CONSTRAINTS (1ull << 30)   // 3 n_constraints row indices fit u32
#define R1CS_MAX_WIRES (1ull << 32)
#define R1CS_MAX_TERMS (1ull << 40)
#define R1CS_MAX_COEFFS (1u << 30)          // the id shares a u32 with the class

#define R1CS_R_WORDS {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u}
// 1 and r - 1 in gnark's Montgomery form
#define R1CS_ONE_WORDS {0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u}
#define R1CS_MINUS_ONE_WORDS {0xa0000006u, 0x974bc177u, 0xda58a367u, 0xf13771b2u, 0x0908122eu, 0x51e1a247u, 0x4729c0fau, 0x2259d6b1u}
// 2^516 mod r as raw limbs: fr_mul(raw w, this) = w 2^256 mod r, the regular -> Montgomery step of a witness word
#define R1CS_2P516 {{35052144, 60364472, 31660984, 7919382, 20964267, 49152533, 25378131, 19489554, 51901668, 547650}}

// one field element: eight little-endian words, canonical
struct r1cs_el {
    u32 w[8];
};
// 16 bytes moved by one access
struct __attribute__((aligned(16), may_alias)) r1cs_q {
    u32 w[4];
};

ZKLC_HD r1cs_el r1cs_load(const u32 *p) {
    const r1cs_q lo = reinterpret_cast<const r1cs_q *>(p)[0], hi = reinterpret_cast<const r1cs_q *>(p)[1];
    r1cs_el r;
    for (int i = 0; i < 4; i++) {
        r.w[i] = lo.w[i];
        r.w[4 + i] = hi.w[i];
    }
    return r;
}
ZKLC_HD void r1cs_store(u32 *p, const r1cs_el &a) {
    r1cs_q lo, hi;
    for (int i = 0; i < 4; i++) {
        lo.w[i] = a.w[i];
        hi.w[i] = a.w[4 + i];
    }
    reinterpret_cast<r1cs_q *>(p)[0] = lo;
    reinterpret_cast<r1cs_q *>(p)[1] = hi;
}
ZKLC_HD r1cs_el r1cs_zero() {
    r1cs_el r;
    for (int i = 0; i < 8; i++) r.w[i] = 0;
    return r;
}
ZKLC_HD u32 r1cs_eq_words(const u32 *a, const u32 *b) {
    u32 d = 0;
    for (int i = 0; i < 8; i++) d |= a[i] ^ b[i];
    return d == 0;
}
// a >= r
ZKLC_HD u32 r1cs_ge_r(const u32 *a) {
    const u32 R[8] = R1CS_R_WORDS;
    u64 borrow = 0;
    for (int i = 0; i < 8; i++) borrow = ((u64)a[i] - R[i] - borrow) >> 63;
    return borrow == 0;
}

// a + b mod r for canonical a, b (the sum is below 2 r < 2^255: no carry out of the eight words)
ZKLC_HD r1cs_el r1cs_add(const r1cs_el &a, const r1cs_el &b) {
    const u32 R[8] = R1CS_R_WORDS;
    r1cs_el s, d;
    u64 c = 0;
    for (int i = 0; i < 8; i++) {
        c += (u64)a.w[i] + b.w[i];
        s.w[i] = (u32)c;
        c >>= 32;
    }
    u64 borrow = 0;
    for (int i = 0; i < 8; i++) {
        const u64 x = (u64)s.w[i] - R[i] - borrow;
        d.w[i] = (u32)x;
        borrow = x >> 63;
    }
    for (int i = 0; i < 8; i++) s.w[i] = borrow ? s.w[i] : d.w[i];
    return s;
}
// a - b mod r for canonical a, b
ZKLC_HD r1cs_el r1cs_sub(const r1cs_el &a, const r1cs_el &b) {
    const u32 R[8] = R1CS_R_WORDS;
    r1cs_el d;
    u64 borrow = 0;
    for (int i = 0; i < 8; i++) {
        const u64 x = (u64)a.w[i] - b.w[i] - borrow;
        d.w[i] = (u32)x;
        borrow = x >> 63;
    }
    const u32 m = borrow ? 0xffffffffu : 0u;
    u64 c = 0;
    for (int i = 0; i < 8; i++) {
        c += (u64)d.w[i] + (R[i] & m);
        d.w[i] = (u32)c;
        c >>= 32;
    }
    return d;
}

// class of a dictionary entry (eight words, gnark's Montgomery form, below r)
ZKLC_HD u32 r1cs_classify(const u32 *c) {
    const u32 one[8] = R1CS_ONE_WORDS, minus_one[8] = R1CS_MINUS_ONE_WORDS;
    u32 o = 0;
    for (int i = 0; i < 8; i++) o |= c[i];
    if (o == 0) return R1CS_ZERO;
    if (r1cs_eq_words(c, one)) return R1CS_PLUS_ONE;
    if (r1cs_eq_words(c, minus_one)) return R1CS_MINUS_ONE;
    return R1CS_GENERAL;
}
ZKLC_HD u64 r1cs_pack_term(u32 wire, u32 coeff, u32 cls) { return (u64)wire | (u64)coeff << 32 | (u64)cls << 62; }

// one witness word, regular form (any value below 2^256: a word >= r is reduced) -> gnark's Montgomery form, canonical
ZKLC_HD r1cs_el r1cs_witness_to_mont(const u32 *regular) {
    const r1cs_el x = r1cs_load(regular);
    const fr k = R1CS_2P516;
    r1cs_el r;
    fr_freeze_words(r.w, fr_mul(fr_from_words_raw(x.w), k));
    return r;
}

// the running sum of (a lane's share of) one row
struct r1cs_acc {
    r1cs_el s;   // canonical
    fr g;        // products not yet canonical: n_lazy of them
    u32 n_lazy;
};
ZKLC_HD void r1cs_acc_init(r1cs_acc &a) {
    a.s = r1cs_zero();
    a.g = fr_zero();
    a.n_lazy = 0;
}
ZKLC_HD void r1cs_acc_flush(r1cs_acc &a) {
    if (!a.n_lazy) return;
    r1cs_el p;
    fr_freeze_words(p.w, a.g);
    a.s = r1cs_add(a.s, p);
    a.g = fr_zero();
    a.n_lazy = 0;
}
// witness: n_wires x 8 words in Montgomery form; coeffs: the dictionary
ZKLC_HD void r1cs_acc_term(r1cs_acc &a, u64 term, const u32 *witness, const u32 *coeffs) {
    const u32 cls = (u32)(term >> 62);
    if (cls == R1CS_ZERO) return;
    const r1cs_el x = r1cs_load(witness + 8 * (u64)(u32)term);
    if (cls == R1CS_PLUS_ONE) {
        a.s = r1cs_add(a.s, x);
    } else if (cls == R1CS_MINUS_ONE) {
        a.s = r1cs_sub(a.s, x);
    } else {
        const r1cs_el c = r1cs_load(coeffs + 8 * (u64)((u32)(term >> 32) & 0x3fffffffu));
        a.g = fr_add(a.g, fr_mul(fr_from_gnark(c.w), fr_from_words_raw(x.w)));
        if (++a.n_lazy == R1CS_LAZY_TERMS) r1cs_acc_flush(a);
    }
}
// terms [begin, end) of one row in steps of `stride`, starting at begin + first: the whole row for (0, 1), a lane's share otherwise
ZKLC_HD r1cs_el r1cs_row_sum(const u64 *terms, u64 begin, u64 end, u32 first, u32 stride, const u32 *witness, const u32 *coeffs) {
    r1cs_acc a;
    r1cs_acc_init(a);
    for (u64 t = begin + first; t < end; t += stride) r1cs_acc_term(a, terms[t], witness, coeffs);
    r1cs_acc_flush(a);
    return a.s;
}

// a b = c for three canonical Montgomery words: a b 2^256 as a lazy element, minus c 2^256 as raw limbs
ZKLC_HD u32 r1cs_satisfied(const u32 *a, const u32 *b, const u32 *c) {
    const r1cs_el x = r1cs_load(a), y = r1cs_load(b), z = r1cs_load(c);
    return fr_is_zero(fr_sub(fr_mul(fr_from_gnark(x.w), fr_from_words_raw(y.w)), fr_from_words_raw(z.w)));
}

// ---- the system as the library keeps it (host side; the device arrays are r1cs_eval.hip's) ----
#include <vector>
struct zklc_r1cs {
    u64 n_constraints = 0, n_wires = 0, nnz = 0;
    u32 n_coeff = 0;
    std::vector<u64> row_ptr;      // 3 n_constraints + 1
    std::vector<u64> terms;        // nnz packed terms, the caller's order
    std::vector<u32> coeffs;       // n_coeff x 8 words
    std::vector<u32> perm;         // the row indices of bin 0, then bin 1, then bin 2 (each ascending)
    u64 bin_rows[3] = {0, 0, 0};
    u64 bin_terms[3] = {0, 0, 0};
    // device copies (ctx != NULL at create)
    int device = -1;
    void *d_row_ptr = nullptr, *d_terms = nullptr, *d_coeffs = nullptr, *d_perm = nullptr;
};
// validates and builds the host form; no GPU call (r1cs_eval_host.cpp)
int32_t r1cs_build_host(uint64_t n_constraints, uint64_t n_wires, const uint64_t *row_ptr, const uint32_t *term_wire,
                        const uint32_t *term_coeff, uint64_t nnz, const uint64_t *coeffs, uint32_t n_coeff, zklc_r1cs **out);
void r1cs_free_host(zklc_r1cs *s);
