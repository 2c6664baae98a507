// plonky2 verifier: the per-lane pieces of the FRI query phase, written once for both compilers (common.cuh) so that the host
// path (csrc/plonky2_verifier_host.cpp) and the kernels (csrc/plonky2_verifier.hip) compute the same thing.
//   p2v_merkle_lane  one Merkle opening (an initial oracle or one FRI reduction) of one query round: leaf hash, path, cap
//   p2v_fri_lane     the fold chain of one query round: initial combination, consistency checks, coset interpolation at
//                    beta (barycentric), final polynomial
// Both read their inputs straight from the proof bytes (ProofWithPublicInputs::to_bytes) at the offsets of a p2v_layout, which
// is the same for every proof of a circuit.  The offsets are not 8-byte aligned (the u8 sibling counts), so every element is
// read bytewise.  Restated from oracle/plonky2_verifier.py (gnark-plonky2-verifier/fri/fri.go:97-160, 187-251, 314-497).
#pragma once
#include "gl_ext.cuh"
#include "poseidon_gl.cuh"
#include "poseidon_bn254.cuh"

#define P2V_MAX_ARITIES 8
#define P2V_MAX_TREES (4 + P2V_MAX_ARITIES)

// byte offsets and shapes of one circuit's proofs
struct p2v_layout {
    u64 bytes;                       // proof length
    u64 cap_off[3];                  // wires, zs / partial products, quotient caps
    u64 openings_off;                // constants, sigmas, wires, zs, zs_next, partial products, quotient (16 bytes each)
    u64 commit_cap_off[P2V_MAX_ARITIES];
    u64 rounds_off, round_bytes;     // query round r starts at rounds_off + r * round_bytes
    u64 tree_off[P2V_MAX_TREES];     // within a round: leaf of tree t (0..3 initial oracles, 4 + i = reduction i)
    u64 final_off, pow_off, npi_off, pi_off;
    u32 hasher, nch, num_arities, num_trees, rounds, lde_bits, final_len;
    u32 cap_h0;                      // cap height of the initial trees (clamped to the tree height)
    u32 arity_bits[P2V_MAX_ARITIES];
    u32 commit_cap_h[P2V_MAX_ARITIES];
    u32 leaf_words[P2V_MAX_TREES];   // u64 elements in the leaf of tree t
    u32 depth[P2V_MAX_TREES];        // siblings of tree t
    u32 n_openings[7];
};

// what the query phase of one proof needs from the transcript replay
struct p2v_proof_tab {
    gl2 fri_alpha, alpha_pow_nch, zeta, gzeta, red[2];
    gl2 betas[P2V_MAX_ARITIES];
};

ZKLC_HD u32 p2v_ld32(const uint8_t *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }
ZKLC_HD u64 p2v_ld64(const uint8_t *p) { return (u64)p2v_ld32(p) | (u64)p2v_ld32(p + 4) << 32; }
ZKLC_HD gl2 p2v_ld_ext(const uint8_t *p) { return gl2_make(p2v_ld64(p), p2v_ld64(p + 8)); }

ZKLC_HD bool p2v_digest_eq(const uint8_t *a, const uint8_t *h32) {
    bool eq = true;
    for (int i = 0; i < 32; i++) eq = eq && a[i] == h32[i];
    return eq;
}

ZKLC_HD void p2v_gl_leaf_hash(const uint8_t *leaf, u32 len, u64 *out4) {
    if (len <= 4) {
        for (u32 i = 0; i < 4; i++) out4[i] = i < len ? p2v_ld64(leaf + 8 * i) : 0;
        return;
    }
    u64 s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 off = 0; off < len; off += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (off + j < len) s[j] = p2v_ld64(leaf + 8 * (size_t)(off + j));
        poseidon_gl_permute(s);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) out4[i] = s[i];
}

ZKLC_HD fr p2v_bn_pack3(const uint8_t *in, u32 count) {
    u32 w[8];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        u64 e = (u32)k < count ? p2v_ld64(in + 8 * k) : 0;
        w[2 * k] = (u32)e;
        w[2 * k + 1] = (u32)(e >> 32);
    }
    w[6] = w[7] = 0;
    return fr_from_regular(w);
}

// Merkle opening of tree `t` in query round `r` of `proof` (x_index = the round's query index, low lde_bits bits).
// cap0: the circuit's constants / sigmas cap.  Returns true when the path reaches its cap entry.  HASHER = L.hasher (a template
// parameter, so that a kernel instance holds the registers of one hasher only).
template <u32 HASHER>
ZKLC_HD bool p2v_merkle_lane(const p2v_layout &L, const uint8_t *proof, const uint8_t *cap0, u32 r, u32 t, u32 x_index) {
    const uint8_t *leaf = proof + L.rounds_off + (u64)r * L.round_bytes + L.tree_off[t];
    const u32 len = L.leaf_words[t], depth = L.depth[t];
    const uint8_t *sib = leaf + 8 * (size_t)len + 1;
    u32 index = x_index;
    const uint8_t *cap;
    if (t == 0) {
        cap = cap0;
    } else if (t < 4) {
        cap = proof + L.cap_off[t - 1];
    } else {
        cap = proof + L.commit_cap_off[t - 4];
        for (u32 i = 0; i <= t - 4; i++) index >>= L.arity_bits[i];
    }
    uint8_t cur[32];
    if (HASHER == 0) {
        u64 h[4];
        p2v_gl_leaf_hash(leaf, len, h);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (u32 d = 0; d < depth; d++) {
            // select left / right, then ONE permutation (the index bits differ across the lanes of a wave)
            u64 l[4], r[4], o[4];
            const bool right = index & 1;
            for (int i = 0; i < 4; i++) {
                const u64 s = p2v_ld64(sib + 32 * (size_t)d + 8 * i);
                l[i] = right ? s : h[i];
                r[i] = right ? h[i] : s;
            }
            poseidon_gl_two_to_one(l, r, o);
            for (int i = 0; i < 4; i++) h[i] = o[i];
            index >>= 1;
        }
        for (int i = 0; i < 32; i++) cur[i] = (uint8_t)(h[i >> 3] >> (8 * (i & 7)));
    } else {
        // Poseidon-BN254: the leaf sponge and the path share ONE permutation site (a second inlined copy of the 4-element Fr state
        // machinery spills); the running digest stays in Montgomery form between levels (every value involved is < r)
        const u32 absorbs = len <= 3 ? 0 : (len + 8) / 9;
        fr st[4];
#pragma unroll
        for (int i = 0; i < 4; i++) st[i] = fr_zero();
        fr h = p2v_bn_pack3(leaf, len < 3 ? len : 3);     // hash_or_noop of <= 3 elements: the elements themselves
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (u32 k = 0; k < absorbs + depth; k++) {
            if (k < absorbs) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    u32 o = 9 * k + 3 * j;
                    if (o < len) st[j + 1] = p2v_bn_pack3(leaf + 8 * (size_t)o, len - o < 3 ? len - o : 3);
                }
            } else {
                u32 w[8];
                for (int i = 0; i < 8; i++) w[i] = p2v_ld32(sib + 32 * (size_t)(k - absorbs) + 4 * i);
                fr sb = fr_from_regular(w);
                st[0] = fr_zero();
                st[1] = fr_zero();
                st[2] = (index & 1) ? sb : h;
                st[3] = (index & 1) ? h : sb;
                index >>= 1;
            }
            poseidon_bn254_permute(st);
            h = st[0];
        }
        u32 out[8];
        fr_to_regular(out, h);
        for (int i = 0; i < 32; i++) cur[i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
    }
    return p2v_digest_eq(cur, cap + 32 * (size_t)index);
}

ZKLC_HD u32 p2v_bitrev(u32 v, u32 bits) {
    u32 r = 0;
    for (u32 i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// Horner step of reduce_with_powers over a leaf of base-field values, last element first
ZKLC_HD gl2 p2v_horner_leaf(gl2 acc, const uint8_t *leaf, u32 len, gl2 alpha) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 i = len; i-- > 0;) acc = gl2_add_base(gl2_mul(acc, alpha), p2v_ld64(leaf + 8 * (size_t)i));
    return acc;
}

// The fold chain of query round r.  Returns 0, 1 + i (consistency of reduction i) or 1 + num_arities (final polynomial).
ZKLC_HD u32 p2v_fri_lane(const p2v_layout &L, const uint8_t *proof, const p2v_proof_tab &T, u32 r, u32 x_index) {
    const uint8_t *rb = proof + L.rounds_off + (u64)r * L.round_bytes;
    // x = g * w^bitrev(x_index) over the LDE domain (fri.go:187-206)
    u64 x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(L.lde_bits), p2v_bitrev(x_index, L.lde_bits)));
    // initial combination (fri.go:208-251): batch 0 = every polynomial of the 4 oracles at zeta, batch 1 = the Zs at g * zeta
    gl2 red0 = gl2_make(0, 0);
    for (int k = 3; k >= 0; k--) red0 = p2v_horner_leaf(red0, rb + L.tree_off[k], L.leaf_words[k], T.fri_alpha);
    gl2 red1 = p2v_horner_leaf(gl2_make(0, 0), rb + L.tree_off[2], L.nch, T.fri_alpha);
    gl2 d0 = gl2_sub(gl2_make(x, 0), T.zeta), d1 = gl2_sub(gl2_make(x, 0), T.gzeta);
    gl2 inv = gl2_inv(gl2_mul(d0, d1));     // one inversion for both denominators
    gl2 s = gl2_mul(gl2_mul(gl2_sub(red0, T.red[0]), d1), inv);
    s = gl2_add(gl2_mul(T.alpha_pow_nch, s), gl2_mul(gl2_mul(gl2_sub(red1, T.red[1]), d0), inv));
    u32 idx = x_index;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 i = 0; i < L.num_arities; i++) {
        const u32 ab = L.arity_bits[i], arity = 1u << ab;
        const uint8_t *ev = rb + L.tree_off[4 + i];
        const u32 within = idx & (arity - 1);
        if (!gl2_eq(p2v_ld_ext(ev + 16 * (size_t)within), s)) return 1 + i;
        // interpolate the coset start * <g_k> at beta (fri.go:314-384), barycentric on a multiplicative coset:
        //   p(beta) = (beta^m - start^m) / (m start^m) * sum_a y_a x_a prod_{b != a} (beta - x_b) / prod_b (beta - x_b)
        // with x_a = start g_k^a, y_a = evals[bitrev(a)] and start^m = x^m (g_k^m = 1): one inversion per reduction, not O(m^2).
        // One backward pass keeps num = sum_{a' >= a} y_a' x_a' prod_{b >= a, b != a'} den_b and suffix = prod_{b >= a} den_b.
        const u64 gk = gl_root_of_unity(ab), gk_inv = gl_pow(gk, arity - 1);
        const u64 start = gl_mul(gl_pow(gk, (arity - p2v_bitrev(within, ab)) & (arity - 1)), x);
        const u64 xm = gl_pow(x, arity);
        const gl2 beta = T.betas[i];
        gl2 num = gl2_make(0, 0), suffix = gl2_make(1, 0), hit_val = gl2_make(0, 0);
        bool hit = false;
        u64 xa = gl_mul(start, gk_inv);     // x_(m-1) = start g_k^(m-1) = start / g_k
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (u32 a = arity; a-- > 0;) {
            const gl2 den = gl2_sub(beta, gl2_make(xa, 0));
            const gl2 ya = p2v_ld_ext(ev + 16 * (size_t)p2v_bitrev(a, ab));
            if (den.a == 0 && den.b == 0) {   // beta is a coset point: the interpolant takes that point's value
                hit = true;
                hit_val = ya;
            }
            num = gl2_add(gl2_mul(num, den), gl2_mul(gl2_scale(ya, xa), suffix));
            suffix = gl2_mul(suffix, den);
            xa = gl_mul(xa, gk_inv);
        }
        gl2 acc = hit_val;
        if (!hit) {
            const gl2 zb = gl2_sub(gl2_pow(beta, arity), gl2_make(xm, 0));
            acc = gl2_mul(gl2_mul(zb, num), gl2_inv(gl2_scale(suffix, gl_mul(arity, xm))));
        }
        s = acc;
        x = xm;
        idx >>= ab;
    }
    // final polynomial (fri.go:253-259, 493-497)
    const uint8_t *fp = proof + L.final_off;
    gl2 e = gl2_make(0, 0);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (u32 i = L.final_len; i-- > 0;) e = gl2_add(gl2_scale(e, x), p2v_ld_ext(fp + 16 * (size_t)i));
    return gl2_eq(e, s) ? 0 : 1 + L.num_arities;
}
