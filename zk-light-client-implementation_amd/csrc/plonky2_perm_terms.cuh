// Lane functions of the prover's per-point arithmetic outside the gates (plonky2_prover.hip), shared with tests/lean_arith_host:
// one chunk of the permutation argument, and the batched inversion of the FRI combination's denominators.
//
// Both restate what the kernels computed before with fewer and cheaper field operations.  Field multiplication is exact and every
// residue class has one canonical representative, so the values -- and with them the proof bytes -- are what they were.
#pragma once
#include "gl_ext.cuh"
#include "goldilocks_ntt_group.cuh"

#define P2_PERM_CHUNK 8   // wires per call (the quotient degree factor of the standard configuration)

// One chunk of prover.rs `wires_permutation_partial_products_and_zs` / plonk.go:84-119 at one point x:
//     np = prod_{q < cnt} (w_q + gamma + k_q (beta x)),    dp = prod_{q < cnt} (w_q + gamma + beta sigma_q),    cnt <= 8.
// wv / sv / kv = the wires, the sigmas and the coset shifts k_q of the chunk (entries q >= cnt are not read), bx = beta * x, which
// the caller computes once per point and challenge.
//
// The chain this replaces did  np = np * (w + beta * (k * x)),  dp = dp * (w + beta * sigma)  per wire: five compiled
// multiply-reduces (28 instructions each), the first product of each chain by 1, and sixteen products that wait for one another.
// Here, for four wires at a time: k_q * bx, then beta * sigma_q as one batch of four independent multiplications, then the four
// numerator and the four denominator factors multiplied as trees, side by side (4 + 2 products); the two halves of a chunk meet
// in one batch of two.  2 * (4 + 4 + 4 + 2) + 2 = 30 multiplications instead of 40, 22 of them through the batched statements
// (gl_mul_batch, 19 instructions; on the host gl_mul).  A partial chunk pads its factors with 1.  (Four wires at a time and not
// eight: the statements need 32 scratch registers and early-clobber results beside their operands, and the other half's eight
// loads stay in flight meanwhile -- the eight-wide batch did not fit 128 VGPRs.)
ZKLC_HD void p2_perm_half_terms(const u64 *wv, const u64 *sv, const u64 *kv, u32 cnt, u64 beta, u64 bx, u64 gamma, u64 &np, u64 &dp) {
    constexpr int H = P2_PERM_CHUNK / 2;
    // k_q * bx through the compiled gl_mul: k_q is wave-uniform in the kernels and stays in scalar registers there, where the
    // statements take vector operands only (eight copies, live across the whole half: the kernel went past 128 VGPRs)
    u64 kb[H], m[H], s[H];    // m[q] = sigma_q -> beta * sigma_q
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < H; q++) {
        const bool in = (u32)q < cnt;
        kb[q] = in ? gl_mul(kv[q], bx) : 0;
        m[q] = in ? sv[q] : 0;
        s[q] = beta;
    }
    gl_mul_batch<H>(m, s);
    // rows of the tree: f = {n0, n1, d0, d1}, h = {n2, n3, d2, d3}
    u64 f[H], h[H];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int q = 0; q < H; q++) {
        const bool in = (u32)q < cnt;
        const u64 w = in ? gl_add(wv[q], gamma) : 0;
        const u64 fn = in ? gl_add(w, kb[q]) : 1, fd = in ? gl_add(w, m[q]) : 1;
        if (q < H / 2) {
            f[q] = fn;
            f[H / 2 + q] = fd;
        } else {
            h[q - H / 2] = fn;
            h[q] = fd;
        }
    }
    gl_mul_batch<H>(f, h);                   // 4 -> 2 per product
    u64 f2[2] = {f[0], f[2]}, h2[2] = {f[1], f[3]};
    gl_mul_batch<2>(f2, h2);                 // 2 -> 1
    np = f2[0];
    dp = f2[1];
}
ZKLC_HD void p2_perm_chunk_terms(const u64 *wv, const u64 *sv, const u64 *kv, u32 cnt, u64 beta, u64 bx, u64 gamma, u64 &np, u64 &dp) {
    constexpr int H = P2_PERM_CHUNK / 2;
    p2_perm_half_terms(wv, sv, kv, cnt < (u32)H ? cnt : (u32)H, beta, bx, gamma, np, dp);
    if (cnt > (u32)H) {
        u64 a[2] = {np, dp}, b[2];
        p2_perm_half_terms(wv + H, sv + H, kv + H, cnt - H, beta, bx, gamma, b[0], b[1]);
        gl_mul_batch<2>(a, b);
        np = a[0];
        dp = a[1];
    }
}

// the chain as it was (ZKLC_LEAN_ARITH=0, and the reference of tests/lean_arith_host)
ZKLC_HD void p2_perm_chunk_terms_chain(const u64 *wv, const u64 *sv, const u64 *kv, u32 cnt, u64 beta, u64 x, u64 gamma, u64 &np, u64 &dp) {
    np = 1;
    dp = 1;
    for (u32 q = 0; q < cnt; q++) {
        u64 w = gl_add(wv[q], gamma);
        np = gl_mul(np, gl_add(w, gl_mul(beta, gl_mul(kv[q], x))));
        dp = gl_mul(dp, gl_add(w, gl_mul(beta, sv[q])));
    }
}

// ---- FRI combination (fri/oracle.rs `prove_openings`): 1 / (x - zeta) and 1 / (x - g zeta) for the LDE points.
// 1 / (a + b X) = (a - b X) / (a^2 - 7 b^2): what costs is the base-field inversion of the norm, a^(p - 2) = 64 squarings and 63
// multiplications, twice per point.  The norms of P2_FRI_DEN_POINTS points (two each) are inverted together with Montgomery's
// trick: one inversion and three multiplications per norm.  gl_inv(0) = 0 is kept element by element: a zero norm (x = zeta with
// zeta in the base field; 7 is a non-residue, so the norm vanishes only there) enters the running product as 1 and its inverse is
// written as 0, so that it cannot reach its neighbours.
#define P2_FRI_DEN_POINTS 8

// v[i] = 1 / v[i] (0 for v[i] = 0), i < N: one gl_inv
template <int N>
ZKLC_HD void gl_batch_inv(u64 *v) {
    u64 pre[N], acc = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < N; i++) {
        pre[i] = acc;
        acc = gl_mul(acc, v[i] ? v[i] : 1);
    }
    u64 inv = gl_inv(acc);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = N - 1; i >= 0; i--) {
        const u64 vi = v[i];
        v[i] = vi ? gl_mul(inv, pre[i]) : 0;
        inv = gl_mul(inv, vi ? vi : 1);
    }
}

// out[q] = (1 / norm(x_q - zeta), 1 / norm(x_q - g zeta)), q < P2_FRI_DEN_POINTS;  norm(x - z) = (x - z.a)^2 - 7 z.b^2
ZKLC_HD void p2_fri_den_inverse_norms(const u64 *x, gl2 zeta, gl2 g_zeta, gl2 *out) {
    constexpr int C = P2_FRI_DEN_POINTS;
    u64 v[2 * C];
    const u64 zb0 = gl_mul7(gl_sqr(zeta.b)), zb1 = gl_mul7(gl_sqr(g_zeta.b));
    for (int q = 0; q < C; q++) {
        v[q] = gl_sub(gl_sqr(gl_sub(x[q], zeta.a)), zb0);
        v[C + q] = gl_sub(gl_sqr(gl_sub(x[q], g_zeta.a)), zb1);
    }
    gl_batch_inv<2 * C>(v);
    for (int q = 0; q < C; q++) out[q] = gl2_make(v[q], v[C + q]);
}

// 1 / (x - z) from the inverse norm: the value gl2_inv(gl2_sub(gl2_make(x, 0), z)) has
ZKLC_HD gl2 p2_fri_den_inverse(u64 x, gl2 z, u64 norm_inv) {
    const gl2 d = gl2_sub(gl2_make(x, 0), z);
    return gl2_make(gl_mul(d.a, norm_inv), gl_mul(gl_neg(d.b), norm_inv));
}
