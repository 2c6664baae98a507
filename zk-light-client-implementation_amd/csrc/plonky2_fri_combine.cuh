// The FRI opening combination (fri/oracle.rs `prove_openings`):
//   out(x) = alpha^nch * (sum_i alpha^i p_i(x) - y0) / (x - zeta) + (sum_{i<nch} alpha^i z_i(x) - y1) / (x - g zeta)
// over the four committed batches (constants and sigmas, wires, Z and partial products, quotient chunks).
//
// The sums are linear in the polynomials, so they are formed in two ways with ONE accumulation loop (p2_fri_alpha_sum):
//   points:       at every LDE point p over the four LDE matrices (stride N) -- p2_fri_combine_kernel in plonky2_prover.hip;
//   coefficients: at every coefficient index j over the four coefficient arrays (stride n), which gives the coefficients of
//                 G = sum_i alpha^i p_i and H = sum_{i<nch} alpha^i z_i as four base-field columns [G.a, G.b, H.a, H.b] x n
//                 (p2_fri_coeff_combine_kernel).  The NTT is linear over the base field, so one LDE of those four columns gives
//                 G and H at the N points, and p2_fri_coeff_finish_kernel does the two divisions.  That reads n words per
//                 polynomial instead of N and does 2^-rate_bits of the multiply-accumulates.
// Every value is exact field arithmetic written canonically, so both ways give the same array element for element.
//
// ZKLC_HD throughout: tests/fri_coeff_host instantiates the lane functions with g++, tests/fri_coeff_dev launches the kernels.
#pragma once
#include "plonky2_perm_terms.cuh"

#define P2_FRI_THREADS 256

// sum_i alpha^i m_i[p] over the columns of four matrices (column i of matrix m at mats[m] + i * stride), added into the limb
// columns (sa, sb) of the two coordinates.  alpha^i comes from a table of 22-bit limbs (p2_ext_pow_limbs_kernel: 12 words per
// power) and every term is twelve carry-free v_mad_u64_u32 (gl_acc3_mul) -- no Horner chain as long as the list.  Sixteen loads
// are in flight; a column holds 2^10 products = 512 terms, so the columns are folded every 384 (the tails below add < 48).
ZKLC_HD void p2_fri_alpha_sum(const u64 *const (&mats)[4], const u32 (&widths)[4], size_t stride, size_t p, gl_ktab *k6, gl_acc3 &sa,
                              gl_acc3 &sb) {
    u32 terms = 0;
    for (int m = 0; m < 4; m++) {
        const u64 *mat = mats[m] + p;
        const u32 w = widths[m];
        u32 j = 0;
        for (; j + 16 <= w; j += 16, k6 += 16 * 12) {   // sixteen loads in flight
            u64 v[16];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int q = 0; q < 16; q++) v[q] = mat[(size_t)(j + q) * stride];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int q = 0; q < 16; q++) {
                gl_acc3_mul(sa, v[q], k6 + 12 * q);
                gl_acc3_mul(sb, v[q], k6 + 12 * q + 6);
            }
            if ((terms += 16) >= 384) {
                terms = 0;
                gl_acc3_normalize(sa);
                gl_acc3_normalize(sb);
            }
        }
        for (; j < w; j++, k6 += 12) {
            u64 v = mat[(size_t)j * stride];
            gl_acc3_mul(sa, v, k6);
            gl_acc3_mul(sb, v, k6 + 6);
        }
        terms += 16;
    }
}
// sum_{i < nch} alpha^i z_i[p]: the first nch columns of the Z batch (nch <= P2_MAX_CH terms, no folding needed)
ZKLC_HD gl2 p2_fri_zs_sum(const u64 *zs, u32 nch, size_t stride, size_t p, gl_ktab *k6) {
    gl_acc3 ta = {0, 0, 0}, tb = {0, 0, 0};
    for (u32 j = 0; j < nch; j++) {
        u64 v = zs[(size_t)j * stride + p];
        gl_acc3_mul(ta, v, k6 + 12 * (size_t)j);
        gl_acc3_mul(tb, v, k6 + 12 * (size_t)j + 6);
    }
    return gl2_make(gl_acc3_reduce(ta), gl_acc3_reduce(tb));
}

// ------------------------------------------------------------------------------------------------ coefficient form
struct p2_fri_coeff_args {
    const u64 *coeffs[4];   // the four batches' coefficient arrays, stride n (any one order, the same in all four)
    u32 widths[4];
    u32 n, nch;
    const u32 *apow;        // alpha^i, i < sum(widths), as limbs (p2_ext_pow_limbs_kernel)
    u64 *out;               // [4][n]: G.a, G.b, H.a, H.b, canonical
};
// coefficient j of G and H
ZKLC_HD void p2_fri_coeff_lane(const p2_fri_coeff_args &a, size_t j) {
    gl_acc3 sa = {0, 0, 0}, sb = {0, 0, 0};
    p2_fri_alpha_sum(a.coeffs, a.widths, a.n, j, (gl_ktab *)a.apow, sa, sb);
    const gl2 h = p2_fri_zs_sum(a.coeffs[2], a.nch, a.n, j, (gl_ktab *)a.apow);
    a.out[j] = gl_acc3_reduce(sa);
    a.out[(size_t)a.n + j] = gl_acc3_reduce(sb);
    a.out[2 * (size_t)a.n + j] = h.a;
    a.out[3 * (size_t)a.n + j] = h.b;
}

struct p2_fri_finish_args {
    const u64 *gh;          // [4][N]: G.a, G.b, H.a, H.b on the LDE points (bit-reversed, as the committed matrices)
    const u64 *xs;          // the circuit's table of LDE points, x = g w^bitrev(p)
    u32 lde_bits;
    gl2 zeta, g_zeta, y0, y1, alpha_pow_nch;
    gl2 *out;               // [N]; in: the two inverse norms of the point (p2_fri_denominators_kernel), out: the combination
};
// out[p] = alpha^nch (G(x_p) - y0) / (x_p - zeta) + (H(x_p) - y1) / (x_p - g zeta)
ZKLC_HD void p2_fri_finish_lane(const p2_fri_finish_args &a, size_t p) {
    const size_t N = (size_t)1 << a.lde_bits;
    const u64 x = a.xs[p];
    const gl2 ninv = a.out[p];
    const gl2 g = gl2_make(a.gh[p], a.gh[N + p]), h = gl2_make(a.gh[2 * N + p], a.gh[3 * N + p]);
    const gl2 q0 = gl2_mul(gl2_sub(g, a.y0), p2_fri_den_inverse(x, a.zeta, ninv.a));
    const gl2 q1 = gl2_mul(gl2_sub(h, a.y1), p2_fri_den_inverse(x, a.g_zeta, ninv.b));
    a.out[p] = gl2_add(gl2_mul(q0, a.alpha_pow_nch), q1);
}

#if defined(__HIPCC__)
// one lane per coefficient index: consecutive lanes read consecutive words of every column
__global__ void __launch_bounds__(P2_FRI_THREADS) p2_fri_coeff_combine_kernel(p2_fri_coeff_args a) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < a.n) p2_fri_coeff_lane(a, j);
}
__global__ void __launch_bounds__(P2_FRI_THREADS) p2_fri_coeff_finish_kernel(p2_fri_finish_args a) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < ((size_t)1 << a.lde_bits)) p2_fri_finish_lane(a, p);
}
#endif
