// TEST INFRASTRUCTURE: a stand-alone host program around the host form of the coefficient-form FRI combination
// (csrc/plonky2_fri_combine.cuh: p2_fri_coeff_lane, the body of p2_fri_coeff_combine_kernel, and p2_fri_finish_lane).  Built by
// tests/test_fri_coeff_host.py with g++, once plain and once with -fsanitize=address,undefined; never linked into
// libzklc_mi355.so.
//
//   fri_coeff_host        every case of fri_coeff_cases.h: the lane function at every index against the Horner sum; then the
//                         pointwise finish against the formula with two extension inversions.  Prints one line per case;
//                         exit 0 = all equal.
#include "fri_coeff_cases.h"
#include <stdio.h>

static int check_finish() {
    // 2^4 points; the inverse norms as p2_fri_denominators_kernel leaves them, eight points to a call
    const u32 lde_bits = 4, N = 1u << lde_bits;
    u64 seed = 99;
    std::vector<u64> gh((size_t)4 * N), xs(N);
    std::vector<gl2> out(N), want(N);
    for (auto &v : gh) v = fc_rand(seed);
    for (auto &v : xs) v = fc_rand(seed);
    gh[0] = 0, gh[N] = GL_P - 1, gh[2 * N + 1] = 1, gh[3 * N + 1] = 0;
    p2_fri_finish_args a = {};
    a.gh = gh.data();
    a.xs = xs.data();
    a.lde_bits = lde_bits;
    a.zeta = gl2_make(fc_rand(seed), fc_rand(seed));
    a.g_zeta = gl2_make(fc_rand(seed), fc_rand(seed));
    a.y0 = gl2_make(fc_rand(seed), GL_P - 1);
    a.y1 = gl2_make(0, fc_rand(seed));
    a.alpha_pow_nch = gl2_make(fc_rand(seed), fc_rand(seed));
    a.out = out.data();
    for (u32 p0 = 0; p0 < N; p0 += P2_FRI_DEN_POINTS) p2_fri_den_inverse_norms(&xs[p0], a.zeta, a.g_zeta, &out[p0]);
    int bad = 0;
    for (u32 p = 0; p < N; p++) {
        const gl2 g = gl2_make(gh[p], gh[N + p]), h = gl2_make(gh[2 * N + p], gh[3 * N + p]);
        const gl2 q0 = gl2_mul(gl2_sub(g, a.y0), gl2_inv(gl2_sub(gl2_make(xs[p], 0), a.zeta)));
        const gl2 q1 = gl2_mul(gl2_sub(h, a.y1), gl2_inv(gl2_sub(gl2_make(xs[p], 0), a.g_zeta)));
        want[p] = gl2_add(gl2_mul(q0, a.alpha_pow_nch), q1);
        p2_fri_finish_lane(a, p);
        bad += out[p].a != want[p].a || out[p].b != want[p].b;
    }
    printf("finish: %u points, %d differ\n", N, bad);
    return bad;
}

int main() {
    int bad = 0;
    for (u32 total : FC_WIDTHS)
        for (u32 log_n : FC_LOG_N)
            for (int spread = 0; spread < 2; spread++) {
                fc_case c;
                fc_make(total, log_n, spread != 0, c);
                std::vector<u64> out((size_t)4 * c.n, ~0ULL);
                p2_fri_coeff_args a = {};
                for (int k = 0; k < 4; k++) {
                    a.coeffs[k] = c.coeffs[k].data();
                    a.widths[k] = c.widths[k];
                }
                a.n = c.n;
                a.nch = c.nch;
                a.apow = c.apow.data();
                a.out = out.data();
                for (u32 j = 0; j < c.n; j++) p2_fri_coeff_lane(a, j);
                int diff = 0;
                for (size_t i = 0; i < out.size(); i++) diff += out[i] != c.want[i] || out[i] >= GL_P;
                printf("width %u (%u %u %u %u) n %u: %d differ\n", total, c.widths[0], c.widths[1], c.widths[2], c.widths[3], c.n, diff);
                bad += diff;
            }
    bad += check_finish();
    return bad ? 1 : 0;
}
