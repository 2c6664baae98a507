// TEST INFRASTRUCTURE: the host half of tests/fri_coeff_dev/libfri_coeff_dev.so (plain C++; the arithmetic headers are host code
// only outside hipcc): one case of tests/fri_coeff_host/fri_coeff_cases.h through the kernel, held against its Horner sum.
#include "../fri_coeff_host/fri_coeff_cases.h"

extern "C" int fcd_combine(const u64 *const *coeffs, const u32 *widths, u32 n, u32 nch, const u32 *apow, u64 *out);

// Returns the number of output words that differ from the Horner sum or are not canonical (0 = equal), or minus the HIP error.
extern "C" int fcd_run_case(u32 total, u32 log_n, int spread) {
    fc_case c;
    fc_make(total, log_n, spread != 0, c);
    const u64 *coeffs[4] = {c.coeffs[0].data(), c.coeffs[1].data(), c.coeffs[2].data(), c.coeffs[3].data()};
    std::vector<u64> out((size_t)4 * c.n);
    const int rc = fcd_combine(coeffs, c.widths, c.n, c.nch, c.apow.data(), out.data());
    if (rc) return -rc;
    int diff = 0;
    for (size_t i = 0; i < out.size(); i++) diff += out[i] != c.want[i] || out[i] >= GL_P;
    return diff;
}
