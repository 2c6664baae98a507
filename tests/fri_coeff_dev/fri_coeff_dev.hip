// TEST INFRASTRUCTURE: p2_fri_coeff_combine_kernel (csrc/plonky2_fri_combine.cuh) behind a host-pointer call, compiled with the
// library's flags and linked with fri_coeff_dev_cases.cpp (build.py: build_fri_coeff_dev) into
// tests/fri_coeff_dev/libfri_coeff_dev.so; never part of libzklc_mi355.so.
#include <hip/hip_runtime.h>
#include "../../zk-light-client-implementation_amd/csrc/plonky2_fri_combine.cuh"

#define FCD_OK(e)                                        \
    do {                                                 \
        hipError_t e_ = (e);                             \
        if (e_ != hipSuccess) {                          \
            for (int q = 0; q < 6; q++)                  \
                if (dev[q]) (void)hipFree(dev[q]);       \
            return (int)e_;                              \
        }                                                \
    } while (0)

// coeffs[k]: widths[k] x n words, apow: 12 words per power for sum(widths) powers, out: 4 x n words.  Returns 0 or the HIP error.
extern "C" int fcd_combine(const u64 *const *coeffs, const u32 *widths, u32 n, u32 nch, const u32 *apow, u64 *out) {
    void *dev[6] = {};
    p2_fri_coeff_args a = {};
    u32 total = 0;
    if (!n || nch > widths[2]) return (int)hipErrorInvalidValue;
    for (int k = 0; k < 4; k++) {
        const size_t bytes = (size_t)widths[k] * n * 8;
        FCD_OK(hipMalloc(&dev[k], bytes ? bytes : 8));
        if (bytes) FCD_OK(hipMemcpy(dev[k], coeffs[k], bytes, hipMemcpyHostToDevice));
        a.coeffs[k] = (const u64 *)dev[k];
        a.widths[k] = widths[k];
        total += widths[k];
    }
    FCD_OK(hipMalloc(&dev[4], (size_t)total * 48 + 8));
    FCD_OK(hipMemcpy(dev[4], apow, (size_t)total * 48, hipMemcpyHostToDevice));
    FCD_OK(hipMalloc(&dev[5], (size_t)4 * n * 8));
    FCD_OK(hipMemset(dev[5], 0xFF, (size_t)4 * n * 8));
    a.n = n;
    a.nch = nch;
    a.apow = (const u32 *)dev[4];
    a.out = (u64 *)dev[5];
    hipLaunchKernelGGL(p2_fri_coeff_combine_kernel, dim3((n + P2_FRI_THREADS - 1) / P2_FRI_THREADS), dim3(P2_FRI_THREADS), 0, 0, a);
    FCD_OK(hipGetLastError());
    FCD_OK(hipDeviceSynchronize());
    FCD_OK(hipMemcpy(out, dev[5], (size_t)4 * n * 8, hipMemcpyDeviceToHost));
    for (int q = 0; q < 6; q++) (void)hipFree(dev[q]);
    return 0;
}
