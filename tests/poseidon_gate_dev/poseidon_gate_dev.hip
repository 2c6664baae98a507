// TEST INFRASTRUCTURE: the evaluators of the Poseidon gate behind a one-row-per-lane kernel, compiled with the library's flags
// (build.py: build_poseidon_gate_dev) into tests/poseidon_gate_dev/libposeidon_gate_dev.so; never part of libzklc_mi355.so.
// TYPE 120 = p2_eval_poseidon_stmt (the generated statements), 110 = p2_eval_poseidon_loose, 7 = p2_eval_poseidon.
#include <hip/hip_runtime.h>
#include "../../zk-light-client-implementation_amd/csrc/plonky2_gates.cuh"

#define PGD_BLOCK 64
#define PGD_POWERS 256

__global__ void pgd_alpha_table_kernel(const u64 *alpha, u32 nch, u32 *tab) {
    const u32 c = threadIdx.x;
    if (c >= P2_MAX_CH) return;
    u64 a = c < nch ? alpha[c] : alpha[0], pw = 1;      // an unused challenge's table is the first one's, as in the prover
    for (int k = 0; k < PGD_POWERS; k++) {
        gl_limbs22(pw, tab + ((size_t)c * PGD_POWERS + k) * 6);
        pw = gl_mul(pw, a);
    }
}

// row i: wires[i * 135 ..]; out[i * nch + c] = sum_k alpha_c^k constraint_k
template <int TYPE>
__global__ void __launch_bounds__(PGD_BLOCK) pgd_eval_kernel(const u64 *wires, const u32 *tab, u32 nch, u64 *acc_out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    p2_vars v;
    v.wires = wires + (size_t)i * 135;
    v.consts = v.wires;
    v.stride = 1;
    v.p = 0;
    v.nsel = 0;
    for (int k = 0; k < 4; k++) v.pih[k] = 0;
    p2_consumer out;
    out.nch = (int)nch;
    for (int c = 0; c < P2_MAX_CH; c++) out.apow[c] = (gl_ktab *)(tab + (size_t)c * PGD_POWERS * 6);
    out.reset(0);
    if constexpr (TYPE == P2_POSEIDON_STMT)
        p2_eval_poseidon_stmt(v, out);
    else if constexpr (TYPE == P2_POSEIDON_LOOSE)
        p2_eval_poseidon_loose(v, out);
    else
        p2_eval_poseidon(v, out);
#pragma unroll
    for (int c = 0; c < P2_MAX_CH; c++)
        if (c < (int)nch) acc_out[(size_t)i * nch + c] = out.result(c);
}

#define PGD_OK(e)                          \
    do {                                   \
        hipError_t e_ = (e);               \
        if (e_ != hipSuccess) {            \
            if (dw) (void)hipFree(dw);     \
            if (da) (void)hipFree(da);     \
            if (dt) (void)hipFree(dt);     \
            if (dout) (void)hipFree(dout); \
            return (int)e_;                \
        }                                  \
    } while (0)

// wires: n x 135, alpha: nch values (1 or 2), acc_out: n x nch.  Returns 0 or the HIP error.
extern "C" int pgd_eval(u32 type, const u64 *wires, const u64 *alpha, u32 nch, u64 *acc_out, u32 n) {
    void *dw = nullptr, *da = nullptr, *dt = nullptr, *dout = nullptr;
    if (!n || !nch || nch > P2_MAX_CH || (type != P2_POSEIDON_STMT && type != P2_POSEIDON_LOOSE && type != P2_POSEIDON)) return (int)hipErrorInvalidValue;
    PGD_OK(hipMalloc(&dw, 8ull * n * 135));
    PGD_OK(hipMalloc(&da, 8ull * nch));
    PGD_OK(hipMalloc(&dt, 4ull * P2_MAX_CH * PGD_POWERS * 6));
    PGD_OK(hipMalloc(&dout, 8ull * n * nch));
    PGD_OK(hipMemcpy(dw, wires, 8ull * n * 135, hipMemcpyHostToDevice));
    PGD_OK(hipMemcpy(da, alpha, 8ull * nch, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pgd_alpha_table_kernel, dim3(1), dim3(64), 0, 0, (const u64 *)da, nch, (u32 *)dt);
    const dim3 grid((n + PGD_BLOCK - 1) / PGD_BLOCK), block(PGD_BLOCK);
    if (type == P2_POSEIDON_STMT)
        hipLaunchKernelGGL(pgd_eval_kernel<P2_POSEIDON_STMT>, grid, block, 0, 0, (const u64 *)dw, (const u32 *)dt, nch, (u64 *)dout, n);
    else if (type == P2_POSEIDON_LOOSE)
        hipLaunchKernelGGL(pgd_eval_kernel<P2_POSEIDON_LOOSE>, grid, block, 0, 0, (const u64 *)dw, (const u32 *)dt, nch, (u64 *)dout, n);
    else
        hipLaunchKernelGGL(pgd_eval_kernel<P2_POSEIDON>, grid, block, 0, 0, (const u64 *)dw, (const u32 *)dt, nch, (u64 *)dout, n);
    PGD_OK(hipGetLastError());
    PGD_OK(hipDeviceSynchronize());
    PGD_OK(hipMemcpy(acc_out, dout, 8ull * n * nch, hipMemcpyDeviceToHost));
    (void)hipFree(dw);
    (void)hipFree(da);
    (void)hipFree(dt);
    (void)hipFree(dout);
    return 0;
}
