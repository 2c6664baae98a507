// TEST INFRASTRUCTURE: the device twin of tests/hostsim.  The same arithmetic headers (csrc/*.cuh), compiled by hipcc for
// gfx950 with the library's flags, behind batched entry points: arrays of operand tuples in, arrays of results out, ONE LANE PER
// TUPLE evaluating the product's own lane function.  This is where the device-only forms (the inline-asm statements of
// goldilocks_mul_asm.inc / poseidon_gl_asm.inc and everything else behind __HIP_DEVICE_COMPILE__) meet edge operands on the
// hardware (tests/test_gpu_devsim.py).  Never linked into libzklc_mi355.so.
//
// Every entry point copies its operands to the device, launches one kernel, copies the results back, frees what it allocated and
// returns the HIP error code (0 = hipSuccess).  Op codes mirror tests/hostsim/hostsim.cpp.
#include "../../zk-light-client-implementation_amd/csrc/ed25519_verify.cuh"
#include "../../zk-light-client-implementation_amd/csrc/poseidon_gl.cuh"
#include "../../zk-light-client-implementation_amd/csrc/goldilocks_ntt_group.cuh"
#include "../../zk-light-client-implementation_amd/csrc/plonky2_gates.cuh"
#include "../../zk-light-client-implementation_amd/csrc/bn254_msm_lane.cuh"
#include "../../zk-light-client-implementation_amd/csrc/poseidon_bn254.cuh"
#include "../../zk-light-client-implementation_amd/csrc/bn254_pairing.cuh"
#include <hip/hip_runtime.h>

#define DS_BLOCK 128   // two waves per workgroup; the rolled Poseidon-gate evaluator sizes its LDS for at most P2_LAZY_THREADS lanes
static_assert(DS_BLOCK <= P2_LAZY_THREADS, "p2_eval_poseidon_lazy<V, 1> indexes its LDS array by threadIdx.x");

namespace {
struct dbuf {   // a device allocation, optionally filled from the host; freed on scope exit
    void *p = nullptr;
    hipError_t err;
    dbuf(size_t bytes, const void *src = nullptr) {
        err = hipMalloc(&p, bytes ? bytes : 8);
        if (err == hipSuccess && src && bytes) err = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
    ~dbuf() {
        if (p) (void)hipFree(p);
    }
    dbuf(const dbuf &) = delete;
    dbuf &operator=(const dbuf &) = delete;
    template <class T>
    T *as() const { return (T *)p; }
};
int ds_finish(void *host, const dbuf &d, size_t bytes) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && bytes) e = hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost);
    return (int)e;
}
}  // namespace
#define DS_OK(b) \
    if ((b).err != hipSuccess) return (int)(b).err
#define DS_LAUNCH(kernel, n, ...) hipLaunchKernelGGL(kernel, dim3(((n) + DS_BLOCK - 1) / DS_BLOCK), dim3(DS_BLOCK), 0, 0, __VA_ARGS__)
#define DS_LANE(i, n)                                   \
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x; \
    if (i >= (n)) return

// ------------------------------------------------------------------------------------------------ Goldilocks
__global__ void ds_gl_op_kernel(int op, const u64 *a, const u64 *b, u64 *out, u32 n) {
    DS_LANE(i, n);
    const u64 x = a[i], y = b[i];
    u64 r = 0;
    switch (op) {   // hostsim_gl_op
        case 0: r = gl_add(x, y); break;
        case 1: r = gl_sub(x, y); break;
        case 2: r = gl_mul(x, y); break;
        case 3: r = gl_inv(x); break;
        case 4: r = gl_reduce128(x, y); break;
        case 5: r = gl_root_of_unity((u32)x); break;
        case 6: r = gl_reduce128_loose(x, y); break;
        case 7: r = gl_add_lc(x, y); break;
        case 8: r = gl_mul_loose(x, y); break;
        case 9: r = gl_canonical(x); break;
    }
    out[i] = r;
}
// the exponent is a compile-time constant wherever the product calls gl_mul_2exp: one instantiation per exponent
template <u32 E>
ZKLC_D u64 ds_mul_2exp_const(u64 x) { return gl_mul_2exp(x, E); }
template <u32 E0>
ZKLC_D u64 ds_mul_2exp_dispatch(u64 x, u32 e) {   // e in [E0, E0 + 8)
    switch (e - E0) {
        case 0: return ds_mul_2exp_const<E0>(x);
        case 1: return ds_mul_2exp_const<E0 + 1>(x);
        case 2: return ds_mul_2exp_const<E0 + 2>(x);
        case 3: return ds_mul_2exp_const<E0 + 3>(x);
        case 4: return ds_mul_2exp_const<E0 + 4>(x);
        case 5: return ds_mul_2exp_const<E0 + 5>(x);
        case 6: return ds_mul_2exp_const<E0 + 6>(x);
        default: return ds_mul_2exp_const<E0 + 7>(x);
    }
}
// tuple i: x[i] * 2^e[i], e < 96; fixed != 0: through the constant-exponent instantiations, else the run-time form
__global__ void ds_gl_mul_2exp_kernel(const u64 *x, const u32 *e, u32 fixed, u64 *out, u32 n) {
    DS_LANE(i, n);
    const u32 ee = e[i];
    if (!fixed) {
        out[i] = gl_mul_2exp(x[i], ee);
        return;
    }
    u64 r;
    switch (ee >> 3) {
        case 0: r = ds_mul_2exp_dispatch<0>(x[i], ee); break;
        case 1: r = ds_mul_2exp_dispatch<8>(x[i], ee); break;
        case 2: r = ds_mul_2exp_dispatch<16>(x[i], ee); break;
        case 3: r = ds_mul_2exp_dispatch<24>(x[i], ee); break;
        case 4: r = ds_mul_2exp_dispatch<32>(x[i], ee); break;
        case 5: r = ds_mul_2exp_dispatch<40>(x[i], ee); break;
        case 6: r = ds_mul_2exp_dispatch<48>(x[i], ee); break;
        case 7: r = ds_mul_2exp_dispatch<56>(x[i], ee); break;
        case 8: r = ds_mul_2exp_dispatch<64>(x[i], ee); break;
        case 9: r = ds_mul_2exp_dispatch<72>(x[i], ee); break;
        case 10: r = ds_mul_2exp_dispatch<80>(x[i], ee); break;
        default: r = ds_mul_2exp_dispatch<88>(x[i], ee); break;
    }
    out[i] = r;
}
// tuple i: sum_j x[i * len + j] * y[i * len + j] through the 160-bit accumulator (hostsim_gl_acc)
__global__ void ds_gl_acc_kernel(const u64 *x, const u64 *y, u32 len, u64 *out, u32 n) {
    DS_LANE(i, n);
    gl_acc160 acc = {0, 0, 0};
    for (u32 j = 0; j < len; j++) gl_acc_mul(acc, x[(size_t)i * len + j], y[(size_t)i * len + j]);
    out[i] = gl_acc_reduce(acc);
}
// tuple i: sum_j x * k through gl_acc3 and the 22-bit limb table, normalised every `fold_every` terms (hostsim_gl_acc3)
__global__ void ds_gl_acc3_kernel(const u64 *x, const u64 *k, u32 len, u32 fold_every, u64 *out, u32 n) {
    DS_LANE(i, n);
    gl_acc3 acc = {0, 0, 0};
    u32 t6[6];
    for (u32 j = 0; j < len; j++) {
        if (fold_every && j && j % fold_every == 0) gl_acc3_normalize(acc);
        gl_limbs22(k[(size_t)i * len + j], t6);
        gl_acc3_mul(acc, x[(size_t)i * len + j], (const u32 *)t6);
    }
    out[i] = gl_acc3_reduce(acc);
}
__global__ void ds_gl2_op_kernel(int op, const u64 *a, const u64 *b, const u64 *e, u64 *out, u32 n) {
    DS_LANE(i, n);
    gl2 x = gl2_make(a[2 * i], a[2 * i + 1]), y = gl2_make(b[2 * i], b[2 * i + 1]), r;
    switch (op) {   // hostsim_gl2_op
        case 0: r = gl2_add(x, y); break;
        case 1: r = gl2_sub(x, y); break;
        case 2: r = gl2_mul(x, y); break;
        case 3: r = gl2_sqr(x); break;
        case 4: r = gl2_inv(x); break;
        case 5: r = gl2_pow(x, e[i]); break;
        default: r = gl2_make(0, 0);
    }
    out[2 * i] = r.a;
    out[2 * i + 1] = r.b;
}
// tuple i: the N products x[i * N + q] * t[i * N + q] through gl_mul_batch<N> (the asm statements of goldilocks_mul_asm.inc)
template <int N>
__global__ void ds_gl_mul_batch_kernel(const u64 *x, const u64 *t, u64 *out, u32 n) {
    DS_LANE(i, n);
    u64 a[N], b[N];
#pragma unroll
    for (int q = 0; q < N; q++) {
        a[q] = x[(size_t)i * N + q];
        b[q] = t[(size_t)i * N + q];
    }
    gl_mul_batch<N>(a, b);
#pragma unroll
    for (int q = 0; q < N; q++) out[(size_t)i * N + q] = a[q];
}
// tuple i: the N range products of x[i * N ..] through p2_range_products4<N> (loose results)
template <int N>
__global__ void ds_p2_range4_kernel(const u64 *x, u64 *out, u32 n) {
    DS_LANE(i, n);
    u64 a[N], r[N];
#pragma unroll
    for (int q = 0; q < N; q++) a[q] = x[(size_t)i * N + q];
    p2_range_products4<N>(a, r);
#pragma unroll
    for (int q = 0; q < N; q++) out[(size_t)i * N + q] = r[q];
}
// tuple i: one butterfly group on the 2^G values x[i * M ..] with the table t[i * (M - 1) ..].  ZP > 0: only the first M >> ZP
// values are taken, the others hold a poison value the group must not read.
template <int G, bool DIT, bool INV, int ZP>
__global__ void ds_gl_ntt_group_kernel(const u64 *x, const u64 *t, u64 *out, u32 n) {
    DS_LANE(i, n);
    constexpr int M = 1 << G;
    u64 a[M], tw[M - 1];
#pragma unroll
    for (int m = 0; m < M; m++) a[m] = m < (M >> ZP) ? x[(size_t)i * M + m] : 0xDEADBEEFDEADBEEFull;
#pragma unroll
    for (int m = 0; m < M - 1; m++) tw[m] = t[(size_t)i * (M - 1) + m];
    gl_ntt_group_regs<G, DIT, INV, ZP>(a, tw);
#pragma unroll
    for (int m = 0; m < M; m++) out[(size_t)i * M + m] = a[m];
}

// ------------------------------------------------------------------------------------------------ Poseidon-Goldilocks
// piece 0: pgl_gate_full_round<ASM>(s, layer); 1: pgl_gate_full_round_init<ASM>(s); 2: the 22 partial rounds + the constant layer
// behind them (pgl_asm_partial_rounds; the statement has no C++ twin, ASM only).  Loose states in, loose states out.
template <bool ASM>
__global__ void ds_pgl_piece_kernel(int piece, int layer, const u64 *in, u64 *out, u32 n) {
    DS_LANE(i, n);
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = in[(size_t)i * 12 + k];
    if (piece == 0) {
        pgl_gate_full_round<ASM>(s, layer);
    } else if (piece == 1) {
        pgl_gate_full_round_init<ASM>(s);
    } else {
#if defined(ZKLC_PGL_ASM)
        if constexpr (ASM) {
            u32 lo[12], hi[12];
#pragma unroll
            for (int k = 0; k < 12; k++) {
                lo[k] = (u32)s[k];
                hi[k] = (u32)(s[k] >> 32);
            }
            pgl_asm_partial_rounds(lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], lo[3], hi[3], lo[4], hi[4], lo[5], hi[5], lo[6], hi[6], lo[7],
                                   hi[7], lo[8], hi[8], lo[9], hi[9], lo[10], hi[10], lo[11], hi[11], PGL_ASM_PBLOCKS);
#pragma unroll
            for (int k = 0; k < 12; k++) s[k] = (u64)lo[k] | ((u64)hi[k] << 32);
        }
#endif
    }
#pragma unroll
    for (int k = 0; k < 12; k++) out[(size_t)i * 12 + k] = s[k];
}
__global__ void ds_poseidon_gl_permute_kernel(const u64 *in, u64 *out, u32 n) {
    DS_LANE(i, n);
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 12; k++) s[k] = in[(size_t)i * 12 + k];
    poseidon_gl_permute(s);
#pragma unroll
    for (int k = 0; k < 12; k++) out[(size_t)i * 12 + k] = s[k];
}
__global__ void ds_poseidon_gl_hash_kernel(const u64 *in, u32 len, u64 *out, u32 n) {
    DS_LANE(i, n);
    u64 o[4];
    poseidon_gl_hash_or_noop(in + (size_t)i * len, 1, len, o);
    for (int k = 0; k < 4; k++) out[(size_t)i * 4 + k] = o[k];
}
__global__ void ds_poseidon_gl_two_to_one_kernel(const u64 *l, const u64 *r, u64 *out, u32 n) {
    DS_LANE(i, n);
    u64 o[4];
    poseidon_gl_two_to_one(l + (size_t)i * 4, r + (size_t)i * 4, o);
    for (int k = 0; k < 4; k++) out[(size_t)i * 4 + k] = o[k];
}

// ------------------------------------------------------------------------------------------------ gate evaluators
// the limb table of the powers of the alphas, as hostsim_p2_eval_gate builds it: tab[c][6 k ..] = gl_limbs22(alpha_c^k), k < 1024
__global__ void ds_alpha_table_kernel(const u64 *alpha, u32 nch, u32 *tab) {
    const u32 c = threadIdx.x;
    if (c >= P2_MAX_CH) return;
    u64 a = c < nch ? alpha[c] : 0, pw = 1;
    for (int k = 0; k < 1024; k++) {
        gl_limbs22(pw, tab + ((size_t)c * 1024 + k) * 6);
        pw = gl_mul(pw, a);
    }
}
struct ds_pih {
    u64 v[4];
};
// tuple i: sum_k alpha_c^k constraint_k of ONE gate on the wires wires[i * n_wires ..] (stride 1) and the constants
// consts[i * n_consts ..].  TYPE is a template argument as in the quotient kernels (plonky2_prover.hip): the evaluator of one gate type
// per kernel; 100 / 101 / 110 = the A/B forms of the Poseidon gate.
template <u32 TYPE>
__global__ void ds_p2_eval_gate_kernel(p2_gate g, const u64 *extra, const u64 *wires, u32 n_wires, const u64 *consts, u32 n_consts,
                                       ds_pih pih, const u32 *tab, u32 nch, u64 *out_acc, u32 n) {
    DS_LANE(i, n);
    g.type = TYPE;
    p2_vars v;
    v.wires = wires + (size_t)i * n_wires;
    v.consts = TYPE >= P2_POSEIDON_LAZY ? v.wires : consts + (size_t)i * n_consts;
    v.stride = 1;
    v.p = 0;
    v.nsel = 0;
    for (int k = 0; k < 4; k++) v.pih[k] = pih.v[k];
    p2_consumer out;
    out.nch = (int)nch;
    for (int c = 0; c < P2_MAX_CH; c++) out.apow[c] = (gl_ktab *)(tab + (size_t)c * 1024 * 6);
    out.reset(0);
    if constexpr (TYPE == P2_POSEIDON_LOOSE)
        p2_eval_poseidon_loose(v, out);
    else if constexpr (TYPE >= P2_POSEIDON_LAZY)
        p2_eval_poseidon_lazy<p2_vars, TYPE - P2_POSEIDON_LAZY>(v, out);
    else
        p2_eval_gate(g, v, extra, out);
#pragma unroll
    for (int c = 0; c < P2_MAX_CH; c++)
        if (c < (int)nch) out_acc[(size_t)i * nch + c] = out.result(c);
}

// ------------------------------------------------------------------------------------------------ BN254 (gnark Montgomery words)
typedef ec_xyzz<FpField> g1_xyzz;
typedef ec_xyzz<Fp2Field> g2_xyzz;

__global__ void ds_fp_op_kernel(int op, const u32 *a, const u32 *b, u32 *out, u32 n) {
    DS_LANE(i, n);
    fp xl = fp_from_gnark(a + 8 * (size_t)i), yl = fp_from_gnark(b + 8 * (size_t)i), x = fp_reduce(xl), y = fp_reduce(yl), r;
    switch (op) {   // hostsim_fp_op
        case 0: r = fp_add(x, y); break;
        case 1: r = fp_sub(x, y); break;
        case 2: r = fp_mul(xl, yl); break;
        case 3: r = fp_sqr(xl); break;
        case 4: r = fp_inv(x); break;
        case 5: r = fp_mul(fp_sub(fp_sub(fp_mul(x, y), x), fp_dbl(y)), fp_add(fp_add(x, y), fp_mul(x, x))); break;
        default: r = fp_zero();
    }
    fp_to_gnark(out + 8 * (size_t)i, r);
}
__global__ void ds_fp_wred_kernel(const i32 *limbs, i32 *out_limbs, u32 *out_words, u32 n) {
    DS_LANE(i, n);
    fp a;
    for (int k = 0; k < 10; k++) a.v[k] = limbs[10 * (size_t)i + k];
    fp r = fp_wred(a);
    for (int k = 0; k < 10; k++) out_limbs[10 * (size_t)i + k] = r.v[k];
    fp_freeze_words(out_words + 8 * (size_t)i, r);
}
__global__ void ds_f12_op_kernel(int op, const u32 *a96, const u32 *b96, u32 *out96, u32 n) {
    DS_LANE(i, n);
    fp12 a, b, r;
    fp2 *xa[6] = {&a.c0.b0, &a.c0.b1, &a.c0.b2, &a.c1.b0, &a.c1.b1, &a.c1.b2};
    fp2 *xb[6] = {&b.c0.b0, &b.c0.b1, &b.c0.b2, &b.c1.b0, &b.c1.b1, &b.c1.b2};
    for (int k = 0; k < 6; k++) {
        *xa[k] = fp2_reduce(fp2_from_gnark(a96 + 96 * (size_t)i + 16 * k));
        *xb[k] = fp2_reduce(fp2_from_gnark(b96 + 96 * (size_t)i + 16 * k));
    }
    switch (op) {   // hostsim_f12_op
        case 0: r = f12_mul(a, b); break;
        case 1: r = f12_sqr(a); break;
        case 2: r = f12_inv(a); break;
        case 3: r = f12_frobenius(a, 1); break;
        case 4: r = f12_frobenius(a, 2); break;
        default: r = f12_conj(a);
    }
    f12_to_gnark(out96 + 96 * (size_t)i, r);
}
__global__ void ds_g1_op_kernel(int op, const u32 *p16, const u32 *pinf, const u32 *q16, const u32 *qinf, const u32 *reps, u32 *out16,
                                u32 *inf_out, u32 n) {
    DS_LANE(i, n);
    const u32 *pp = p16 + 16 * (size_t)i, *qq = q16 + 16 * (size_t)i;
    const u32 qi = qinf[i];
    fp qx = fp_from_gnark(qq), qy = fp_from_gnark(qq + 8);      // Q stays lazy, as in the MSM bucket loop
    g1_xyzz a, r;
    a.X = fp_reduce(fp_from_gnark(pp));
    a.Y = fp_reduce(fp_from_gnark(pp + 8));
    a.ZZ = pinf[i] ? fp_zero() : FpField::one();
    a.ZZZ = a.ZZ;
    switch (op) {   // hostsim_g1_op
        case 0: r = qi ? a : ec_add_affine<FpField>(a, qx, qy, 0); break;
        case 1: r = qi ? a : ec_add_affine<FpField>(a, qx, qy, 1); break;
        case 2: r = ec_double(a); break;
        case 3: { g1_xyzz s = qi ? a : ec_add_affine<FpField>(a, qx, qy, 0); r = ec_add(s, s); break; }
        case 4: { r = a; for (u32 k = 0; k < reps[i]; k++) r = ec_add_affine<FpField>(r, qx, qy, 0); break; }
        case 5: {
            g1_xyzz s;
            s.X = fp_reduce(qx);
            s.Y = fp_reduce(qy);
            s.ZZ = qi ? fp_zero() : FpField::one();
            s.ZZZ = s.ZZ;
            r = ec_add(a, s);
            break;
        }
        default: r = ec_infinity<FpField>();
    }
    inf_out[i] = ec_to_affine_gnark(out16 + 16 * (size_t)i, r);
}
__global__ void ds_g2_op_kernel(int op, const u32 *p32, const u32 *q32, u32 *out32, u32 *inf_out, u32 n) {
    DS_LANE(i, n);
    const u32 *pp = p32 + 32 * (size_t)i, *qq = q32 + 32 * (size_t)i;
    g2_xyzz a, r;
    a.X = fp2_reduce(fp2_from_gnark(pp));
    a.Y = fp2_reduce(fp2_from_gnark(pp + 16));
    a.ZZ = a.ZZZ = fp2_one();
    fp2 qx = fp2_from_gnark(qq), qy = fp2_from_gnark(qq + 16);
    switch (op) {   // hostsim_g2_op
        case 0: r = ec_add_affine<Fp2Field>(a, qx, qy, 0); break;
        case 1: r = ec_add_affine<Fp2Field>(a, qx, qy, 1); break;
        case 2: r = ec_double(a); break;
        default: { g2_xyzz s = ec_add_affine<Fp2Field>(a, qx, qy, 0); r = ec_add(s, a); }
    }
    inf_out[i] = ec_to_affine_gnark(out32 + 32 * (size_t)i, r);
}
// states as 4 x 8 words, regular form.  coop = 0: one lane per permutation; 1: the four-lane form, one state word per lane with the
// real quad broadcast (idle quads of the last wave redo the last state, as in the product's kernels)
__global__ void ds_poseidon_bn254_permute_kernel(u32 coop, const u32 *in, u32 *out, u32 n) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (!coop) {
        if (t >= n) return;
        fr s[4];
        for (int k = 0; k < 4; k++) s[k] = fr_from_regular(in + 32 * (size_t)t + 8 * k);
        poseidon_bn254_permute(s);
        for (int k = 0; k < 4; k++) fr_to_regular(out + 32 * (size_t)t + 8 * k, s[k]);
        return;
    }
    u32 i = t >> 2, q = t & 3;
    const bool live = i < n;
    if (!live) i = n - 1;
    fr s = fr_from_regular(in + 32 * (size_t)i + 8 * q);
    poseidon_bn254_permute_coop(s, q);
    if (live) fr_to_regular(out + 32 * (size_t)i + 8 * q, s);
}

// ------------------------------------------------------------------------------------------------ Ed25519
__global__ void ds_fe_op_kernel(int op, const u32 *a, const u32 *b, u32 *out, u32 n) {
    DS_LANE(i, n);
    fe x = fe_from_words(a + 8 * (size_t)i), y = fe_from_words(b + 8 * (size_t)i), r;  // inputs < 2^255
    switch (op) {   // hostsim_fe_op
        case 0: r = fe_add(x, y); break;
        case 1: r = fe_sub(x, y); break;
        case 2: r = fe_mul(x, y); break;
        case 3: r = fe_sqr(x); break;
        case 4: r = fe_invert(x); break;
        case 5: r = fe_pow22523(x); break;
        case 6: r = fe_freeze(x); break;
        case 7: r = fe_sqr2(x); break;
        case 8: {  // three-term lazy inputs built from REDUCED values
            fe xr = fe_mul(x, fe_one()), yr = fe_mul(y, fe_one());
            r = fe_mul(fe_add(fe_add(xr, yr), xr), fe_sub(fe_sub(yr, xr), xr));
            break;
        }
        default: r = fe_zero();
    }
    fe_freeze_words(out + 8 * (size_t)i, r);  // canonical
}
__global__ void ds_sc_reduce512_kernel(const u32 *x, u32 *out, u32 n) {
    DS_LANE(i, n);
    u32 w[16], o[8];
    for (int k = 0; k < 16; k++) w[k] = x[16 * (size_t)i + k];
    sc_reduce512(o, w);
    for (int k = 0; k < 8; k++) out[8 * (size_t)i + k] = o[k];
}
__global__ void ds_sc_is_canonical_kernel(const u32 *x, u32 *out, u32 n) {
    DS_LANE(i, n);
    u32 w[8];
    for (int k = 0; k < 8; k++) w[k] = x[8 * (size_t)i + k];
    out[i] = sc_is_canonical(w);
}
__global__ void ds_decompress_compress_kernel(const u32 *in, u32 *out, u32 *ok, u32 n) {
    DS_LANE(i, n);
    u32 w[8], o[8];
    for (int k = 0; k < 8; k++) w[k] = in[8 * (size_t)i + k];
    ge_p3 p;
    ok[i] = ge_decompress(p, w);
    ge_compress(o, p);
    for (int k = 0; k < 8; k++) out[8 * (size_t)i + k] = o[k];
}

extern "C" {

int devsim_gl_op(int op, const u64 *a, const u64 *b, u64 *out, u32 n) {
    if (!n) return 0;
    dbuf da(8ull * n, a), db(8ull * n, b), dout(8ull * n);
    DS_OK(da); DS_OK(db); DS_OK(dout);
    DS_LAUNCH(ds_gl_op_kernel, n, op, da.as<u64>(), db.as<u64>(), dout.as<u64>(), n);
    return ds_finish(out, dout, 8ull * n);
}
int devsim_gl_mul_2exp(const u64 *x, const u32 *e, u32 fixed, u64 *out, u32 n) {
    if (!n) return 0;
    for (u32 i = 0; i < n; i++)
        if (e[i] >= 96) return (int)hipErrorInvalidValue;
    dbuf dx(8ull * n, x), de(4ull * n, e), dout(8ull * n);
    DS_OK(dx); DS_OK(de); DS_OK(dout);
    DS_LAUNCH(ds_gl_mul_2exp_kernel, n, dx.as<u64>(), de.as<u32>(), fixed, dout.as<u64>(), n);
    return ds_finish(out, dout, 8ull * n);
}
int devsim_gl_acc(const u64 *x, const u64 *y, u32 len, u64 *out, u32 n) {
    if (!n) return 0;
    dbuf dx(8ull * n * len, x), dy(8ull * n * len, y), dout(8ull * n);
    DS_OK(dx); DS_OK(dy); DS_OK(dout);
    DS_LAUNCH(ds_gl_acc_kernel, n, dx.as<u64>(), dy.as<u64>(), len, dout.as<u64>(), n);
    return ds_finish(out, dout, 8ull * n);
}
int devsim_gl_acc3(const u64 *x, const u64 *k, u32 len, u32 fold_every, u64 *out, u32 n) {
    if (!n) return 0;
    dbuf dx(8ull * n * len, x), dk(8ull * n * len, k), dout(8ull * n);
    DS_OK(dx); DS_OK(dk); DS_OK(dout);
    DS_LAUNCH(ds_gl_acc3_kernel, n, dx.as<u64>(), dk.as<u64>(), len, fold_every, dout.as<u64>(), n);
    return ds_finish(out, dout, 8ull * n);
}
int devsim_gl2_op(int op, const u64 *a, const u64 *b, const u64 *e, u64 *out, u32 n) {
    if (!n) return 0;
    dbuf da(16ull * n, a), db(16ull * n, b), de(8ull * n, e), dout(16ull * n);
    DS_OK(da); DS_OK(db); DS_OK(de); DS_OK(dout);
    DS_LAUNCH(ds_gl2_op_kernel, n, op, da.as<u64>(), db.as<u64>(), de.as<u64>(), dout.as<u64>(), n);
    return ds_finish(out, dout, 16ull * n);
}
int devsim_gl_mul_batch(u32 width, const u64 *x, const u64 *t, u64 *out, u32 n) {
    if (!n) return 0;
    const size_t bytes = 8ull * n * width;
    dbuf dx(bytes, x), dt(bytes, t), dout(bytes);
    DS_OK(dx); DS_OK(dt); DS_OK(dout);
#define DS_W(N) \
    case N: DS_LAUNCH(ds_gl_mul_batch_kernel<N>, n, dx.as<u64>(), dt.as<u64>(), dout.as<u64>(), n); break;
    switch (width) {
        DS_W(1) DS_W(2) DS_W(3) DS_W(4) DS_W(5) DS_W(6) DS_W(7) DS_W(8) DS_W(15)
        default: return (int)hipErrorInvalidValue;
    }
#undef DS_W
    return ds_finish(out, dout, bytes);
}
int devsim_p2_range_products4(u32 width, const u64 *x, u64 *out, u32 n) {
    if (!n) return 0;
    const size_t bytes = 8ull * n * width;
    dbuf dx(bytes, x), dout(bytes);
    DS_OK(dx); DS_OK(dout);
#define DS_W(N) \
    case N: DS_LAUNCH(ds_p2_range4_kernel<N>, n, dx.as<u64>(), dout.as<u64>(), n); break;
    switch (width) {   // 1..9: every split into batches of four / three / two / one; 12, 16, 18: the other widths the evaluators use
        DS_W(1) DS_W(2) DS_W(3) DS_W(4) DS_W(5) DS_W(6) DS_W(7) DS_W(8) DS_W(9) DS_W(12) DS_W(16) DS_W(18)
        default: return (int)hipErrorInvalidValue;
    }
#undef DS_W
    return ds_finish(out, dout, bytes);
}
// g = 1..4; zp = 0 (every order and direction) or 3 (the zero-padded DIF forward groups goldilocks.hip instantiates: g = 3, 4)
int devsim_gl_ntt_group(u32 g, u32 dit, u32 inverse, u32 zp, const u64 *x, const u64 *t, u64 *out, u32 n) {
    if (!n) return 0;
    if (g < 1 || g > 4) return (int)hipErrorInvalidValue;
    const size_t M = (size_t)1 << g;
    dbuf dx(8ull * n * M, x), dt(8ull * n * (M - 1), t), dout(8ull * n * M);
    DS_OK(dx); DS_OK(dt); DS_OK(dout);
#define DS_GO(G, DIT, INV, ZP) DS_LAUNCH((ds_gl_ntt_group_kernel<G, DIT, INV, ZP>), n, dx.as<u64>(), dt.as<u64>(), dout.as<u64>(), n)
#define DS_G(G)                                      \
    case G:                                          \
        if (dit && inverse) DS_GO(G, true, true, 0); \
        else if (dit) DS_GO(G, true, false, 0);      \
        else if (inverse) DS_GO(G, false, true, 0);  \
        else DS_GO(G, false, false, 0);              \
        break;
    if (zp == 3 && !dit && !inverse && g == 3) DS_GO(3, false, false, 3);
    else if (zp == 3 && !dit && !inverse && g == 4) DS_GO(4, false, false, 3);
    else if (zp) return (int)hipErrorInvalidValue;
    else
        switch (g) { DS_G(1) DS_G(2) DS_G(3) DS_G(4) }
#undef DS_G
#undef DS_GO
    return ds_finish(out, dout, 8ull * n * M);
}

int devsim_pgl_piece(u32 piece, u32 layer, u32 use_asm, const u64 *in, u64 *out, u32 n) {
    if (!n) return 0;
    if (piece > 2 || layer > 7 || (piece == 2 && !use_asm)) return (int)hipErrorInvalidValue;
    dbuf din(96ull * n, in), dout(96ull * n);
    DS_OK(din); DS_OK(dout);
    if (use_asm) DS_LAUNCH(ds_pgl_piece_kernel<true>, n, (int)piece, (int)layer, din.as<u64>(), dout.as<u64>(), n);
    else DS_LAUNCH(ds_pgl_piece_kernel<false>, n, (int)piece, (int)layer, din.as<u64>(), dout.as<u64>(), n);
    return ds_finish(out, dout, 96ull * n);
}
int devsim_poseidon_gl_permute(const u64 *in, u64 *out, u32 n) {
    if (!n) return 0;
    dbuf din(96ull * n, in), dout(96ull * n);
    DS_OK(din); DS_OK(dout);
    DS_LAUNCH(ds_poseidon_gl_permute_kernel, n, din.as<u64>(), dout.as<u64>(), n);
    return ds_finish(out, dout, 96ull * n);
}
int devsim_poseidon_gl_hash(const u64 *in, u32 len, u64 *out4, u32 n) {
    if (!n) return 0;
    dbuf din(8ull * n * len, in), dout(32ull * n);
    DS_OK(din); DS_OK(dout);
    DS_LAUNCH(ds_poseidon_gl_hash_kernel, n, din.as<u64>(), len, dout.as<u64>(), n);
    return ds_finish(out4, dout, 32ull * n);
}
int devsim_poseidon_gl_two_to_one(const u64 *l, const u64 *r, u64 *out4, u32 n) {
    if (!n) return 0;
    dbuf dl(32ull * n, l), dr(32ull * n, r), dout(32ull * n);
    DS_OK(dl); DS_OK(dr); DS_OK(dout);
    DS_LAUNCH(ds_poseidon_gl_two_to_one_kernel, n, dl.as<u64>(), dr.as<u64>(), dout.as<u64>(), n);
    return ds_finish(out4, dout, 32ull * n);
}

// wires: n x n_wires, consts: n x n_consts (n_consts >= 1; unused columns zero), extra: n_extra words (>= 1), alpha: nch values,
// acc_out: n x nch
int devsim_p2_eval_gate(u32 type, const u32 *params, const u64 *extra, u32 n_extra, const u64 *wires, u32 n_wires, const u64 *consts,
                        u32 n_consts, const u64 *pih, const u64 *alpha, u32 nch, u64 *acc_out, u32 n) {
    if (!n) return 0;
    if (!nch || nch > P2_MAX_CH || !n_wires || !n_consts || !n_extra) return (int)hipErrorInvalidValue;
    p2_gate g;
    g.type = type;
    for (int k = 0; k < 4; k++) g.p[k] = params[k];
    g.selector_index = g.group_start = g.group_end = g.extra_off = 0;
    ds_pih ph;
    for (int k = 0; k < 4; k++) ph.v[k] = pih[k];
    dbuf dex(8ull * n_extra, extra), dw(8ull * n * n_wires, wires), dc(8ull * n * n_consts, consts), da(8ull * nch, alpha),
        dtab(4ull * P2_MAX_CH * 1024 * 6), dout(8ull * n * nch);
    DS_OK(dex); DS_OK(dw); DS_OK(dc); DS_OK(da); DS_OK(dtab); DS_OK(dout);
    hipLaunchKernelGGL(ds_alpha_table_kernel, dim3(1), dim3(64), 0, 0, da.as<u64>(), nch, dtab.as<u32>());
#define DS_T(T)                                                                                                                     \
    case T:                                                                                                                         \
        DS_LAUNCH(ds_p2_eval_gate_kernel<T>, n, g, dex.as<u64>(), dw.as<u64>(), n_wires, dc.as<u64>(), n_consts, ph, dtab.as<u32>(), \
                  nch, dout.as<u64>(), n);                                                                                          \
        break;
    switch (type) {
        DS_T(P2_NOOP) DS_T(P2_CONSTANT) DS_T(P2_PUBLIC_INPUT) DS_T(P2_ARITHMETIC) DS_T(P2_ARITHMETIC_EXT) DS_T(P2_MUL_EXT)
        DS_T(P2_BASE_SUM) DS_T(P2_POSEIDON) DS_T(P2_POSEIDON_MDS) DS_T(P2_RANDOM_ACCESS) DS_T(P2_REDUCING) DS_T(P2_REDUCING_EXT)
        DS_T(P2_EXPONENTIATION) DS_T(P2_COSET_INTERPOLATION) DS_T(P2_U32_ARITHMETIC) DS_T(P2_U32_ADD_MANY) DS_T(P2_U32_SUBTRACTION)
        DS_T(P2_U32_RANGE_CHECK) DS_T(P2_COMPARISON) DS_T(P2_U32_INTERLEAVE) DS_T(P2_UNINTERLEAVE_TO_U32) DS_T(P2_UNINTERLEAVE_TO_B32)
        DS_T(P2_POSEIDON_LAZY) DS_T(P2_POSEIDON_LAZY + 1) DS_T(P2_POSEIDON_LOOSE)
        default: return (int)hipErrorInvalidValue;
    }
#undef DS_T
    return ds_finish(acc_out, dout, 8ull * n * nch);
}

int devsim_fp_op(int op, const u32 *a, const u32 *b, u32 *out, u32 n) {
    if (!n) return 0;
    dbuf da(32ull * n, a), db(32ull * n, b), dout(32ull * n);
    DS_OK(da); DS_OK(db); DS_OK(dout);
    DS_LAUNCH(ds_fp_op_kernel, n, op, da.as<u32>(), db.as<u32>(), dout.as<u32>(), n);
    return ds_finish(out, dout, 32ull * n);
}
int devsim_fp_wred(const i32 *limbs, i32 *out_limbs, u32 *out_words, u32 n) {
    if (!n) return 0;
    dbuf dl(40ull * n, limbs), dol(40ull * n), dow(32ull * n);
    DS_OK(dl); DS_OK(dol); DS_OK(dow);
    DS_LAUNCH(ds_fp_wred_kernel, n, dl.as<i32>(), dol.as<i32>(), dow.as<u32>(), n);
    int e = ds_finish(out_limbs, dol, 40ull * n);
    return e ? e : (int)hipMemcpy(out_words, dow.p, 32ull * n, hipMemcpyDeviceToHost);
}
int devsim_f12_op(int op, const u32 *a96, const u32 *b96, u32 *out96, u32 n) {
    if (!n) return 0;
    dbuf da(384ull * n, a96), db(384ull * n, b96), dout(384ull * n);
    DS_OK(da); DS_OK(db); DS_OK(dout);
    DS_LAUNCH(ds_f12_op_kernel, n, op, da.as<u32>(), db.as<u32>(), dout.as<u32>(), n);
    return ds_finish(out96, dout, 384ull * n);
}
int devsim_g1_op(int op, const u32 *p16, const u32 *pinf, const u32 *q16, const u32 *qinf, const u32 *reps, u32 *out16, u32 *inf_out,
                 u32 n) {
    if (!n) return 0;
    dbuf dp(64ull * n, p16), dpi(4ull * n, pinf), dq(64ull * n, q16), dqi(4ull * n, qinf), dr(4ull * n, reps), dout(64ull * n), dinf(4ull * n);
    DS_OK(dp); DS_OK(dpi); DS_OK(dq); DS_OK(dqi); DS_OK(dr); DS_OK(dout); DS_OK(dinf);
    DS_LAUNCH(ds_g1_op_kernel, n, op, dp.as<u32>(), dpi.as<u32>(), dq.as<u32>(), dqi.as<u32>(), dr.as<u32>(), dout.as<u32>(), dinf.as<u32>(), n);
    int e = ds_finish(out16, dout, 64ull * n);
    return e ? e : (int)hipMemcpy(inf_out, dinf.p, 4ull * n, hipMemcpyDeviceToHost);
}
int devsim_g2_op(int op, const u32 *p32, const u32 *q32, u32 *out32, u32 *inf_out, u32 n) {
    if (!n) return 0;
    dbuf dp(128ull * n, p32), dq(128ull * n, q32), dout(128ull * n), dinf(4ull * n);
    DS_OK(dp); DS_OK(dq); DS_OK(dout); DS_OK(dinf);
    DS_LAUNCH(ds_g2_op_kernel, n, op, dp.as<u32>(), dq.as<u32>(), dout.as<u32>(), dinf.as<u32>(), n);
    int e = ds_finish(out32, dout, 128ull * n);
    return e ? e : (int)hipMemcpy(inf_out, dinf.p, 4ull * n, hipMemcpyDeviceToHost);
}
int devsim_poseidon_bn254_permute(u32 coop, const u32 *in, u32 *out, u32 n) {
    if (!n) return 0;
    dbuf din(128ull * n, in), dout(128ull * n);
    DS_OK(din); DS_OK(dout);
    DS_LAUNCH(ds_poseidon_bn254_permute_kernel, coop ? 4 * (size_t)n : n, coop, din.as<u32>(), dout.as<u32>(), n);
    return ds_finish(out, dout, 128ull * n);
}

int devsim_fe_op(int op, const u32 *a, const u32 *b, u32 *out, u32 n) {
    if (!n) return 0;
    dbuf da(32ull * n, a), db(32ull * n, b), dout(32ull * n);
    DS_OK(da); DS_OK(db); DS_OK(dout);
    DS_LAUNCH(ds_fe_op_kernel, n, op, da.as<u32>(), db.as<u32>(), dout.as<u32>(), n);
    return ds_finish(out, dout, 32ull * n);
}
int devsim_sc_reduce512(const u32 *x, u32 *out, u32 n) {
    if (!n) return 0;
    dbuf dx(64ull * n, x), dout(32ull * n);
    DS_OK(dx); DS_OK(dout);
    DS_LAUNCH(ds_sc_reduce512_kernel, n, dx.as<u32>(), dout.as<u32>(), n);
    return ds_finish(out, dout, 32ull * n);
}
int devsim_sc_is_canonical(const u32 *x, u32 *out, u32 n) {
    if (!n) return 0;
    dbuf dx(32ull * n, x), dout(4ull * n);
    DS_OK(dx); DS_OK(dout);
    DS_LAUNCH(ds_sc_is_canonical_kernel, n, dx.as<u32>(), dout.as<u32>(), n);
    return ds_finish(out, dout, 4ull * n);
}
int devsim_decompress_compress(const u32 *in, u32 *out, u32 *ok, u32 n) {
    if (!n) return 0;
    dbuf din(32ull * n, in), dout(32ull * n), dok(4ull * n);
    DS_OK(din); DS_OK(dout); DS_OK(dok);
    DS_LAUNCH(ds_decompress_compress_kernel, n, din.as<u32>(), dout.as<u32>(), dok.as<u32>(), n);
    int e = ds_finish(out, dout, 32ull * n);
    return e ? e : (int)hipMemcpy(ok, dok.p, 4ull * n, hipMemcpyDeviceToHost);
}

}  // extern "C"
