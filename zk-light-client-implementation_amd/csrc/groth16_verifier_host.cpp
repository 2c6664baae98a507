// Groth16 verifier, host part (plain C++): validation of a verifying key, the fixed-base table of its K points, and the
// host-only batch path -- the lane functions of groth16_verify.cuh compiled with the host compiler, one proof per task.
#include "groth16_verifier_host.h"
#include "plonky2_verifier_host.h"   // p2v_parallel_for
#include <new>
#include <string.h>

static bool g16_read_fp(const uint64_t *w, fp &out, bool &zero) {
    u32 w32[8];
    memcpy(w32, w, 32);
    zero = g16_words_zero(w32);
    if (g16_words_ge_p(w32)) return false;
    out = fp_reduce(fp_from_gnark(w32));
    return true;
}
// affine G1 in gnark's layout: coordinates reduced, on the curve; (0, 0) = infinity
static bool g16_read_g1(const uint64_t *w, fp &x, fp &y, bool &inf) {
    bool zx, zy;
    if (!g16_read_fp(w, x, zx) || !g16_read_fp(w + 4, y, zy)) return false;
    inf = zx && zy;
    return inf || g16_g1_on_curve(x, y);
}
// affine G2: reduced, finite, on the twist, in the r-torsion subgroup
static bool g16_read_g2(const g16_key &k, const uint64_t *w, fp2 &x, fp2 &y) {
    bool z[4];
    if (!g16_read_fp(w, x.c0, z[0]) || !g16_read_fp(w + 4, x.c1, z[1]) || !g16_read_fp(w + 8, y.c0, z[2]) || !g16_read_fp(w + 12, y.c1, z[3]))
        return false;
    if (z[0] && z[1] && z[2] && z[3]) return false;
    return g16_g2_on_curve(k, x, y) && g16_g2_in_subgroup(x, y);
}

// rows d 16^w P, d = 1..15, w = 0..63, affine: 960 additions / doublings, one inversion (Montgomery's trick)
static void g16_build_rows(const fp &x, const fp &y, g16_tab_entry *out) {
    const u32 N = G16_WINDOWS * G16_ROW;
    std::vector<g16_g1> pts(N);
    g16_g1 base;
    base.X = x;
    base.Y = y;
    base.ZZ = base.ZZZ = FpField::one();
    for (u32 w = 0; w < G16_WINDOWS; w++) {
        pts[w * G16_ROW] = base;
        for (u32 d = 2; d <= G16_ROW; d++) pts[w * G16_ROW + d - 1] = ec_add<FpField>(pts[w * G16_ROW + d - 2], base);
        base = ec_double<FpField>(pts[w * G16_ROW + 7]);   // 16 * 16^w P
    }
    // z_i = ZZ_i ZZZ_i; prefix products, one inversion, back substitution
    std::vector<fp> z(N), pre(N);
    for (u32 i = 0; i < N; i++) {
        z[i] = fp_mul(pts[i].ZZ, pts[i].ZZZ);
        pre[i] = i ? fp_mul(pre[i - 1], z[i]) : z[i];
    }
    fp inv = fp_inv(pre[N - 1]);
    for (u32 i = N; i-- > 0;) {
        fp zi = i ? fp_mul(inv, pre[i - 1]) : inv;         // 1 / (ZZ ZZZ)
        inv = fp_mul(inv, z[i]);
        out[i].x = fp_mul(pts[i].X, fp_mul(zi, pts[i].ZZZ));   // X / ZZ
        out[i].y = fp_mul(pts[i].Y, fp_mul(zi, pts[i].ZZ));    // Y / ZZZ
    }
}

// constants of the twist equation and of the Fp2 square root, from the field code itself
const g16_key &g16_key_constants() {
    static const g16_key key = [] {
        g16_key k;
        memset(&k, 0, sizeof(k));
        const u32 nine[8] = {9, 0, 0, 0, 0, 0, 0, 0}, two[8] = {2, 0, 0, 0, 0, 0, 0, 0};
        const fp three = FP_THREE, one = FP_ONE;
        fp2 xi, t3;
        xi.c0 = g16_fp_from_words(nine);
        xi.c1 = one;
        t3.c0 = three;
        t3.c1 = fp_zero();
        k.twist_b = fp2_reduce(fp2_mul(t3, fp2_inv(xi)));
        k.half = fp_inv(g16_fp_from_words(two));
        return k;
    }();
    return key;
}

extern "C" int32_t zklc_groth16_verifier_create(zklc_ctx *, const uint64_t *alpha1, const uint64_t *beta2, const uint64_t *gamma2,
                                                const uint64_t *delta2, const uint64_t *K, uint32_t n_public,
                                                zklc_groth16_verifier **out) {
    if (!alpha1 || !beta2 || !gamma2 || !delta2 || !K || !out || n_public > G16_MAX_PUBLIC) return ZKLC_ERR_INVALID_ARG;
    *out = nullptr;
    uint64_t entries;
    if (!g16_mul_ok((uint64_t)n_public, (uint64_t)G16_WINDOWS * G16_ROW, &entries)) return ZKLC_ERR_INVALID_ARG;
    zklc_groth16_verifier *v = new (std::nothrow) zklc_groth16_verifier();
    if (!v) return ZKLC_ERR_OOM;
    g16_key &k = v->key;
    k = g16_key_constants();
    k.n_public = n_public;
    bool ok = true, inf = false;
    fp ax, ay;
    ok = g16_read_g1(alpha1, ax, ay, inf) && !inf;
    if (ok) memcpy(k.alpha, alpha1, 64);
    const uint64_t *g2s[3] = {delta2, gamma2, beta2};
    for (int i = 0; i < 3 && ok; i++) {
        fp2 x, y;
        ok = g16_read_g2(k, g2s[i], x, y);
        if (!ok) break;
        fp2_to_gnark(k.neg_g2[i], x);
        fp2_to_gnark(k.neg_g2[i] + 16, fp2_neg(y));
    }
    try {
        v->k_inf.assign(((size_t)n_public + 1 + 3) & ~(size_t)3, 0);
        v->tab.resize((size_t)entries);
    } catch (const std::bad_alloc &) {
        delete v;
        return ZKLC_ERR_OOM;
    }
    std::vector<fp> kx(n_public + 1), ky(n_public + 1);
    for (uint32_t i = 0; i <= n_public && ok; i++) {
        ok = g16_read_g1(K + 8 * (size_t)i, kx[i], ky[i], inf);
        v->k_inf[i] = inf;
    }
    if (!ok) {
        delete v;
        return ZKLC_ERR_INVALID_ARG;
    }
    k.k0_inf = v->k_inf[0];
    k.k0x = kx[0];
    k.k0y = ky[0];
    p2v_parallel_for(n_public, 16, [&](uint64_t i) {
        if (!v->k_inf[i + 1]) g16_build_rows(kx[i + 1], ky[i + 1], v->tab.data() + i * G16_WINDOWS * G16_ROW);
    });
    *out = v;
    return ZKLC_OK;
}

// one proof on the host: the same lane functions in the order the kernels run them
static int32_t g16_verify_one_host(const zklc_groth16_verifier *v, const uint8_t *proof, const uint64_t *inputs, uint32_t compressed) {
    u32 g1[4 * 16], g2[4 * 32];
    u32 st = g16_validate_lane(v->key, proof, compressed, g1, g1 + 16, g2);
    if (st != G16_OK) return (int32_t)st;
    g16_g1 sum = g16_fold_lane(v->tab.data(), v->k_inf.data(), inputs, v->key.n_public, 0, 1);
    g16_fold_finish(v->key, sum, g1 + 32);
    memcpy(g1 + 48, v->key.alpha, 64);
    memcpy(g2 + 32, v->key.neg_g2, 3 * 128);
    return g16_pairing_is_one(g1, g2) ? ZKLC_G16_OK : ZKLC_G16_PAIRING;
}

extern "C" int32_t zklc_groth16_verify_batch_host(zklc_groth16_verifier *v, const uint8_t *proofs, const uint64_t *public_inputs,
                                                  uint64_t n, uint32_t nthreads, uint32_t flags, int32_t *status_out) {
    if (!v || (flags & ~ZKLC_G16_COMPRESSED)) return ZKLC_ERR_INVALID_ARG;
    if (!n) return ZKLC_OK;
    if (!proofs || !status_out || (v->key.n_public && !public_inputs)) return ZKLC_ERR_INVALID_ARG;
    const uint32_t compressed = flags & ZKLC_G16_COMPRESSED;
    const uint64_t pbytes = compressed ? 128 : 256;
    uint64_t total, in_words;
    if (!g16_mul_ok(n, pbytes, &total) || !g16_mul_ok(n, (uint64_t)v->key.n_public * 4, &in_words) || in_words > UINT64_MAX / 8)
        return ZKLC_ERR_INVALID_ARG;
    p2v_parallel_for(n, nthreads, [&](uint64_t i) {
        status_out[i] = g16_verify_one_host(v, proofs + i * pbytes, public_inputs + i * (uint64_t)v->key.n_public * 4, compressed);
    });
    return ZKLC_OK;
}
