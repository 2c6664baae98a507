// plonky2 verifier, host part (see plonky2_verifier_host.h).  Replaces `CircuitData::verify` / `VerifierCircuitData::verify` of the
// un-vendored plonky2 fork at the reference's call sites (near_bft_finality/src/prove_block_data/primitives.rs:110,160,
// header_bphash.rs:94; the tests of prove_crypto/{ed25519,recursion,sha256}.rs).  The checks and their order restate
// oracle/plonky2_verifier.py (gnark-plonky2-verifier/verifier/verifier.go, fri/fri.go, plonk/plonk.go); the gate evaluators restate
// oracle/plonky2_gates.py (gnark-plonky2-verifier/plonk/gates/*.go, crypto/plonky2_u32/src/gates/*.rs), written once over a field
// adapter and used here in the quadratic extension at zeta.
#include "plonky2_verifier_host.h"
#include <string.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <thread>
#include "plonky2_host.h"

// ---------------------------------------------------------------------------------------------------------- field adapter
struct p2v_ext {
    typedef gl2 T;
    static T zero() { return gl2_make(0, 0); }
    static T one() { return gl2_make(1, 0); }
    static T add(T a, T b) { return gl2_add(a, b); }
    static T sub(T a, T b) { return gl2_sub(a, b); }
    static T mul(T a, T b) { return gl2_mul(a, b); }
    static T cst(u64 c) { return gl2_make(gl_canonical(c), 0); }
};

// the degree-2 extension algebra over K (pairs of K, X^2 = 7): quadratic_extension_algebra.go
template <class K>
struct p2v_alg {
    typename K::T a, b;
};
template <class K>
static p2v_alg<K> alg_at(const typename K::T *w, u32 i) { return {w[i], w[i + 1]}; }
template <class K>
static p2v_alg<K> alg_add(p2v_alg<K> x, p2v_alg<K> y) { return {K::add(x.a, y.a), K::add(x.b, y.b)}; }
template <class K>
static p2v_alg<K> alg_sub(p2v_alg<K> x, p2v_alg<K> y) { return {K::sub(x.a, y.a), K::sub(x.b, y.b)}; }
template <class K>
static p2v_alg<K> alg_mul(p2v_alg<K> x, p2v_alg<K> y) {
    return {K::add(K::mul(x.a, y.a), K::mul(K::cst(7), K::mul(x.b, y.b))), K::add(K::mul(x.a, y.b), K::mul(x.b, y.a))};
}
template <class K>
static p2v_alg<K> alg_scalar(typename K::T s, p2v_alg<K> x) { return {K::mul(s, x.a), K::mul(s, x.b)}; }

template <class K>
static typename K::T reduce_with_powers(const typename K::T *terms, u32 n, typename K::T base, u32 stride = 1) {
    typename K::T acc = K::zero();
    for (u32 i = n; i-- > 0;) acc = K::add(K::mul(acc, base), terms[(size_t)i * stride]);
    return acc;
}
template <class K>
static typename K::T range_product(typename K::T x, u32 base) {
    typename K::T acc = K::one();
    for (u32 k = 0; k < base; k++) acc = K::mul(acc, K::sub(x, K::cst(k)));
    return acc;
}

// accumulates constraint i of the current gate, multiplied by the gate's filter, into acc[i]
template <class K>
struct p2v_emit {
    typename K::T *acc;
    typename K::T filter;
    u32 k, cap;
    bool overflow;
    void operator()(typename K::T v) {
        if (k >= cap) {
            overflow = true;
            return;
        }
        acc[k] = K::add(acc[k], K::mul(v, filter));
        k++;
    }
    void operator()(p2v_alg<K> v) {
        (*this)(v.a);
        (*this)(v.b);
    }
};

// One gate's constraints (eval_unfiltered) at one point.  c: the gate constants (selectors excluded), w: the wires.
// Returns false for an unknown gate type.
template <class K>
static bool p2v_gate_eval(const zklc_plonky2_gate &g, const u64 *extra, const typename K::T *c, const typename K::T *w,
                          const u64 *pih, p2v_emit<K> &out) {
    typedef typename K::T T;
    typedef p2v_alg<K> A;
    const u32 *p = g.p;
    switch (g.type) {
    case ZKLC_GATE_NOOP:
        return true;
    case ZKLC_GATE_CONSTANT:
        for (u32 i = 0; i < p[0]; i++) out(K::sub(c[i], w[i]));
        return true;
    case ZKLC_GATE_PUBLIC_INPUT:
        for (u32 i = 0; i < 4; i++) out(K::sub(w[i], K::cst(pih[i])));
        return true;
    case ZKLC_GATE_ARITHMETIC:
        for (u32 i = 0; i < p[0]; i++) {
            const T *q = w + 4 * i;
            out(K::sub(q[3], K::add(K::mul(K::mul(q[0], q[1]), c[0]), K::mul(q[2], c[1]))));
        }
        return true;
    case ZKLC_GATE_ARITHMETIC_EXT:
        for (u32 i = 0; i < p[0]; i++) {
            A m0 = alg_at<K>(w, 8 * i), m1 = alg_at<K>(w, 8 * i + 2), a = alg_at<K>(w, 8 * i + 4), o = alg_at<K>(w, 8 * i + 6);
            out(alg_sub<K>(o, alg_add<K>(alg_scalar<K>(c[1], a), alg_scalar<K>(c[0], alg_mul<K>(m0, m1)))));
        }
        return true;
    case ZKLC_GATE_MUL_EXT:
        for (u32 i = 0; i < p[0]; i++) {
            A m0 = alg_at<K>(w, 6 * i), m1 = alg_at<K>(w, 6 * i + 2), o = alg_at<K>(w, 6 * i + 4);
            out(alg_sub<K>(o, alg_scalar<K>(c[0], alg_mul<K>(m0, m1))));
        }
        return true;
    case ZKLC_GATE_BASE_SUM: {
        out(K::sub(reduce_with_powers<K>(w + 1, p[0], K::cst(p[1])), w[0]));
        for (u32 i = 0; i < p[0]; i++) out(range_product<K>(w[1 + i], p[1]));
        return true;
    }
    case ZKLC_GATE_POSEIDON: {
        static const u64 CIRC[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
        T swap = w[24];
        out(K::mul(swap, K::sub(swap, K::one())));
        for (u32 i = 0; i < 4; i++) out(K::sub(K::mul(swap, K::sub(w[i + 4], w[i])), w[25 + i]));
        T st[12], t[12];
        for (u32 i = 0; i < 4; i++) {
            st[i] = K::add(w[i], w[25 + i]);
            st[i + 4] = K::sub(w[i + 4], w[25 + i]);
        }
        for (u32 i = 8; i < 12; i++) st[i] = w[i];
        auto sbox = [](T x) {
            T x2 = K::mul(x, x), x4 = K::mul(x2, x2);
            return K::mul(x4, K::mul(x, x2));
        };
        auto mds = [&](T *v) {
            T r[12];
            for (u32 row = 0; row < 12; row++) {
                T acc = K::zero();
                for (u32 i = 0; i < 12; i++) acc = K::add(acc, K::mul(v[(i + row) % 12], K::cst(CIRC[i])));
                r[row] = row == 0 ? K::add(acc, K::mul(v[0], K::cst(8))) : acc;
            }
            for (u32 i = 0; i < 12; i++) v[i] = r[i];
        };
        u32 rnd = 0;
        for (u32 r = 0; r < 4; r++, rnd++) {
            for (u32 i = 0; i < 12; i++) st[i] = K::add(st[i], K::cst(PGL_RC[12 * rnd + i]));
            if (r)
                for (u32 i = 0; i < 12; i++) {
                    T sin = w[29 + 12 * (r - 1) + i];
                    out(K::sub(st[i], sin));
                    st[i] = sin;
                }
            for (u32 i = 0; i < 12; i++) st[i] = sbox(st[i]);
            mds(st);
        }
        for (u32 i = 0; i < 12; i++) st[i] = K::add(st[i], K::cst(PGL_FP_FIRST[i]));
        t[0] = st[0];
        for (u32 d = 1; d < 12; d++) t[d] = K::zero();
        for (u32 r = 1; r < 12; r++)
            for (u32 d = 1; d < 12; d++) t[d] = K::add(t[d], K::mul(st[r], K::cst(PGL_FP_INIT[(r - 1) * 11 + d - 1])));
        for (u32 i = 0; i < 12; i++) st[i] = t[i];
        for (u32 r = 0; r < 22; r++) {
            T sin = w[65 + r];
            out(K::sub(st[0], sin));
            T s0 = K::add(sbox(sin), K::cst(PGL_FP_RC[r]));   // PGL_FP_RC[21] = 0
            T d = K::mul(s0, K::cst(25));
            for (u32 i = 1; i < 12; i++) d = K::add(d, K::mul(st[i], K::cst(PGL_FP_WHATS[r * 11 + i - 1])));
            for (u32 i = 1; i < 12; i++) st[i] = K::add(K::mul(s0, K::cst(PGL_FP_VS[r * 11 + i - 1])), st[i]);
            st[0] = d;
        }
        rnd += 22;
        for (u32 r = 0; r < 4; r++, rnd++) {
            for (u32 i = 0; i < 12; i++) {
                st[i] = K::add(st[i], K::cst(PGL_RC[12 * rnd + i]));
                T sin = w[87 + 12 * r + i];
                out(K::sub(st[i], sin));
                st[i] = sbox(sin);
            }
            mds(st);
        }
        for (u32 i = 0; i < 12; i++) out(K::sub(st[i], w[12 + i]));
        return true;
    }
    case ZKLC_GATE_POSEIDON_MDS: {
        static const u64 CIRC[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
        for (u32 r = 0; r < 12; r++) {
            A acc = {K::zero(), K::zero()};
            for (u32 i = 0; i < 12; i++) acc = alg_add<K>(acc, alg_scalar<K>(K::cst(CIRC[i]), alg_at<K>(w, 2 * ((i + r) % 12))));
            if (r == 0) acc = alg_add<K>(acc, alg_scalar<K>(K::cst(8), alg_at<K>(w, 0)));
            out(alg_sub<K>(alg_at<K>(w, 2 * (12 + r)), acc));
        }
        return true;
    }
    case ZKLC_GATE_RANDOM_ACCESS: {
        const u32 bits = p[0], copies = p[1], nextra = p[2], vs = 1u << bits, routed = (2 + vs) * copies + nextra;
        std::vector<T> items(vs);
        for (u32 cp = 0; cp < copies; cp++) {
            const u32 base = (2 + vs) * cp;
            const T *b = w + routed + cp * bits;
            for (u32 i = 0; i < bits; i++) out(K::sub(K::mul(b[i], b[i]), b[i]));
            out(K::sub(reduce_with_powers<K>(b, bits, K::cst(2)), w[base]));
            for (u32 i = 0; i < vs; i++) items[i] = w[base + 2 + i];
            u32 len = vs;
            for (u32 k = 0; k < bits; k++) {
                for (u32 i = 0; i < len; i += 2) items[i / 2] = K::add(items[i], K::mul(b[k], K::sub(items[i + 1], items[i])));
                len /= 2;
            }
            out(K::sub(items[0], w[base + 1]));
        }
        for (u32 i = 0; i < nextra; i++) out(K::sub(c[i], w[(2 + vs) * copies + i]));
        return true;
    }
    case ZKLC_GATE_REDUCING:
    case ZKLC_GATE_REDUCING_EXT: {
        const u32 n = p[0];
        const bool ext = g.type == ZKLC_GATE_REDUCING_EXT;
        const u32 start_accs = ext ? 6 + 2 * n : 6 + n;
        A alpha = alg_at<K>(w, 2), acc = alg_at<K>(w, 4);
        for (u32 i = 0; i < n; i++) {
            A nxt = i == n - 1 ? alg_at<K>(w, 0) : alg_at<K>(w, start_accs + 2 * i);
            A coeff = ext ? alg_at<K>(w, 6 + 2 * i) : A{w[6 + i], K::zero()};
            out(alg_sub<K>(alg_add<K>(alg_mul<K>(acc, alpha), coeff), nxt));
            acc = nxt;
        }
        return true;
    }
    case ZKLC_GATE_EXPONENTIATION: {
        const u32 n = p[0];
        const T base = w[0], *bits = w + 1, outp = w[1 + n], *inter = w + 2 + n;
        for (u32 i = 0; i < n; i++) {
            T prev = i == 0 ? K::one() : K::mul(inter[i - 1], inter[i - 1]);
            T b = bits[n - 1 - i];
            T mul_by = K::sub(K::mul(b, base), K::sub(b, K::one()));
            out(K::sub(K::mul(prev, mul_by), inter[i]));
        }
        out(K::sub(outp, inter[n - 1]));
        return true;
    }
    case ZKLC_GATE_COSET_INTERPOLATION: {
        const u32 np = 1u << p[0], d = p[1], n_inter = (np - 2) / (d - 1);
        const u64 *weights = extra + g.extra_off, *dom = weights + np;
        const u32 start_pt = 1 + 2 * np, start_val = start_pt + 2, start_inter = start_val + 2;
        const T shift = w[0];
        const A point = alg_at<K>(w, start_pt), shifted = alg_at<K>(w, start_inter + 4 * n_inter);
        out(alg_add<K>(alg_scalar<K>(K::sub(K::zero(), shift), shifted), point));
        auto partial = [&](u32 s, u32 e, A ev, A prod, A *ev_out, A *prod_out) {
            for (u32 i = s; i < e; i++) {
                A term = alg_sub<K>(shifted, A{K::cst(dom[i]), K::zero()});
                A wv = alg_scalar<K>(K::cst(weights[i]), alg_at<K>(w, 1 + 2 * i));
                ev = alg_add<K>(alg_mul<K>(ev, term), alg_mul<K>(wv, prod));
                prod = alg_mul<K>(prod, term);
            }
            *ev_out = ev;
            *prod_out = prod;
        };
        A ev, prod;
        partial(0, d < np ? d : np, A{K::zero(), K::zero()}, A{K::one(), K::zero()}, &ev, &prod);
        for (u32 i = 0; i < n_inter; i++) {
            A iev = alg_at<K>(w, start_inter + 2 * i), ipr = alg_at<K>(w, start_inter + 2 * (n_inter + i));
            out(alg_sub<K>(iev, ev));
            out(alg_sub<K>(ipr, prod));
            u32 s = 1 + (d - 1) * (i + 1), e = s + d - 1 < np ? s + d - 1 : np;
            partial(s, e, iev, ipr, &ev, &prod);
        }
        out(alg_sub<K>(alg_at<K>(w, start_val), ev));
        return true;
    }
    case ZKLC_GATE_U32_ARITHMETIC: {
        const u32 n = p[0];
        for (u32 i = 0; i < n; i++) {
            const T *q = w + 6 * i;
            T computed = K::add(K::mul(q[0], q[1]), q[2]);
            T hi_not_max = K::sub(K::mul(q[5], K::sub(K::cst(0xFFFFFFFFull), q[4])), K::one());
            out(K::mul(hi_not_max, q[3]));
            out(K::sub(K::add(K::mul(q[4], K::cst(1ull << 32)), q[3]), computed));
            const T *limbs = w + 6 * n + 32 * i;
            for (u32 j = 32; j-- > 0;) out(range_product<K>(limbs[j], 4));
            out(K::sub(reduce_with_powers<K>(limbs, 16, K::cst(4)), q[3]));
            out(K::sub(reduce_with_powers<K>(limbs + 16, 16, K::cst(4)), q[4]));
        }
        return true;
    }
    case ZKLC_GATE_U32_ADD_MANY: {
        const u32 na = p[0], n = p[1], per = na + 3;
        for (u32 i = 0; i < n; i++) {
            T comp = w[per * i + na];
            for (u32 j = 0; j < na; j++) comp = K::add(comp, w[per * i + j]);
            T res = w[per * i + na + 1], carry = w[per * i + na + 2];
            out(K::sub(K::add(K::mul(carry, K::cst(1ull << 32)), res), comp));
            T cr = K::zero(), cc = K::zero();
            for (u32 j = 18; j-- > 0;) {
                T l = w[per * n + 18 * i + j];
                out(range_product<K>(l, 4));
                if (j < 16) cr = K::add(K::mul(K::cst(4), cr), l);
                else cc = K::add(K::mul(K::cst(4), cc), l);
            }
            out(K::sub(cr, res));
            out(K::sub(cc, carry));
        }
        return true;
    }
    case ZKLC_GATE_U32_SUBTRACTION: {
        const u32 n = p[0];
        for (u32 i = 0; i < n; i++) {
            const T *q = w + 5 * i;
            T initial = K::sub(K::sub(q[0], q[1]), q[2]);
            out(K::sub(q[3], K::add(initial, K::mul(K::cst(1ull << 32), q[4]))));
            T comb = K::zero();
            for (u32 j = 16; j-- > 0;) {
                T l = w[5 * n + 16 * i + j];
                out(range_product<K>(l, 4));
                comb = K::add(K::mul(K::cst(4), comb), l);
            }
            out(K::sub(comb, q[3]));
            out(K::mul(q[4], K::sub(K::one(), q[4])));
        }
        return true;
    }
    case ZKLC_GATE_U32_RANGE_CHECK: {
        const u32 n = p[0];
        for (u32 i = 0; i < n; i++) {
            const T *aux = w + n + 16 * i;
            out(K::sub(reduce_with_powers<K>(aux, 16, K::cst(4)), w[i]));
            for (u32 j = 0; j < 16; j++) out(range_product<K>(aux[j], 4));
        }
        return true;
    }
    case ZKLC_GATE_COMPARISON: {
        const u32 nc = p[1], cb = (p[0] + nc - 1) / nc, size = 1u << cb;
        const T *first = w + 4, *second = w + 4 + nc;
        out(K::sub(reduce_with_powers<K>(first, nc, K::cst(size)), w[0]));
        out(K::sub(reduce_with_powers<K>(second, nc, K::cst(size)), w[1]));
        T msd = K::zero();
        for (u32 i = 0; i < nc; i++) {
            out(range_product<K>(first[i], size));
            out(range_product<K>(second[i], size));
            T diff = K::sub(second[i], first[i]);
            T dummy = w[4 + 2 * nc + i], eq = w[4 + 3 * nc + i];
            out(K::sub(K::mul(diff, dummy), K::sub(K::one(), eq)));
            out(K::mul(eq, diff));
            T inter = w[4 + 4 * nc + i];
            out(K::sub(inter, K::mul(eq, msd)));
            msd = K::add(inter, K::mul(K::sub(K::one(), eq), diff));
        }
        out(K::sub(w[3], msd));
        const T *bits = w + 4 + 5 * nc;
        for (u32 i = 0; i <= cb; i++) out(K::mul(bits[i], K::sub(K::one(), bits[i])));
        out(K::sub(K::add(K::cst(size), w[3]), reduce_with_powers<K>(bits, cb + 1, K::cst(2))));
        out(K::sub(w[2], bits[cb]));
        return true;
    }
    case ZKLC_GATE_U32_INTERLEAVE: {
        const u32 n = p[0];
        for (u32 i = 0; i < n; i++) {
            const T *bits = w + 2 * n + 32 * i;   // big-endian: bits[31] is the least significant
            T v2 = K::zero(), v4 = K::zero();
            for (u32 j = 0; j < 32; j++) {
                v2 = K::add(K::mul(v2, K::cst(2)), bits[j]);
                v4 = K::add(K::mul(v4, K::cst(4)), bits[j]);
            }
            out(K::sub(v2, w[2 * i]));
            out(K::sub(v4, w[2 * i + 1]));
            for (u32 j = 0; j < 32; j++) out(range_product<K>(bits[j], 2));
        }
        return true;
    }
    case ZKLC_GATE_UNINTERLEAVE_TO_U32:
    case ZKLC_GATE_UNINTERLEAVE_TO_B32: {
        const u32 n = p[0];
        const bool b32 = g.type == ZKLC_GATE_UNINTERLEAVE_TO_B32;
        for (u32 i = 0; i < n; i++) {
            const T *bits = w + 3 * n + 64 * i;
            T v = K::zero();
            for (u32 j = 0; j < 64; j++) v = K::add(K::mul(v, K::cst(2)), bits[j]);
            out(K::sub(v, w[3 * i]));
            T ev = K::zero(), od = K::zero();
            for (u32 j = 0; j < 32; j++) {
                T coeff = K::cst(b32 ? 1ull << (2 * (31 - j)) : 1ull << (31 - j));
                ev = K::add(ev, K::mul(coeff, bits[2 * j]));
                od = K::add(od, K::mul(coeff, bits[2 * j + 1]));
            }
            out(K::sub(ev, w[3 * i + 1]));
            out(K::sub(od, w[3 * i + 2]));
            for (u32 j = 0; j < 64; j++) out(range_product<K>(bits[j], 2));
        }
        return true;
    }
    default:
        return false;
    }
}

// ---------------------------------------------------------------------------------------------------------- layout
static const u64 BN_R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

static bool p2v_make_layout(const zklc_plonky2_params &P, p2v_layout &L) {
    memset(&L, 0, sizeof(L));
    if (P.num_arities > P2V_MAX_ARITIES || P.hasher > 1 || P.num_challenges == 0) return false;
    u32 sum = 0;
    for (u32 i = 0; i < P.num_arities; i++) {
        if (P.arity_bits[i] == 0 || P.arity_bits[i] > 16) return false;
        sum += P.arity_bits[i];
    }
    if (sum > P.degree_bits) return false;
    L.hasher = P.hasher;
    L.nch = P.num_challenges;
    L.num_arities = P.num_arities;
    L.num_trees = 4 + P.num_arities;
    L.rounds = P.num_query_rounds;
    L.lde_bits = P.degree_bits + P.rate_bits;
    if (L.lde_bits > 32) return false;
    L.final_len = 1u << (P.degree_bits - sum);
    L.cap_h0 = P.cap_height < L.lde_bits ? P.cap_height : L.lde_bits;
    const u32 nch = P.num_challenges;
    u32 widths[4] = {P.num_constants + P.num_routed_wires, P.num_wires, nch * (1 + P.num_partial_products),
                     nch * P.quotient_degree_factor};
    u32 nop[7] = {P.num_constants, P.num_routed_wires, P.num_wires, nch, nch, nch * P.num_partial_products,
                  nch * P.quotient_degree_factor};
    u64 o = 0;
    for (int k = 0; k < 3; k++) {
        L.cap_off[k] = o;
        o += (u64)32 << L.cap_h0;
    }
    L.openings_off = o;
    for (int k = 0; k < 7; k++) {
        L.n_openings[k] = nop[k];
        o += 16 * (u64)nop[k];
    }
    u32 bits = L.lde_bits;
    for (u32 i = 0; i < P.num_arities; i++) {
        L.arity_bits[i] = P.arity_bits[i];
        bits -= P.arity_bits[i];
        L.commit_cap_h[i] = P.cap_height < bits ? P.cap_height : bits;
        L.commit_cap_off[i] = o;
        o += (u64)32 << L.commit_cap_h[i];
    }
    L.rounds_off = o;
    u64 r = 0;
    for (int k = 0; k < 4; k++) {
        L.tree_off[k] = r;
        L.leaf_words[k] = widths[k];
        L.depth[k] = L.lde_bits - L.cap_h0;
        r += 8 * (u64)widths[k] + 1 + 32 * (u64)L.depth[k];
    }
    bits = L.lde_bits;
    for (u32 i = 0; i < P.num_arities; i++) {
        bits -= P.arity_bits[i];
        L.tree_off[4 + i] = r;
        L.leaf_words[4 + i] = 2u << P.arity_bits[i];
        L.depth[4 + i] = bits - L.commit_cap_h[i];
        r += 8 * (u64)L.leaf_words[4 + i] + 1 + 32 * (u64)L.depth[4 + i];
    }
    L.round_bytes = r;
    o += r * P.num_query_rounds;
    L.final_off = o;
    o += 16 * (u64)L.final_len;
    L.pow_off = o;
    L.npi_off = o + 8;
    L.pi_off = o + 16;
    L.bytes = L.pi_off + 8 * (u64)P.num_public_inputs;
    return true;
}

extern "C" int32_t zklc_plonky2_verifier_create(zklc_ctx *ctx, const zklc_plonky2_params *params, const zklc_plonky2_gate *gates,
                                                const uint64_t *gate_extra, uint32_t gate_extra_words, const uint64_t *k_is,
                                                const uint8_t *cap, const uint8_t *digest, zklc_plonky2_verifier **out) {
    (void)ctx;   // the device side is set up by the first zklc_plonky2_verify_batch
    if (!params || !gates || !k_is || !cap || !digest || !out || (gate_extra_words && !gate_extra)) return ZKLC_ERR_INVALID_ARG;
    *out = nullptr;
    const zklc_plonky2_params &P = *params;
    if (P.num_gates == 0 || P.num_selectors == 0 || P.num_constants < P.num_selectors || P.num_routed_wires > P.num_wires ||
        P.quotient_degree_factor == 0 || P.proof_of_work_bits > 63)
        return ZKLC_ERR_INVALID_ARG;
    zklc_plonky2_verifier *v = new (std::nothrow) zklc_plonky2_verifier();
    if (!v) return ZKLC_ERR_OOM;
    v->P = P;
    if (!p2v_make_layout(P, v->L)) {
        delete v;
        return ZKLC_ERR_INVALID_ARG;
    }
    v->gates.assign(gates, gates + P.num_gates);
    for (const zklc_plonky2_gate &g : v->gates) {
        bool bad = g.type > ZKLC_GATE_UNINTERLEAVE_TO_B32 || g.selector_index >= P.num_selectors || g.group_start >= g.group_end;
        if (g.type == ZKLC_GATE_COSET_INTERPOLATION)
            bad = bad || g.p[0] < 1 || g.p[0] > 16 || g.p[1] < 2 || (u64)g.extra_off + (2ull << g.p[0]) > gate_extra_words;
        if (g.type == ZKLC_GATE_RANDOM_ACCESS) bad = bad || g.p[0] > 16;
        if (g.type == ZKLC_GATE_COMPARISON) bad = bad || g.p[1] == 0 || (g.p[0] + g.p[1] - 1) / g.p[1] > 16;
        if (g.type == ZKLC_GATE_BASE_SUM) bad = bad || g.p[1] < 2;
        if (bad) {
            delete v;
            return ZKLC_ERR_INVALID_ARG;
        }
    }
    v->extra.assign(gate_extra, gate_extra + gate_extra_words);
    v->k_is.assign(k_is, k_is + P.num_routed_wires);
    v->cap.assign(cap, cap + ((size_t)32 << v->L.cap_h0));
    v->digest.assign(digest, digest + 32);
    *out = v;
    return ZKLC_OK;
}

extern "C" int32_t zklc_plonky2_verifier_create_from_circuit(zklc_ctx *ctx, zklc_plonky2_circuit *c, zklc_plonky2_verifier **out) {
    if (!c || !out) return ZKLC_ERR_INVALID_ARG;
    zklc_plonky2_params P;
    std::vector<zklc_plonky2_gate> gates;
    std::vector<uint64_t> extra, k_is;
    int32_t rc = p2_circuit_verifier_args(c, &P, &gates, &extra, &k_is);
    if (rc) return rc;
    // the circuit's commitment: constants / sigmas cap (2^min(cap_height, lde bits) digests) and circuit digest
    const u32 lde_bits = P.degree_bits + P.rate_bits;
    std::vector<uint8_t> cap((size_t)32 << (P.cap_height < lde_bits ? P.cap_height : lde_bits)), digest(32);
    if ((rc = zklc_plonky2_verifier_data(c, cap.data(), digest.data()))) return rc;
    return zklc_plonky2_verifier_create(ctx, &P, gates.data(), extra.empty() ? nullptr : extra.data(), (uint32_t)extra.size(),
                                        k_is.data(), cap.data(), digest.data(), out);
}

extern "C" uint64_t zklc_plonky2_verifier_proof_bytes(const zklc_plonky2_verifier *v) { return v ? v->L.bytes : 0; }

// ---------------------------------------------------------------------------------------------------------- host stage
static bool p2v_digest_canonical(const uint8_t *h, u32 hasher) {
    if (hasher == 0) {
        for (int i = 0; i < 4; i++)
            if (p2v_ld64(h + 8 * i) >= GL_P) return false;
        return true;
    }
    for (int i = 3; i >= 0; i--) {     // a BN254 Fr value below r
        u64 x = p2v_ld64(h + 8 * i);
        if (x != BN_R[i]) return x < BN_R[i];
    }
    return false;
}

static bool p2v_elems_canonical(const uint8_t *p, u64 n) {
    for (u64 i = 0; i < n; i++)
        if (p2v_ld64(p + 8 * i) >= GL_P) return false;
    return true;
}

static bool p2v_format_ok(const zklc_plonky2_verifier *v, const uint8_t *pr) {
    const p2v_layout &L = v->L;
    const u32 cap_n = 1u << L.cap_h0;
    for (int k = 0; k < 3; k++)
        for (u32 i = 0; i < cap_n; i++)
            if (!p2v_digest_canonical(pr + L.cap_off[k] + 32 * i, L.hasher)) return false;
    u64 nop = 0;
    for (int k = 0; k < 7; k++) nop += L.n_openings[k];
    if (!p2v_elems_canonical(pr + L.openings_off, 2 * nop)) return false;
    for (u32 i = 0; i < L.num_arities; i++)
        for (u32 j = 0; j < (1u << L.commit_cap_h[i]); j++)
            if (!p2v_digest_canonical(pr + L.commit_cap_off[i] + 32 * j, L.hasher)) return false;
    for (u32 r = 0; r < L.rounds; r++) {
        const uint8_t *rb = pr + L.rounds_off + (u64)r * L.round_bytes;
        for (u32 t = 0; t < L.num_trees; t++) {
            const uint8_t *leaf = rb + L.tree_off[t];
            if (!p2v_elems_canonical(leaf, L.leaf_words[t])) return false;
            const uint8_t *cnt = leaf + 8 * (u64)L.leaf_words[t];
            if (*cnt != L.depth[t]) return false;
            for (u32 d = 0; d < L.depth[t]; d++)
                if (!p2v_digest_canonical(cnt + 1 + 32 * (u64)d, L.hasher)) return false;
        }
    }
    if (!p2v_elems_canonical(pr + L.final_off, 2 * (u64)L.final_len) || !p2v_elems_canonical(pr + L.pow_off, 1)) return false;
    if (p2v_ld64(pr + L.npi_off) != v->P.num_public_inputs) return false;
    return p2v_elems_canonical(pr + L.pi_off, v->P.num_public_inputs);
}

static gl2 p2v_reduce_ext(const gl2 *t, u64 n, gl2 alpha) {
    gl2 s = gl2_make(0, 0);
    for (u64 i = n; i-- > 0;) s = gl2_add(gl2_mul(s, alpha), t[i]);
    return s;
}

int32_t p2v_host_stage(const zklc_plonky2_verifier *v, const uint8_t *pr, p2v_proof_tab *tab, uint32_t *x_index) {
    const p2v_layout &L = v->L;
    const zklc_plonky2_params &P = v->P;
    if (!p2v_format_ok(v, pr)) return ZKLC_PROOF_BAD_FORMAT;
    const u32 nch = P.num_challenges, hs = L.hasher;
    // ---- transcript (oracle/plonky2_verifier.py `challenges`; the prover's order, plonky2_prover.hip zklc_plonky2_prove_dev)
    std::vector<u64> pis(P.num_public_inputs);
    for (u32 i = 0; i < P.num_public_inputs; i++) pis[i] = p2v_ld64(pr + L.pi_off + 8 * (u64)i);
    u64 pih[4];
    zklc_host_poseidon_hash_no_pad(pis.data(), pis.size(), pih);
    zklc_challenger ch;
    const u32 cap_n = 1u << L.cap_h0;
    ch.observe_hash(v->digest.data(), hs);
    ch.observe_many(pih, 4);
    for (u32 i = 0; i < cap_n; i++) ch.observe_hash(pr + L.cap_off[0] + 32 * i, hs);
    std::vector<u64> betas(nch), gammas(nch), alphas(nch);
    for (u32 k = 0; k < nch; k++) betas[k] = ch.challenge();
    for (u32 k = 0; k < nch; k++) gammas[k] = ch.challenge();
    for (u32 i = 0; i < cap_n; i++) ch.observe_hash(pr + L.cap_off[1] + 32 * i, hs);
    for (u32 k = 0; k < nch; k++) alphas[k] = ch.challenge();
    for (u32 i = 0; i < cap_n; i++) ch.observe_hash(pr + L.cap_off[2] + 32 * i, hs);
    gl2 zeta;
    zeta.a = ch.challenge();
    zeta.b = ch.challenge();
    // openings in byte order: constants, sigmas, wires, zs, zs_next, partial products, quotient
    std::vector<gl2> op[7];
    u64 o = L.openings_off;
    for (int k = 0; k < 7; k++) {
        op[k].resize(L.n_openings[k]);
        for (u32 i = 0; i < L.n_openings[k]; i++, o += 16) op[k][i] = p2v_ld_ext(pr + o);
    }
    // FRI batches: batch 0 = constants, sigmas, wires, zs, partial products, quotient; batch 1 = zs_next
    std::vector<gl2> batch0;
    for (int k : {0, 1, 2, 3, 5, 6}) batch0.insert(batch0.end(), op[k].begin(), op[k].end());
    for (const gl2 &e : batch0) {
        ch.observe(e.a);
        ch.observe(e.b);
    }
    for (const gl2 &e : op[4]) {
        ch.observe(e.a);
        ch.observe(e.b);
    }
    gl2 fri_alpha;
    fri_alpha.a = ch.challenge();
    fri_alpha.b = ch.challenge();
    for (u32 i = 0; i < L.num_arities; i++) {
        for (u32 j = 0; j < (1u << L.commit_cap_h[i]); j++) ch.observe_hash(pr + L.commit_cap_off[i] + 32 * j, hs);
        tab->betas[i].a = ch.challenge();
        tab->betas[i].b = ch.challenge();
    }
    for (u32 i = 0; i < L.final_len; i++) {
        ch.observe(p2v_ld64(pr + L.final_off + 16 * (u64)i));
        ch.observe(p2v_ld64(pr + L.final_off + 16 * (u64)i + 8));
    }
    ch.observe(p2v_ld64(pr + L.pow_off));
    const u64 pow_response = ch.challenge();
    for (u32 r = 0; r < L.rounds; r++) {
        u64 q = ch.challenge();
        x_index[r] = (u32)(L.lde_bits == 32 ? q : q & ((1ull << L.lde_bits) - 1));
    }
    // ---- proof of work (fri.go:75-80)
    if (P.proof_of_work_bits && (pow_response >> (64 - P.proof_of_work_bits)) != 0) return ZKLC_PROOF_BAD_POW;
    // ---- vanishing identity at zeta (plonk.go:60-250)
    typedef p2v_ext K;
    const u64 n = 1ull << P.degree_bits;
    const gl2 zeta_n = gl2_pow(zeta, n), zh = gl2_sub(zeta_n, K::one());
    const gl2 l0 = gl2_mul(zh, gl2_inv(gl2_sub(gl2_scale(zeta, n % GL_P), K::cst(n))));
    const u32 routed = P.num_routed_wires, npp = P.num_partial_products, qdf = P.quotient_degree_factor;
    const u32 nsel = P.num_selectors;
    const std::vector<gl2> &consts = op[0], &sigmas = op[1], &wires = op[2], &zs = op[3], &zs_next = op[4], &pps = op[5];
    std::vector<gl2> terms;
    terms.reserve(nch * (1 + npp + 1) + P.num_gate_constraints);
    std::vector<gl2> s_ids(routed);
    for (u32 j = 0; j < routed; j++) s_ids[j] = gl2_scale(zeta, v->k_is[j]);
    for (u32 i = 0; i < nch; i++) terms.push_back(gl2_mul(l0, gl2_sub(zs[i], K::one())));
    for (u32 i = 0; i < nch; i++) {
        const u64 b = betas[i], g = gammas[i];
        std::vector<gl2> acc(npp + 2);
        acc[0] = zs[i];
        for (u32 k = 0; k < npp; k++) acc[1 + k] = pps[i * npp + k];
        acc[npp + 1] = zs_next[i];
        for (u32 k = 0; k <= npp; k++) {
            gl2 nu = K::one(), de = K::one();
            for (u32 j = k * qdf; j < (k + 1) * qdf && j < routed; j++) {
                gl2 wg = gl2_add_base(wires[j], g);
                nu = gl2_mul(nu, gl2_add(gl2_scale(s_ids[j], b), wg));
                de = gl2_mul(de, gl2_add(gl2_scale(sigmas[j], b), wg));
            }
            terms.push_back(gl2_sub(gl2_mul(acc[k], nu), gl2_mul(acc[k + 1], de)));
        }
    }
    // gate constraints: filters of the selector groups (evaluate_gates.go:34-105)
    std::vector<gl2> cons(P.num_gate_constraints, K::zero());
    for (u32 row = 0; row < P.num_gates; row++) {
        const zklc_plonky2_gate &g = v->gates[row];
        const gl2 s = consts[g.selector_index];
        gl2 f = K::one();
        for (u32 i = g.group_start; i < g.group_end; i++)
            if (i != row) f = gl2_mul(f, gl2_sub(K::cst(i), s));
        if (nsel > 1) f = gl2_mul(f, gl2_sub(K::cst(0xFFFFFFFFull), s));
        p2v_emit<K> em = {cons.data(), f, 0, P.num_gate_constraints, false};
        if (!p2v_gate_eval<K>(g, v->extra.data(), consts.data() + nsel, wires.data(), pih, em) || em.overflow)
            return ZKLC_PROOF_BAD_VANISHING;
    }
    terms.insert(terms.end(), cons.begin(), cons.end());
    for (u32 i = 0; i < nch; i++) {
        gl2 van = p2v_reduce_ext(terms.data(), terms.size(), gl2_make(alphas[i], 0));
        gl2 t = p2v_reduce_ext(op[6].data() + (size_t)i * qdf, qdf, zeta_n);
        if (!gl2_eq(van, gl2_mul(zh, t))) return ZKLC_PROOF_BAD_VANISHING;
    }
    // ---- what the query phase needs: reduced openings (powers of the FRI alpha) and the two opening points
    tab->fri_alpha = fri_alpha;
    tab->alpha_pow_nch = gl2_pow(fri_alpha, nch);
    tab->zeta = zeta;
    tab->gzeta = gl2_scale(zeta, gl_root_of_unity(P.degree_bits));
    tab->red[0] = p2v_reduce_ext(batch0.data(), batch0.size(), fri_alpha);
    tab->red[1] = p2v_reduce_ext(op[4].data(), op[4].size(), fri_alpha);
    return ZKLC_PROOF_OK;
}

int32_t p2v_query_host(const zklc_plonky2_verifier *v, const uint8_t *pr, const p2v_proof_tab &tab, const uint32_t *x_index) {
    const p2v_layout &L = v->L;
    bool (*merkle)(const p2v_layout &, const uint8_t *, const uint8_t *, u32, u32, u32) =
        L.hasher == 0 ? p2v_merkle_lane<0> : p2v_merkle_lane<1>;
    for (u32 r = 0; r < L.rounds; r++) {
        for (u32 t = 0; t < 4; t++)
            if (!merkle(L, pr, v->cap.data(), r, t, x_index[r])) return ZKLC_PROOF_BAD_MERKLE;
        const u32 fri = p2v_fri_lane(L, pr, tab, r, x_index[r]);
        for (u32 i = 0; i < L.num_arities; i++) {
            if (fri == 1 + i) return ZKLC_PROOF_BAD_FRI;
            if (!merkle(L, pr, v->cap.data(), r, 4 + i, x_index[r])) return ZKLC_PROOF_BAD_MERKLE;
        }
        if (fri) return ZKLC_PROOF_BAD_FRI;
    }
    return ZKLC_PROOF_OK;
}

void p2v_parallel_for(uint64_t n, uint32_t nthreads, const std::function<void(uint64_t)> &fn) {
    if (nthreads == 0) nthreads = 16;
    if (nthreads > 256) nthreads = 256;
    const uint64_t nt = n < nthreads ? n : nthreads;
    if (nt <= 1) {
        for (uint64_t i = 0; i < n; i++) fn(i);
        return;
    }
    std::atomic<uint64_t> next(0);
    auto work = [&]() {
        for (uint64_t i; (i = next.fetch_add(1)) < n;) fn(i);
    };
    std::vector<std::thread> th;
    th.reserve(nt - 1);
    for (uint64_t k = 1; k < nt; k++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

extern "C" int32_t zklc_plonky2_verify_batch_host(zklc_plonky2_verifier *v, const uint8_t *proofs, uint64_t n, uint32_t nthreads,
                                                  int32_t *status_out) {
    if (!v || (n && (!proofs || !status_out))) return ZKLC_ERR_INVALID_ARG;
    const p2v_layout &L = v->L;
    p2v_parallel_for(n, nthreads, [&](uint64_t i) {
        const uint8_t *pr = proofs + i * L.bytes;
        p2v_proof_tab tab;
        std::vector<uint32_t> idx(L.rounds);
        int32_t st = p2v_host_stage(v, pr, &tab, idx.data());
        if (st == ZKLC_PROOF_OK) st = p2v_query_host(v, pr, tab, idx.data());
        status_out[i] = st;
    });
    return ZKLC_OK;
}
