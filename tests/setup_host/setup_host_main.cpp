// Stand-alone caller of csrc/groth16_setup_host.cpp (its own main; linked with csrc/r1cs_eval_host.cpp and nothing else, no GPU, no
// Python): built by tests/test_setup_host_sanitized.py with -fsanitize=address,undefined and run as a child process.  It makes every
// malformed call of include/zklc.h -- with arrays exactly as long as they claim, so that a read or write behind them is the
// sanitizer's to report -- then runs the cases of the file named on the command line and compares with the words recorded there.
// Exit 0: all as expected.
//
// File (little-endian u64): n_cases; per case: n_constraints, n_wires, nnz, n_coeff, n_public, n, row_ptr [3 n_constraints + 1],
// term_wire [nnz], term_coeff [nnz], coeffs [n_coeff x 4], toxic [5 x 4], a_t, b_t, k [n_wires x 4 each], z [(n - 1) x 4].
#include "../../zk-light-client-implementation_amd/csrc/groth16_setup.cuh"
#include "../../include/zklc.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond, what)                                        \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "FAILED: %s (%s)\n", what, #cond);    \
            failures++;                                           \
        }                                                         \
    } while (0)

// 16-byte aligned arrays of exactly n u64 (operator new aligns to 16 on this ABI; the sanitizer guards both ends)
struct buf {
    uint64_t *p;
    size_t n;
    explicit buf(size_t n_, uint64_t fill = 0) : p(new uint64_t[n_ ? n_ : 1]), n(n_) {
        for (size_t i = 0; i < n; i++) p[i] = fill;
    }
    ~buf() { delete[] p; }
    bool all(uint64_t v) const {
        for (size_t i = 0; i < n; i++)
            if (p[i] != v) return false;
        return true;
    }
};

static const uint64_t R_WORDS[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};

// x * x = y over wires (1, x, y): one constraint, three wires
static zklc_r1cs *tiny_system() {
    const uint64_t row_ptr[4] = {0, 1, 2, 3};
    const uint32_t wire[3] = {1, 1, 2}, coeff[3] = {0, 0, 0};
    const uint32_t one[8] = R1CS_ONE_WORDS;
    zklc_r1cs *s = nullptr;
    EXPECT(r1cs_build_host(1, 3, row_ptr, wire, coeff, 3, (const uint64_t *)one, 1, &s) == ZKLC_OK && s, "the tiny system");
    return s;
}

static void malformed() {
    zklc_r1cs *s = tiny_system();
    if (!s) return;
    buf toxic(20), a(12, 9), b(12, 9), k(12, 9), z(4, 9), out5(5, 9);
    for (int i = 0; i < 5; i++) toxic.p[4 * i] = 3 + i;
    auto run = [&](const zklc_r1cs *sys, const uint64_t *t, uint32_t npub, uint64_t n, uint64_t *pa, uint64_t *pb, uint64_t *pk, uint64_t *pz) {
        return zklc_groth16_setup_scalars_host(sys, t, npub, n, 1, pa, pb, pk, pz);
    };
    EXPECT(run(nullptr, toxic.p, 1, 2, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "no system");
    EXPECT(run(s, nullptr, 1, 2, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "no toxic waste");
    EXPECT(run(s, toxic.p, 1, 2, nullptr, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "no a_t");
    EXPECT(run(s, toxic.p, 1, 2, a.p, nullptr, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "no b_t");
    EXPECT(run(s, toxic.p, 1, 2, a.p, b.p, nullptr, z.p) == ZKLC_ERR_INVALID_ARG, "no k");
    EXPECT(run(s, toxic.p, 1, 2, a.p, b.p, k.p, nullptr) == ZKLC_ERR_INVALID_ARG, "no z");
    EXPECT(run(s, toxic.p, 1, 2, a.p + 1, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "misaligned a_t");
    EXPECT(run(s, toxic.p, 1, 2, a.p, b.p + 1, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "misaligned b_t");
    EXPECT(run(s, toxic.p, 1, 2, a.p, b.p, k.p + 1, z.p) == ZKLC_ERR_INVALID_ARG, "misaligned k");
    EXPECT(run(s, toxic.p, 1, 2, a.p, b.p, k.p, z.p + 1) == ZKLC_ERR_INVALID_ARG, "misaligned z");
    for (uint64_t n : {0ull, 1ull, 3ull, 6ull, 1ull << 29, 1ull << 63, ~0ull})
        EXPECT(run(s, toxic.p, 1, n, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "a domain that is no power of two in [2, 2^28]");
    EXPECT(run(s, toxic.p, 3, 2, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "n_public + 1 > n_wires");
    EXPECT(run(s, toxic.p, ~0u, 2, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "n_public = 2^32 - 1");
    for (int which = 3; which < 5; which++) {
        buf t(20);
        memcpy(t.p, toxic.p, 160);
        for (int i = 0; i < 4; i++) t.p[4 * which + i] = 0;
        EXPECT(run(s, t.p, 1, 2, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "gamma / delta = 0");
        memcpy(t.p + 4 * which, R_WORDS, 32);
        EXPECT(run(s, t.p, 1, 2, a.p, b.p, k.p, z.p) == ZKLC_ERR_INVALID_ARG, "gamma / delta = r");
    }
    EXPECT(a.all(9) && b.all(9) && k.all(9) && z.all(9), "a refused call writes nothing");
    EXPECT(zklc_groth16_setup_plan(nullptr, out5.p) == ZKLC_ERR_INVALID_ARG && zklc_groth16_setup_plan(s, nullptr) == ZKLC_ERR_INVALID_ARG,
           "a plan of nothing");
    EXPECT(out5.all(9), "a refused plan writes nothing");
    EXPECT(zklc_groth16_setup_plan(s, out5.p) == ZKLC_OK && out5.p[0] == 9 && out5.p[1] + out5.p[2] + out5.p[3] + out5.p[4] == 0,
           "nine columns of at most one term");
    // domain 2 with one constraint: z has one element; and the same system on a domain of 8 (z: seven)
    EXPECT(run(s, toxic.p, 1, 2, a.p, b.p, k.p, z.p) == ZKLC_OK && z.p[0] != 9, "the smallest domain");
    {   // toxic needs 8-byte alignment only: the same words 8 bytes further give the same scalars, and nothing is read past them
        buf shifted(21), a2(12, 9), b2(12, 9), k2(12, 9), z2(4, 9);
        memcpy(shifted.p + 1, toxic.p, 160);
        EXPECT(((uintptr_t)(shifted.p + 1) & 15) == 8, "a toxic pointer at 8 mod 16");
        EXPECT(run(s, shifted.p + 1, 1, 2, a2.p, b2.p, k2.p, z2.p) == ZKLC_OK, "toxic at 8 mod 16 is a good call");
        EXPECT(!memcmp(a2.p, a.p, 96) && !memcmp(b2.p, b.p, 96) && !memcmp(k2.p, k.p, 96) && !memcmp(z2.p, z.p, 32), "the same scalars");
    }
    buf z8(28, 9);
    EXPECT(run(s, toxic.p, 1, 8, a.p, b.p, k.p, z8.p) == ZKLC_OK && z8.p[27] != 9, "a domain of 8");
    r1cs_free_host(s);
}

static bool read_u64(FILE *f, uint64_t *dst, size_t n) { return fread(dst, 8, n, f) == n; }

static void cases(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        failures++;
        return;
    }
    uint64_t n_cases = 0;
    if (!read_u64(f, &n_cases, 1)) failures++;
    for (uint64_t c = 0; c < n_cases && !failures; c++) {
        uint64_t h[6];
        if (!read_u64(f, h, 6)) {
            failures++;
            break;
        }
        const uint64_t nc = h[0], nw = h[1], nnz = h[2], n_coeff = h[3], n_public = h[4], n = h[5];
        buf row_ptr(3 * nc + 1), wire64(nnz), coeff64(nnz), coeffs(4 * n_coeff), toxic(20);
        buf want_a(4 * nw), want_b(4 * nw), want_k(4 * nw), want_z(4 * (n - 1));
        if (!read_u64(f, row_ptr.p, 3 * nc + 1) || !read_u64(f, wire64.p, nnz) || !read_u64(f, coeff64.p, nnz) ||
            !read_u64(f, coeffs.p, 4 * n_coeff) || !read_u64(f, toxic.p, 20) || !read_u64(f, want_a.p, 4 * nw) ||
            !read_u64(f, want_b.p, 4 * nw) || !read_u64(f, want_k.p, 4 * nw) || !read_u64(f, want_z.p, 4 * (n - 1))) {
            failures++;
            break;
        }
        std::vector<uint32_t> wire(nnz), coeff(nnz);
        for (uint64_t t = 0; t < nnz; t++) {
            wire[t] = (uint32_t)wire64.p[t];
            coeff[t] = (uint32_t)coeff64.p[t];
        }
        zklc_r1cs *s = nullptr;
        EXPECT(r1cs_build_host(nc, nw, row_ptr.p, wire.data(), coeff.data(), nnz, coeffs.p, (uint32_t)n_coeff, &s) == ZKLC_OK && s, "system");
        if (!s) break;
        for (uint32_t nthreads : {1u, 3u}) {
            buf a(4 * nw, ~0ull), b(4 * nw, ~0ull), k(4 * nw, ~0ull), z(4 * (n - 1), ~0ull);
            EXPECT(zklc_groth16_setup_scalars_host(s, toxic.p, (uint32_t)n_public, n, nthreads, a.p, b.p, k.p, z.p) == ZKLC_OK, "scalar stage");
            EXPECT(!memcmp(a.p, want_a.p, 32 * nw), "a_t");
            EXPECT(!memcmp(b.p, want_b.p, 32 * nw), "b_t");
            EXPECT(!memcmp(k.p, want_k.p, 32 * nw), "k");
            EXPECT(!memcmp(z.p, want_z.p, 32 * (n - 1)), "z");
        }
        if (failures)
            fprintf(stderr, "case %llu: %llu constraints, %llu wires, domain %llu\n", (unsigned long long)c, (unsigned long long)nc,
                    (unsigned long long)nw, (unsigned long long)n);
        r1cs_free_host(s);
    }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    malformed();
    cases(argv[1]);
    if (failures) return 1;
    printf("setup host: ok\n");
    return 0;
}
