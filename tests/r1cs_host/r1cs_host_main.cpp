// Stand-alone caller of csrc/r1cs_eval_host.cpp (its own main, nothing else linked, no GPU, no Python): built by
// tests/test_r1cs_host.py with -fsanitize=address,undefined and run as a child process.  It feeds the validation every malformed
// input of include/zklc.h -- with arrays exactly as long as they claim, so that a read behind them is the sanitizer's to report --
// then evaluates the system of the file named on the command line against the words recorded there.  Exit 0: all as expected.
//
// File (little-endian u64 unless noted): n_constraints, n_wires, nnz, n_coeff, n, n_broken; row_ptr [3 n_constraints + 1];
// term_wire u32 [nnz]; term_coeff u32 [nnz]; (padding to 8 bytes); coeffs [n_coeff x 4]; then 1 + n_broken cases of: witness
// [n_wires x 4], a, b, c [n x 4 each], summary [2].
#include "../../zk-light-client-implementation_amd/csrc/r1cs_eval.cuh"
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

static const uint64_t R_WORDS[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const uint64_t ONE_MONT[4] = {0xac96341c4ffffffbull, 0x36fc76959f60cd29ull, 0x666ea36f7879462eull, 0x0e0a77c19a07df2full};

// a two-constraint system, well formed: A = [{0: 1}, {1: 1}], B = [{0: 1}, {}], C = [{0: 1}, {}]
struct tiny {
    std::vector<uint64_t> row_ptr = {0, 1, 2, 3, 3, 4, 4};
    std::vector<uint32_t> wire = {0, 1, 0, 0}, coeff = {0, 0, 0, 0};
    std::vector<uint64_t> coeffs = {ONE_MONT[0], ONE_MONT[1], ONE_MONT[2], ONE_MONT[3]};
    uint64_t nc = 2, n_wires = 2;
    int32_t create(zklc_r1cs **out) {
        return r1cs_build_host(nc, n_wires, row_ptr.data(), wire.data(), coeff.data(), wire.size(), coeffs.data(), (uint32_t)(coeffs.size() / 4), out);
    }
};

static void expect_rejected(tiny &t, const char *what) {
    zklc_r1cs *s = (zklc_r1cs *)1;
    const int32_t rc = t.create(&s);
    EXPECT(rc == ZKLC_ERR_INVALID_ARG && s == nullptr, what);
    if (rc == ZKLC_OK) r1cs_free_host(s);
}

static void malformed() {
    zklc_r1cs *s = nullptr;
    {
        tiny t;
        EXPECT(t.create(&s) == ZKLC_OK && s, "the well-formed system is accepted");
        // calls of the evaluation that must be refused
        alignas(16) uint64_t w[8] = {1, 0, 0, 0, 5, 0, 0, 0}, a[12], b[12], c[12], sum[2];
        EXPECT(zklc_r1cs_abc_host(s, w, 1, a, b, c, 0, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "n < n_constraints");
        EXPECT(zklc_r1cs_abc_host(s, w, 2, a, b, c, 2, 1, sum) == ZKLC_ERR_INVALID_ARG, "unknown flag bits");
        EXPECT(zklc_r1cs_abc_host(s, w, 2, a, b, c, ZKLC_R1CS_CHECK, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "check without a summary");
        EXPECT(zklc_r1cs_abc_host(s, w, 2, a, nullptr, c, 0, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "missing output");
        EXPECT(zklc_r1cs_abc_host(s, nullptr, 2, a, b, c, 0, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "missing witness");
        EXPECT(zklc_r1cs_abc_host(s, w + 1, 2, a, b, c, 0, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "misaligned witness");
        EXPECT(zklc_r1cs_abc_host(s, w, 2, a, b + 1, c, 0, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "misaligned output");
        EXPECT(zklc_r1cs_abc_host(nullptr, w, 2, a, b, c, 0, 1, nullptr) == ZKLC_ERR_INVALID_ARG, "missing system");
        // and one that must not: 1 * 1 = 1, 5 * 0 = 0; n = 3 pads one row
        memset(a, 0xff, sizeof a), memset(b, 0xff, sizeof b), memset(c, 0xff, sizeof c);
        EXPECT(zklc_r1cs_abc_host(s, w, 3, a, b, c, ZKLC_R1CS_CHECK, 2, sum) == ZKLC_OK, "the tiny system evaluates");
        EXPECT(sum[0] == 0 && sum[1] == ~0ull, "the tiny system is satisfied");
        EXPECT(!memcmp(a, ONE_MONT, 32) && !memcmp(c, ONE_MONT, 32) && b[4] == 0 && a[8] == 0 && a[11] == 0 && c[11] == 0, "words of the tiny system");
        EXPECT(zklc_r1cs_workspace_bytes(s) == 64, "workspace bytes");
        r1cs_free_host(s);
    }
    {
        // sizes whose products wrap, with four-entry arrays: refused before anything is read
        tiny t;
        t.nc = 1ull << 62;
        expect_rejected(t, "n_constraints = 2^62");
        t.nc = (1ull << 62) + 2;
        expect_rejected(t, "n_constraints = 2^62 + 2");
        t.nc = 0x5555555555555556ull;                       // 3 n + 1 wraps to 3
        expect_rejected(t, "3 n_constraints + 1 wraps");
    }
    {
        tiny t;
        zklc_r1cs *q = (zklc_r1cs *)1;
        EXPECT(r1cs_build_host(2, 2, t.row_ptr.data(), t.wire.data(), t.coeff.data(), 1ull << 62, t.coeffs.data(), 1, &q) == ZKLC_ERR_INVALID_ARG && !q,
               "nnz = 2^62");
        EXPECT(r1cs_build_host(2, 2, t.row_ptr.data(), t.wire.data(), t.coeff.data(), 4, t.coeffs.data(), (1u << 30) + 1, &q) == ZKLC_ERR_INVALID_ARG,
               "n_coeff above 2^30");
        EXPECT(r1cs_build_host(2, 2, nullptr, t.wire.data(), t.coeff.data(), 4, t.coeffs.data(), 1, &q) == ZKLC_ERR_INVALID_ARG, "missing row_ptr");
        EXPECT(r1cs_build_host(2, 2, t.row_ptr.data(), nullptr, t.coeff.data(), 4, t.coeffs.data(), 1, &q) == ZKLC_ERR_INVALID_ARG, "missing wires");
        EXPECT(r1cs_build_host(2, 2, t.row_ptr.data(), t.wire.data(), t.coeff.data(), 4, nullptr, 1, &q) == ZKLC_ERR_INVALID_ARG, "missing coefficients");
        EXPECT(r1cs_build_host(2, 2, t.row_ptr.data(), t.wire.data(), t.coeff.data(), 4, t.coeffs.data(), 1, nullptr) == ZKLC_ERR_INVALID_ARG, "missing out");
    }
    { tiny t; t.n_wires = 0; expect_rejected(t, "n_wires = 0"); }
    { tiny t; t.n_wires = (1ull << 32) + 1; expect_rejected(t, "n_wires above 2^32"); }
    { tiny t; t.row_ptr[0] = 1; expect_rejected(t, "row_ptr[0] != 0"); }
    { tiny t; t.row_ptr[3] = 1; expect_rejected(t, "row_ptr decreasing in the middle"); }
    { tiny t; t.row_ptr[3] = 1ull << 63; expect_rejected(t, "row_ptr with a huge entry in the middle"); }
    { tiny t; t.row_ptr[6] = 3; expect_rejected(t, "last entry below nnz"); }
    { tiny t; t.row_ptr[6] = 5; expect_rejected(t, "last entry above nnz"); }
    { tiny t; t.wire[3] = 2; expect_rejected(t, "wire = n_wires"); }
    { tiny t; t.coeff[1] = 1; expect_rejected(t, "coefficient id = n_coeff"); }
    { tiny t; memcpy(t.coeffs.data(), R_WORDS, 32); expect_rejected(t, "coefficient = r"); }
    { tiny t; t.coeffs[3] = ~0ull; expect_rejected(t, "coefficient above r"); }
    {
        tiny t;                                              // r - 1 is a coefficient
        memcpy(t.coeffs.data(), R_WORDS, 32);
        t.coeffs[0] -= 1;
        EXPECT(t.create(&s) == ZKLC_OK, "coefficient = r - 1");
        r1cs_free_host(s);
    }
}

static std::vector<uint64_t> read_words(FILE *f, size_t n) {
    std::vector<uint64_t> v(n);
    if (n && fread(v.data(), 8, n, f) != n) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

static void from_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    const std::vector<uint64_t> hd = read_words(f, 6);
    const uint64_t nc = hd[0], n_wires = hd[1], nnz = hd[2], n_coeff = hd[3], n = hd[4], n_broken = hd[5];
    const std::vector<uint64_t> row_ptr = read_words(f, 3 * nc + 1);
    const std::vector<uint64_t> tw = read_words(f, (nnz + 1) / 2), tc = read_words(f, (nnz + 1) / 2);
    const std::vector<uint64_t> coeffs = read_words(f, 4 * n_coeff);
    // exact-length copies: a read behind nnz entries is out of bounds for the sanitizer
    std::vector<uint32_t> wire(nnz), coeff(nnz);
    memcpy(wire.data(), tw.data(), 4 * nnz);
    memcpy(coeff.data(), tc.data(), 4 * nnz);
    zklc_r1cs *s = nullptr;
    EXPECT(r1cs_build_host(nc, n_wires, row_ptr.data(), wire.data(), coeff.data(), nnz, coeffs.data(), (uint32_t)n_coeff, &s) == ZKLC_OK && s,
           "the system of the file is accepted");
    if (!s) return;
    for (uint64_t k = 0; k <= n_broken; k++) {
        const std::vector<uint64_t> w = read_words(f, 4 * n_wires), ea = read_words(f, 4 * n), eb = read_words(f, 4 * n),
                                    ec = read_words(f, 4 * n), es = read_words(f, 2);
        for (uint32_t threads : {1u, 3u, 0u}) {
            std::vector<r1cs_q> wa(2 * n_wires), a(2 * n), b(2 * n), c(2 * n);       // 16-byte aligned, exact length
            memcpy((void *)wa.data(), w.data(), 32 * n_wires);
            memset((void *)a.data(), 0xff, 32 * n), memset((void *)b.data(), 0xff, 32 * n), memset((void *)c.data(), 0xff, 32 * n);
            uint64_t sum[2] = {7, 7};
            EXPECT(zklc_r1cs_abc_host(s, (const uint64_t *)wa.data(), n, (uint64_t *)a.data(), (uint64_t *)b.data(), (uint64_t *)c.data(),
                                      ZKLC_R1CS_CHECK, threads, sum) == ZKLC_OK, "evaluation of the file's system");
            EXPECT(!memcmp(a.data(), ea.data(), 32 * n), "A w");
            EXPECT(!memcmp(b.data(), eb.data(), 32 * n), "B w");
            EXPECT(!memcmp(c.data(), ec.data(), 32 * n), "C w");
            EXPECT(sum[0] == es[0] && sum[1] == es[1], "summary");
        }
    }
    fclose(f);
    r1cs_free_host(s);
}

int main(int argc, char **argv) {
    malformed();
    if (argc > 1) from_file(argv[1]);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("r1cs host: ok\n");
    return 0;
}
