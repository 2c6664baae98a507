// Stand-alone caller of csrc/bn254_fixed_mul_host.cpp (its own main, nothing else linked, no GPU, no Python): built by
// tests/test_fixed_base_sanitized.py with -fsanitize=address,undefined and run as a child process.  It makes every malformed call of
// include/zklc.h -- with arrays exactly as long as they claim, so that a read or write behind them is the sanitizer's to report --
// then multiplies the batches of the file named on the command line and compares with the words recorded there.  Exit 0: all as
// expected.
//
// File (little-endian u64): n_batches; per batch: group, window_bits, n, scalars [n x 4], words [n x 8 | 16], summary [2].
#include "../../zk-light-client-implementation_amd/csrc/bn254_fixed_mul.cuh"
#include "../../include/zklc.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <utility>
#include <vector>

static int failures = 0;
#define EXPECT(cond, what)                                        \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "FAILED: %s (%s)\n", what, #cond);    \
            failures++;                                           \
        }                                                         \
    } while (0)

typedef int32_t (*mul_fn)(const zklc_fixed_base *, const uint64_t *, uint64_t, uint32_t, uint64_t *, uint64_t *);
static mul_fn mul_of(uint32_t group) { return group == ZKLC_GROUP_G2 ? zklc_bn254_g2_fixed_mul_host : zklc_bn254_g1_fixed_mul_host; }

// 16-byte aligned arrays of exactly n u64 (operator new aligns to 16 on this ABI; the sanitizer guards both ends)
struct buf {
    uint64_t *p;
    explicit buf(size_t n, uint64_t fill = 0) : p(new uint64_t[n ? n : 1]) {
        for (size_t i = 0; i < n; i++) p[i] = fill;
    }
    ~buf() { delete[] p; }
};

static void malformed() {
    zklc_fixed_base *t = (zklc_fixed_base *)1;
    EXPECT(fbm_build_host(2, nullptr, 8, &t) == ZKLC_ERR_INVALID_ARG && !t, "unknown group");
    EXPECT(fbm_build_host(ZKLC_GROUP_G1, nullptr, 3, &t) == ZKLC_ERR_INVALID_ARG && !t, "window below 4");
    EXPECT(fbm_build_host(ZKLC_GROUP_G2, nullptr, 17, &t) == ZKLC_ERR_INVALID_ARG && !t, "window above 16");
    EXPECT(fbm_build_host(ZKLC_GROUP_G1, nullptr, 4, nullptr) == ZKLC_ERR_INVALID_ARG, "no place for the table");
    {
        buf zero1(8), zero2(16);
        EXPECT(fbm_build_host(ZKLC_GROUP_G1, zero1.p, 4, &t) == ZKLC_ERR_INVALID_ARG && !t, "G1 base at infinity");
        EXPECT(fbm_build_host(ZKLC_GROUP_G2, zero2.p, 4, &t) == ZKLC_ERR_INVALID_ARG && !t, "G2 base at infinity");
    }
    EXPECT(zklc_bn254_fixed_mul_workspace_bytes(2, 5) == 0 && zklc_bn254_fixed_mul_workspace_bytes(0, (1ull << 30) + 1) == 0, "workspace of nothing");
    EXPECT(zklc_bn254_fixed_mul_workspace_bytes(ZKLC_GROUP_G1, 3) == 600 && zklc_bn254_fixed_mul_workspace_bytes(ZKLC_GROUP_G2, 3) == 1200, "workspace");
    EXPECT(zklc_bn254_fixed_base_table_bytes(ZKLC_GROUP_G1, 4) == 64ull * 15 * 64, "table bytes");
    for (uint32_t group = 0; group < 2; group++) {
        zklc_fixed_base *tab = nullptr, *other = nullptr;
        EXPECT(fbm_build_host(group, nullptr, 4, &tab) == ZKLC_OK && tab, "a table of the smallest window");
        EXPECT(fbm_build_host(1 - group, nullptr, 4, &other) == ZKLC_OK && other, "a table of the other group");
        if (!tab || !other) return;
        const size_t width = group ? 16 : 8;
        buf s(3 * 4, 5), w(3 * width, 9), sum(2, 9);
        const mul_fn mul = mul_of(group);
        EXPECT(mul(nullptr, s.p, 3, 1, w.p, sum.p) == ZKLC_ERR_INVALID_ARG, "no table");
        EXPECT(mul(other, s.p, 3, 1, w.p, sum.p) == ZKLC_ERR_INVALID_ARG, "a table of the other group");
        EXPECT(mul(tab, nullptr, 3, 1, w.p, sum.p) == ZKLC_ERR_INVALID_ARG, "no scalars");
        EXPECT(mul(tab, s.p, 3, 1, nullptr, sum.p) == ZKLC_ERR_INVALID_ARG, "no output");
        EXPECT(mul(tab, s.p, 3, 1, w.p, nullptr) == ZKLC_ERR_INVALID_ARG, "no summary");
        EXPECT(mul(tab, s.p + 1, 2, 1, w.p, sum.p) == ZKLC_ERR_INVALID_ARG, "misaligned scalars");
        EXPECT(mul(tab, s.p, 2, 1, w.p + 1, sum.p) == ZKLC_ERR_INVALID_ARG, "misaligned output");
        EXPECT(mul(tab, s.p, (1ull << 30) + 1, 1, w.p, sum.p) == ZKLC_ERR_INVALID_ARG, "too many scalars");
        bool untouched = sum.p[0] == 9 && sum.p[1] == 9;
        for (size_t i = 0; i < 3 * width; i++) untouched = untouched && w.p[i] == 9;
        EXPECT(untouched, "a refused call writes nothing");
        EXPECT(mul(tab, nullptr, 0, 1, nullptr, sum.p) == ZKLC_OK && sum.p[0] == 0 && sum.p[1] == ~0ull, "an empty batch");
        // three times the scalar 5: all three points equal and finite, whatever their place in the inversion group
        for (size_t i = 0; i < 12; i++) s.p[i] = i % 4 ? 0 : 5;
        EXPECT(mul(tab, s.p, 3, 0, w.p, sum.p) == ZKLC_OK && sum.p[0] == 0, "5 P three times");
        EXPECT(!memcmp(w.p, w.p + width, width * 8) && !memcmp(w.p, w.p + 2 * width, width * 8) && w.p[0] != 9, "the same point three times");
        delete tab;
        delete other;
    }
}

static bool read_u64(FILE *f, uint64_t *dst, size_t n) { return fread(dst, 8, n, f) == n; }

static void batches(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        failures++;
        return;
    }
    uint64_t nb = 0;
    if (!read_u64(f, &nb, 1)) failures++;
    std::map<std::pair<uint32_t, uint32_t>, zklc_fixed_base *> tables;
    for (uint64_t b = 0; b < nb && !failures; b++) {
        uint64_t hdr[3];
        if (!read_u64(f, hdr, 3)) {
            failures++;
            break;
        }
        const uint32_t group = (uint32_t)hdr[0], c = (uint32_t)hdr[1];
        const uint64_t n = hdr[2], width = group ? 16 : 8;
        buf s(n * 4), want(n * width), got(n * width, ~0ull), sum_want(2), sum(2, 7);
        if (!read_u64(f, s.p, n * 4) || !read_u64(f, want.p, n * width) || !read_u64(f, sum_want.p, 2)) {
            failures++;
            break;
        }
        zklc_fixed_base *&t = tables[{group, c}];
        if (!t) EXPECT(fbm_build_host(group, nullptr, c, &t) == ZKLC_OK && t, "table");
        if (!t) break;
        for (uint32_t nthreads : {1u, 3u}) {
            EXPECT(mul_of(group)(t, s.p, n, nthreads, got.p, sum.p) == ZKLC_OK, "multiplication");
            EXPECT(!memcmp(got.p, want.p, n * width * 8), "words");
            EXPECT(sum.p[0] == sum_want.p[0] && sum.p[1] == sum_want.p[1], "summary");
        }
        if (failures) fprintf(stderr, "batch %llu: group %u, window %u, n %llu\n", (unsigned long long)b, group, c, (unsigned long long)n);
    }
    for (auto &kv : tables) delete kv.second;
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s batches.bin\n", argv[0]);
        return 2;
    }
    malformed();
    batches(argv[1]);
    if (failures) return 1;
    printf("fixed base host: ok\n");
    return 0;
}
