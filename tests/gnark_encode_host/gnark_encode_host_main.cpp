// Stand-alone caller of csrc/gnark_points_encode_host.cpp (its own main, nothing else linked, no GPU, no Python): built by
// tests/test_gnark_encode_host.py with -fsanitize=address,undefined and run as a child process.  The two functions that file takes
// from the rest of the library are defined HERE, so that it links alone: the thread pool (p2v_parallel_for; the library's lives
// with the plonky2 verifier and its transcript) and the constants of the twist (g16_key_constants; the library's lives with the
// Groth16 verifier and the pairing) -- the second from the field code, as the library derives it: were it wrong, the valid G2
// points of the batches would be rejected under validation.  It makes every
// malformed call of include/zklc.h -- with arrays exactly as long as they claim, so that a read or write behind them is the
// sanitizer's to report -- then encodes the batches of the file named on the command line into buffers of exactly n x stride bytes
// and compares with the bytes, statuses and summary recorded there.  Exit 0: all as expected.
//
// File (little-endian u64): n_batches; per batch: g2, flags, n, words [n x 8 | 16], summary [4], then status [n] as u32 (padded to a
// multiple of 8 bytes) and the expected bytes [n x stride].
#include "../../zk-light-client-implementation_amd/csrc/gnark_points_encode.cuh"
#include "../../zk-light-client-implementation_amd/csrc/groth16_verifier_host.h"
#include "../../zk-light-client-implementation_amd/csrc/plonky2_verifier_host.h"
#include "../../include/zklc.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <thread>
#include <vector>

// fn(task) for every task < n on min(n, nthreads) threads (0 = 16)
void p2v_parallel_for(uint64_t n, uint32_t nthreads, const std::function<void(uint64_t)> &fn) {
    if (!nthreads) nthreads = 16;
    if (nthreads > n) nthreads = (uint32_t)n;
    std::atomic<uint64_t> next(0);
    auto work = [&] {
        for (uint64_t i = next++; i < n; i = next++) fn(i);
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nthreads; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

// twist_b = 3 / (9 + u); nothing else of the key is read by the encoder
const g16_key &g16_key_constants() {
    static const g16_key key = [] {
        g16_key k;
        memset(&k, 0, sizeof(k));
        const u32 nine[8] = {9, 0, 0, 0, 0, 0, 0, 0};
        const fp three = FP_THREE, one = FP_ONE;
        fp2 xi, t3;
        xi.c0 = g16_fp_from_words(nine);
        xi.c1 = one;
        t3.c0 = three;
        t3.c1 = fp_zero();
        k.twist_b = fp2_reduce(fp2_mul(t3, fp2_inv(xi)));
        return k;
    }();
    return key;
}

static int failures = 0;
#define EXPECT(cond, what)                                        \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "FAILED: %s (%s)\n", what, #cond);    \
            failures++;                                           \
        }                                                         \
    } while (0)

typedef int32_t (*enc_fn)(const uint64_t *, uint64_t, uint32_t, uint32_t, uint8_t *, uint32_t *, uint64_t *);
static enc_fn fn_of(bool g2) { return g2 ? zklc_bn254_g2_encode_host : zklc_bn254_g1_encode_host; }

// exactly `bytes` bytes, the sanitizer guards both ends; nothing for 0.  A multiple of 16 bytes sits at a 16-byte aligned address
// (words, bytes), anything else where malloc puts it (statuses: 4-byte alignment is all they need)
struct buf {
    uint8_t *p;
    size_t n;
    explicit buf(size_t bytes, uint8_t fill = 0) : p(nullptr), n(bytes) {
        if (!bytes) return;
        p = (uint8_t *)(bytes % 16 ? malloc(bytes) : aligned_alloc(16, bytes));
        if (!p) abort();
        memset(p, fill, bytes);
    }
    ~buf() { free(p); }
    bool all(uint8_t v) const {
        for (size_t i = 0; i < n; i++)
            if (p[i] != v) return false;
        return true;
    }
};

static void malformed() {
    const int32_t BAD = ZKLC_ERR_INVALID_ARG;
    for (int g2 = 0; g2 < 2; g2++) {
        const enc_fn enc = fn_of(g2);
        const size_t n = 4, width = g2 ? 16 : 8, stride = g2 ? 128 : 64;
        buf words(n * width * 8 + 16, 0), bytes(n * stride + 16, 0xA5), status(16, 0xA5), summary(32, 0xA5);
        uint64_t *w = (uint64_t *)words.p, *sum = (uint64_t *)summary.p;
        uint32_t *st = (uint32_t *)status.p;
        EXPECT(enc(w, n, 0, 1, bytes.p, st, nullptr) == BAD, "no summary");
        EXPECT(enc(nullptr, n, 0, 1, bytes.p, st, sum) == BAD, "no words");
        EXPECT(enc(w, n, 0, 1, nullptr, st, sum) == BAD, "no bytes");
        EXPECT(enc(w, n, 0, 1, bytes.p, nullptr, sum) == BAD, "no status");
        EXPECT(enc(w, n, ZKLC_POINTS_CHECK_SUBGROUP, 1, bytes.p, st, sum) == BAD, "the subgroup flag");
        EXPECT(enc(w, n, 8u, 1, bytes.p, st, sum) == BAD && enc(w, n, 0x80000000u, 1, bytes.p, st, sum) == BAD, "unknown flag bits");
        EXPECT(enc(w + 1, n, 0, 1, bytes.p, st, sum) == BAD, "misaligned words");
        EXPECT(enc(w, n, 0, 1, bytes.p + 8, st, sum) == BAD, "misaligned bytes");
        EXPECT(enc(w, 3, 0, 1, bytes.p, (uint32_t *)(status.p + 2), sum) == BAD, "misaligned status");
        EXPECT(enc(w, n, 0, 1, bytes.p, st, (uint64_t *)(summary.p + 4)) == BAD, "misaligned summary");
        EXPECT(enc(w, (1ull << 31) + 1, 0, 1, bytes.p, st, sum) == BAD, "too many points");
        EXPECT(bytes.all(0xA5) && status.all(0xA5) && summary.all(0xA5), "a refused call writes nothing");
        EXPECT(enc(nullptr, 0, ZKLC_POINTS_COMPRESSED | ZKLC_POINTS_VALIDATE, 1, nullptr, nullptr, sum) == ZKLC_OK, "an empty array");
        EXPECT(sum[0] == 0 && sum[1] == 0 && sum[2] == 0 && sum[3] == ~0ull, "the summary of an empty array");
        EXPECT(bytes.all(0xA5) && status.all(0xA5), "an empty array writes the summary alone");
    }
}

static bool read_exact(FILE *f, void *dst, size_t bytes) { return !bytes || fread(dst, 1, bytes, f) == bytes; }

static void batches(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        failures++;
        return;
    }
    uint64_t nb = 0;
    if (!read_exact(f, &nb, 8)) failures++;
    for (uint64_t b = 0; b < nb && !failures; b++) {
        uint64_t hdr[3], sum_want[4];
        if (!read_exact(f, hdr, 24)) {
            failures++;
            break;
        }
        const bool g2 = hdr[0] != 0;
        const uint32_t flags = (uint32_t)hdr[1];
        const uint64_t n = hdr[2], width = g2 ? 16 : 8, stride = (g2 ? 128u : 64u) >> (flags & ZKLC_POINTS_COMPRESSED);
        buf words(n * width * 8), want(n * stride), got(n * stride, 0x5A), st_want((n * 4 + 7) / 8 * 8), st(n * 4, 0x5A), sum(32, 0x5A);
        if (!read_exact(f, words.p, n * width * 8) || !read_exact(f, sum_want, 32) || !read_exact(f, st_want.p, st_want.n) ||
            !read_exact(f, want.p, n * stride)) {
            failures++;
            break;
        }
        for (uint32_t nthreads : {1u, 3u}) {
            EXPECT(fn_of(g2)((const uint64_t *)words.p, n, flags, nthreads, got.p, (uint32_t *)st.p, (uint64_t *)sum.p) == ZKLC_OK, "encoding");
            EXPECT(!n || !memcmp(got.p, want.p, n * stride), "bytes");
            EXPECT(!n || !memcmp(st.p, st_want.p, n * 4), "statuses");
            EXPECT(!memcmp(sum.p, sum_want, 32), "summary");
        }
        if (failures) fprintf(stderr, "batch %llu: g2 %d, flags %u, n %llu\n", (unsigned long long)b, (int)g2, flags, (unsigned long long)n);
    }
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
    printf("gnark encode host: ok\n");
    return 0;
}
