// TEST INFRASTRUCTURE: the host forms of poseidon_gl_permute_keep<0/4/8>, poseidon_gl_hash_or_noop and poseidon_gl_two_to_one
// (csrc/poseidon_gl.cuh) as a stand-alone program, so that they run plain and under -fsanitize=address,undefined with nothing
// loaded into Python (tests/test_poseidon_tail_host.py).  Input file (little-endian u64):
//   n_states, n_states x 12 words;  n_inputs, n_inputs x (len, len words);  n_pairs, n_pairs x 8 words.
// Output lines:  "K i FIRST loose w0 w1 w2 w3" (the kept words; loose = 1: the form that skips the canonicalisation, reduced here),
//                "H i tail d0 d1 d2 d3" (tail = 0: the sponge of full permutations),  "T i tail d0 d1 d2 d3".
#include "../../zk-light-client-implementation_amd/csrc/poseidon_gl.cuh"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static bool read_words(FILE *f, u64 *dst, size_t n) { return fread(dst, sizeof(u64), n, f) == n; }

template <int FIRST, bool CANON>
static void keep_line(size_t i, const u64 *st) {
    u64 s[12];
    for (int k = 0; k < 12; k++) s[k] = st[k];
    poseidon_gl_permute_keep<FIRST, CANON>(s);
    printf("K %zu %d %d", i, FIRST, CANON ? 0 : 1);
    for (int k = 0; k < 4; k++) printf(" %llu", (unsigned long long)(CANON ? s[FIRST + k] : gl_canonical(s[FIRST + k])));
    printf("\n");
}

static void digest_line(const char *tag, size_t i, int tail, const u64 *d) {
    printf("%s %zu %d %llu %llu %llu %llu\n", tag, i, tail, (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2],
           (unsigned long long)d[3]);
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s vectors.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    u64 n;
    if (!read_words(f, &n, 1)) return 3;
    for (size_t i = 0; i < n; i++) {
        u64 st[12];
        if (!read_words(f, st, 12)) return 3;
        keep_line<0, true>(i, st);
        keep_line<4, true>(i, st);
        keep_line<8, true>(i, st);
        keep_line<0, false>(i, st);
        keep_line<4, false>(i, st);
        keep_line<8, false>(i, st);
    }
    if (!read_words(f, &n, 1)) return 3;
    for (size_t i = 0; i < n; i++) {
        u64 len;
        if (!read_words(f, &len, 1) || len > (1u << 20)) return 3;
        std::vector<u64> in(len);          // exactly `len` words: a read past the input is a heap overflow for the sanitizer
        if (len && !read_words(f, in.data(), len)) return 3;
        u64 d[4];
        poseidon_gl_hash_or_noop<true>(in.data(), 1, (u32)len, d);
        digest_line("H", i, 1, d);
        poseidon_gl_hash_or_noop<false>(in.data(), 1, (u32)len, d);
        digest_line("H", i, 0, d);
    }
    if (!read_words(f, &n, 1)) return 3;
    for (size_t i = 0; i < n; i++) {
        u64 lr[8], d[4];
        if (!read_words(f, lr, 8)) return 3;
        poseidon_gl_two_to_one<true>(lr, lr + 4, d);
        digest_line("T", i, 1, d);
        poseidon_gl_two_to_one<false>(lr, lr + 4, d);
        digest_line("T", i, 0, d);
    }
    fclose(f);
    return 0;
}
