// TEST INFRASTRUCTURE: a stand-alone host program around the host form of p2_eval_poseidon_stmt (csrc/plonky2_gates.cuh) and the
// plain evaluator p2_eval_poseidon.  Built by tests/test_poseidon_gate_host.py with g++, once plain and once with
// -fsanitize=address,undefined; never linked into libzklc_mi355.so.
//
//   poseidon_gate_host ROWS.bin      ROWS.bin = u64 n, then n x { u64 expect (0 none, 1 zero, 2 non-zero), u64 wires[135] },
//                                               then u64 n_alpha, then n_alpha x u64 alpha[2]
// For every row and every pair of challenges: both evaluators must give the same two reductions; `expect` is checked on the
// statement form.  Prints "row pair acc0 acc1" of the statement form for the caller to hold against the oracle; exit 0 = all equal.
#include "../../zk-light-client-implementation_amd/csrc/plonky2_gates.cuh"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static const u32 NW = 135;

static void alpha_table(u64 a, std::vector<u32> &tab) {
    tab.resize(256 * 6);
    u64 pw = 1;
    for (int i = 0; i < 256; i++) {
        gl_limbs22(pw, &tab[6 * i]);
        pw = gl_mul(pw, a);
    }
}

template <bool STMT>
static void eval(const u64 *wires, const std::vector<u32> (&tab)[2], u64 *acc) {
    p2_vars v;
    v.wires = wires;
    v.consts = wires;
    v.stride = 1;
    v.p = 0;
    v.nsel = 0;
    for (int k = 0; k < 4; k++) v.pih[k] = 0;
    p2_consumer out;
    out.nch = 2;
    for (int c = 0; c < 2; c++) out.apow[c] = tab[c].data();
    out.reset(0);
    if (STMT)
        p2_eval_poseidon_stmt(v, out);
    else
        p2_eval_poseidon(v, out);
    if (out.k != 123) {
        fprintf(stderr, "evaluator emitted %u constraints, not 123\n", out.k);
        exit(3);
    }
    for (int c = 0; c < 2; c++) acc[c] = out.result(c);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    u64 n = 0, na = 0;
    if (fread(&n, 8, 1, f) != 1 || n > 4096) return 2;
    std::vector<u64> rows((size_t)n * (NW + 1));
    if (fread(rows.data(), 8, rows.size(), f) != rows.size()) return 2;
    if (fread(&na, 8, 1, f) != 1 || na > 16) return 2;
    std::vector<u64> alphas((size_t)na * 2);
    if (fread(alphas.data(), 8, alphas.size(), f) != alphas.size()) return 2;
    fclose(f);
    int bad = 0;
    for (u64 p = 0; p < na; p++) {
        std::vector<u32> tab[2];
        alpha_table(alphas[2 * p], tab[0]);
        alpha_table(alphas[2 * p + 1], tab[1]);
        for (u64 i = 0; i < n; i++) {
            const u64 expect = rows[i * (NW + 1)], *w = &rows[i * (NW + 1) + 1];
            u64 a[2], b[2];
            eval<true>(w, tab, a);
            eval<false>(w, tab, b);
            printf("%llu %llu %llu %llu\n", (unsigned long long)i, (unsigned long long)p, (unsigned long long)a[0], (unsigned long long)a[1]);
            if (a[0] != b[0] || a[1] != b[1]) {
                fprintf(stderr, "row %llu pair %llu: statement form differs from the plain evaluator\n", (unsigned long long)i, (unsigned long long)p);
                bad++;
            }
            const bool zero = a[0] == 0 && a[1] == 0;
            if ((expect == 1 && !zero) || (expect == 2 && zero)) {
                fprintf(stderr, "row %llu pair %llu: expected %s\n", (unsigned long long)i, (unsigned long long)p, expect == 1 ? "zero" : "non-zero");
                bad++;
            }
        }
    }
    return bad ? 1 : 0;
}
