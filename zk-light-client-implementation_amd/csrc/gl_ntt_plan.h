// Pass plan of a Goldilocks NTT / LDE (gl_ntt_run in goldilocks.hip): the split of the transform's stages into passes and of a pass
// into butterfly groups, every group's block in the group-twiddle table, the launch shape of every pass and the index maps of its
// kernels -- in plain C++ with no HIP dependency, so that the host test (tests/ntt_plan_host) can walk every accepted size and run
// the plan on the CPU without a device.
//
// One pass = k consecutive radix-2 stages of a size-2^logn transform, done in LDS on tiles of 2^(k+c+d) elements: all 2^k values of
// the k-bit index window the stages act on, times 2^c consecutive low indices (coalesced 8*2^c-byte runs), times 2^d high indices.
// Stage s (0-based from the top) pairs indices that differ in bit (logn-1-s).
//   DIF (forward order of stages): natural-order input -> bit-reversed output
//   DIT (reverse order of stages): bit-reversed input  -> natural-order output
// The plan is laid out in DIF order; a DIT run walks it backwards (gl_ntt_plan_launch_pass).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GL_NTT_HD __host__ __device__
#else
#define GL_NTT_HD
#endif

#define ZKLC_GL_MAX_LOG 24      // largest log2 of a transform (zklc_internal.h takes it from here)
#define NTT_THREADS 256
#define NTT_TILE_LOG_MAX 12
// the radix-8 and shift-twiddle pass kernels take their tile as dynamic LDS: 2^12 elements (256 threads) or 2^13 (512 threads)
#define NTT_TILE_LOG_BIG 13
#define NTT_THREADS_MAX 512
#define GL_SCALE_LO_LOG 10      // two-level table of coset-shift powers: shift^j = hi[j >> 10] * lo[j & 1023]
#define GL_NTT_MAX_PASSES 3     // logn <= 24 with a tile of 2^12: 12 + 8 + 4 (checked by the host test at every size)

// kernel argument: the layout must not move
struct ntt_pass {
    int logn, s0, k, c, d;
    int log_in;        // input indices >= 2^log_in read as zero (LDE zero padding); = logn otherwise
    int scale_shift;   // log2 of the low table size of the two-level load scale (0 = no load scale)
    uint64_t out_scale;  // multiplied into every stored value when != 1 (1/n of the inverse transform)
    // shift-twiddle kernel (gl_ntt_pass_g4_kernel): the k stages in ng groups of gsz[i] <= 4 stages (top stage first); goff[i] =
    // offset of the group's block in the table of per-element twiddles (gl_ntt_group_table_index)
    int ng, gsz[4];
    uint64_t goff[4];
    int zskip_ok;      // the zero-aware first group of an 8x LDE may be used (off: ZKLC_NTT_ZSKIP=0)
};

struct gl_ntt_plan_pass {
    ntt_pass p;
    uint32_t grid_x;   // tiles of one transform (grid y = batch)
    uint32_t threads;  // 256, or 512 for a tile of 2^13
    uint32_t lds_g4;   // dynamic LDS bytes of the shift-twiddle kernel: the tile + one pad per 16 elements
    uint32_t lds_r8;   // ... of the radix-8 kernel: one pad per 8 elements (the radix-2 kernel's tile is static)
};
struct gl_ntt_plan {
    int n_passes;          // <= GL_NTT_MAX_PASSES
    int tile_log;          // NTT_TILE_LOG_MAX or NTT_TILE_LOG_BIG
    uint64_t table_elems;  // entries of the group-twiddle table (depends on logn and the tile only)
    gl_ntt_plan_pass pass[GL_NTT_MAX_PASSES];
};

// entries of the table block of a group of g stages whose first stage is s_first: one per (m = 1 .. 2^g - 1, J < 2^(logn - s_first - g))
GL_NTT_HD static inline uint64_t gl_ntt_group_block_elems(int logn, int s_first, int g) {
    return ((1ULL << g) - 1) << (logn - s_first - g);
}

// Strided windows from the top (each leaves >= 4 low bits in the tile: 128-byte runs), then one contiguous window.  Tile of 2^12
// elements, or 2^13 where that saves a whole pass over the data (e.g. 2^21: two passes instead of three); tile_pin = 12 | 13 pins it
// (ZKLC_NTT_TILE, A/B), the radix-2 kernel's static tile is always 2^12.  `log_in`, `load_shift` (the first launch scales its loads)
// and `n_inv` (the last launch multiplies its stores; 1 = none) describe the first and the last pass.  Returns false on arguments no
// transform has.
static inline bool gl_ntt_make_plan(int logn, int log_in, bool radix2, int tile_pin, bool zskip_ok, bool load_shift, uint64_t n_inv,
                                    gl_ntt_plan *plan) {
    if (!plan || logn < 1 || logn > ZKLC_GL_MAX_LOG || log_in > logn) return false;
    auto n_passes = [&](int T) { return 1 + (logn > T ? (logn - T + (T - 4) - 1) / (T - 4) : 0); };
    int T = NTT_TILE_LOG_MAX;
    if (!radix2 && (tile_pin == NTT_TILE_LOG_BIG || (tile_pin == 0 && n_passes(NTT_TILE_LOG_BIG) < n_passes(NTT_TILE_LOG_MAX))))
        T = NTT_TILE_LOG_BIG;
    const int np = n_passes(T);
    if (np > GL_NTT_MAX_PASSES) return false;
    plan->n_passes = np;
    plan->tile_log = T;
    int ks[GL_NTT_MAX_PASSES], n = 0;
    const int k_last = logn < T ? logn : T;
    int remaining = logn - k_last;
    for (int m = np - 1; m > 0; m--) {      // even split of the strided bits
        int k = (remaining + m - 1) / m;
        ks[n++] = k;
        remaining -= k;
    }
    ks[n++] = k_last;
    uint64_t tab_elems = 0;
    int s0 = 0;
    for (int i = 0; i < np; i++) {
        gl_ntt_plan_pass *pp = &plan->pass[i];
        ntt_pass &p = pp->p;
        p.logn = logn;
        p.s0 = s0;
        p.k = ks[i];
        const int lowbits = logn - p.s0 - p.k;
        p.c = lowbits < (T - p.k) ? lowbits : (T - p.k);
        const int room = T - p.k - p.c;
        p.d = p.s0 < room ? p.s0 : room;
        const bool first = (i == 0), last = (i == np - 1);
        p.log_in = first ? log_in : logn;
        p.scale_shift = (first && load_shift) ? GL_SCALE_LO_LOG : 0;
        p.out_scale = last ? n_inv : 1;
        p.zskip_ok = zskip_ok ? 1 : 0;
        // groups of <= 4 stages (sizes as even as possible: 13 = 4 + 3 + 3 + 3) and their blocks in the twiddle table
        const int ng = (p.k + 3) / 4, base = p.k / ng, extra = p.k % ng;
        p.ng = ng;
        int t0 = 0;
        for (int j = 0; j < 4; j++) {
            const int g = j < ng ? base + (j < extra ? 1 : 0) : 0;
            p.gsz[j] = g;
            p.goff[j] = j < ng ? tab_elems : 0;
            if (j < ng) tab_elems += gl_ntt_group_block_elems(logn, p.s0 + t0, g);
            t0 += g;
        }
        const int tile_log = p.k + p.c + p.d;
        pp->grid_x = 1u << (logn - tile_log);
        pp->threads = tile_log > NTT_TILE_LOG_MAX ? NTT_THREADS_MAX : NTT_THREADS;
        pp->lds_g4 = ((1u << tile_log) + (1u << tile_log) / 16) * (uint32_t)sizeof(uint64_t);
        pp->lds_r8 = ((1u << tile_log) + (1u << tile_log) / 8) * (uint32_t)sizeof(uint64_t);
        s0 += p.k;
    }
    plan->table_elems = tab_elems;
    return true;
}

// The pass of launch number ii.  DIF walks pass[0 .. n_passes), DIT walks it backwards; what belongs to the first and to the last
// LAUNCH (zero padding and load scale, out_scale) stays with the position in the launch order.  *index = the entry of pass[].
static inline ntt_pass gl_ntt_plan_launch_pass(const gl_ntt_plan *plan, int ii, bool dit, int *index) {
    *index = dit ? plan->n_passes - 1 - ii : ii;
    ntt_pass p = plan->pass[*index].p;
    const ntt_pass &role = plan->pass[ii].p;
    p.log_in = role.log_in;
    p.scale_shift = role.scale_shift;
    p.out_scale = role.out_scale;
    return p;
}

// ---- index maps of the pass kernels (and of the host test's emulation of them).  `lowbits` = gl_ntt_lowbits(p), the index bits below
// the pass's window: the kernels hold it in a local and hand it in, so that it is derived once per kernel
GL_NTT_HD static inline int gl_ntt_lowbits(const ntt_pass &p) { return p.logn - p.s0 - p.k; }
// tile number -> its low part (which 2^c run of the low indices) and high part (which 2^d block of the indices above the window)
GL_NTT_HD static inline void gl_ntt_tile_split(const ntt_pass &p, int lowbits, uint64_t tile_id, uint64_t *tileL, uint64_t *tileH) {
    *tileL = tile_id & ((1ULL << (lowbits - p.c)) - 1);
    *tileH = tile_id >> (lowbits - p.c);
}
// element e of a tile -> index in the transform: e = (hid : d bits | mid : k bits | lowc : c bits)
GL_NTT_HD static inline uint64_t gl_ntt_global_index(const ntt_pass &p, int lowbits, uint64_t tileL, uint64_t tileH, uint32_t e) {
    uint64_t lowc = e & ((1u << p.c) - 1);
    uint64_t mid = (e >> p.c) & ((1u << p.k) - 1);
    uint64_t hid = e >> (p.c + p.k);
    uint64_t L = (tileL << p.c) | lowc;
    uint64_t H = (tileH << p.d) | hid;
    return (H << (lowbits + p.k)) | (mid << lowbits) | L;
}
// group number gi of a tile -> the tile element with group bits m = 0: the g group bits sit at pb_low, gi fills the others
GL_NTT_HD static inline uint32_t gl_ntt_group_base(uint32_t gi, int pb_low, int g) {
    return ((gi >> pb_low) << (pb_low + g)) | (gi & ((1u << pb_low) - 1));
}
// J = the transform-index bits below the group of the elements at `base`; mg = number of window bits below the group
GL_NTT_HD static inline uint64_t gl_ntt_group_J(const ntt_pass &p, int lowbits, uint64_t tileL, uint32_t base, int mg) {
    uint64_t lowc = base & ((1u << p.c) - 1);
    uint64_t mid_low = (base >> p.c) & ((1u << mg) - 1);
    return (mid_low << lowbits) | ((tileL << p.c) | lowc);
}
// layout of a group's table block (nj = 2^(index bits below the group)): entry (m, J), 1 <= m < 2^g, holds w^exponent
GL_NTT_HD static inline uint64_t gl_ntt_group_table_index(uint32_t m, uint64_t nj, uint64_t J) { return (uint64_t)(m - 1) * nj + J; }
GL_NTT_HD static inline uint64_t gl_ntt_group_table_exponent(uint32_t m, int g, uint64_t J, int s_first) {
    uint32_t r = 0;      // bitrev_g(m)
    for (int i = 0; i < g; i++) r |= ((m >> i) & 1u) << (g - 1 - i);
    return ((uint64_t)r * J) << s_first;
}
