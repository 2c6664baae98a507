// Stand-alone check of csrc/gl_ntt_plan.h (no HIP, no Python), in two parts.
//
// a. The plan's conditions, for every logn 1..24, log_in in {logn, logn - 1, logn - 3}, tile pin in {0, 12, 13}, radix-2 on and off:
//    windows and groups that add up, 128-byte runs, tiles and LDS within the kernels' limits, table blocks that are disjoint, in order
//    and end at table_elems, a tile index map that is a bijection onto [0, 2^logn), and the zero-skip condition of the shift-twiddle
//    kernel implying that exactly the first eighth of every tile is non-zero input.  These are what the fixed arrays of struct
//    ntt_pass and the kernels' index arithmetic rely on.
// b. The plan run on the CPU: an emulation of gl_ntt_pass_g4_kernel (goldilocks.hip) -- the tile loaded through the index map, every
//    group with gl_ntt_group_regs and table entries placed by the shared layout helpers, the tile stored -- chained over the plan in
//    DIF and DIT order and compared with a plain radix-2 transform written here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gl_ntt_plan.h"
#include "goldilocks.cuh"
#include "goldilocks_ntt_group.cuh"

static long failures = 0;
#define CHECK(cond, ...)                                                                                                                 \
    do {                                                                                                                                 \
        if (!(cond)) {                                                                                                                   \
            if (failures++ < 20) {                                                                                                       \
                std::printf("FAIL %s: ", #cond);                                                                                         \
                std::printf(__VA_ARGS__);                                                                                                \
                std::printf("\n");                                                                                                       \
            }                                                                                                                            \
        }                                                                                                                                \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rng() {      // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------- a. plan conditions
static long plans_checked = 0;
static void check_plan(int logn, int log_in, int pin, bool radix2) {
    gl_ntt_plan plan;
    std::memset(&plan, 0xEE, sizeof plan);
    const bool load_shift = log_in != logn;
    const uint64_t n_inv = 0x1234567;
    const bool ok = gl_ntt_make_plan(logn, log_in, radix2, pin, true, load_shift, n_inv, &plan);
    CHECK(ok, "logn %d log_in %d pin %d radix2 %d", logn, log_in, pin, radix2);
    if (!ok) return;
    plans_checked++;
    const uint64_t n = 1ULL << logn;
    const int np = plan.n_passes;
    CHECK(np >= 1 && np <= GL_NTT_MAX_PASSES && np <= 3, "logn %d: %d passes", logn, np);
    CHECK(plan.tile_log == 12 || plan.tile_log == 13, "tile_log %d", plan.tile_log);
    if (radix2 || pin == 12) CHECK(plan.tile_log == 12, "logn %d pin %d radix2 %d: tile_log %d", logn, pin, radix2, plan.tile_log);
    if (!radix2 && pin == 13) CHECK(plan.tile_log == 13, "logn %d pin 13: tile_log %d", logn, plan.tile_log);
    if (np < 1 || np > GL_NTT_MAX_PASSES) return;
    int s = 0;
    uint64_t off = 0;
    for (int i = 0; i < np; i++) {
        const gl_ntt_plan_pass &pp = plan.pass[i];
        const ntt_pass &p = pp.p;
        const bool first = i == 0, last = i == np - 1;
        CHECK(p.logn == logn && p.s0 == s && p.k >= 1, "logn %d pass %d: logn %d s0 %d (want %d) k %d", logn, i, p.logn, p.s0, s, p.k);
        const int lowbits = logn - p.s0 - p.k, t = p.k + p.c + p.d;
        CHECK(gl_ntt_lowbits(p) == lowbits, "logn %d pass %d: gl_ntt_lowbits %d", logn, i, gl_ntt_lowbits(p));
        CHECK(lowbits >= 0 && (lowbits == 0) == last, "logn %d pass %d: %d bits below the window", logn, i, lowbits);
        if (!last) CHECK(p.c >= 4, "logn %d pass %d: c %d (runs shorter than 128 bytes)", logn, i, p.c);
        CHECK(p.c >= 0 && p.d >= 0 && p.c <= lowbits && p.d <= p.s0, "logn %d pass %d: c %d d %d", logn, i, p.c, p.d);
        CHECK(t <= plan.tile_log && plan.tile_log <= 13, "logn %d pass %d: tile 2^%d", logn, i, t);
        CHECK(pp.threads == (t > 12 ? 512u : 256u), "logn %d pass %d: tile 2^%d, %u threads", logn, i, t, pp.threads);
        CHECK(p.log_in == (first ? log_in : logn), "logn %d pass %d: log_in %d", logn, i, p.log_in);
        CHECK(p.scale_shift == (first && load_shift ? GL_SCALE_LO_LOG : 0), "logn %d pass %d: scale_shift %d", logn, i, p.scale_shift);
        CHECK(p.out_scale == (last ? n_inv : 1), "logn %d pass %d: out_scale", logn, i);
        CHECK(p.zskip_ok == 1, "logn %d pass %d: zskip_ok %d", logn, i, p.zskip_ok);
        // groups and their table blocks
        CHECK(p.ng >= 1 && p.ng <= 4, "logn %d pass %d: %d groups", logn, i, p.ng);
        int sum = 0;
        for (int j = 0; j < 4; j++) {
            if (j < p.ng) {
                CHECK(p.gsz[j] >= 1 && p.gsz[j] <= 4, "logn %d pass %d group %d: %d stages", logn, i, j, p.gsz[j]);
                CHECK(p.goff[j] == off, "logn %d pass %d group %d: block at %llu, previous ends at %llu", logn, i, j,
                      (unsigned long long)p.goff[j], (unsigned long long)off);
                const uint64_t block = ((1ULL << p.gsz[j]) - 1) << (logn - (p.s0 + sum) - p.gsz[j]);
                CHECK(gl_ntt_group_block_elems(logn, p.s0 + sum, p.gsz[j]) == block, "logn %d pass %d group %d: block size", logn, i, j);
                off += block;
                sum += p.gsz[j];
            } else {
                CHECK(p.gsz[j] == 0 && p.goff[j] == 0, "logn %d pass %d: unused group %d is %d / %llu", logn, i, j, p.gsz[j],
                      (unsigned long long)p.goff[j]);
            }
        }
        CHECK(sum == p.k, "logn %d pass %d: groups sum to %d, k %d", logn, i, sum, p.k);
        // launch shape
        const uint32_t tile_n = 1u << t;
        CHECK(pp.lds_g4 == (tile_n + tile_n / 16) * 8 && pp.lds_g4 <= 72 * 1024, "logn %d pass %d: %u bytes of LDS (g4)", logn, i, pp.lds_g4);
        CHECK(pp.lds_r8 == (tile_n + tile_n / 8) * 8 && pp.lds_r8 <= 72 * 1024, "logn %d pass %d: %u bytes of LDS (r8)", logn, i, pp.lds_r8);
        CHECK((uint64_t)pp.grid_x << t == n, "logn %d pass %d: %u tiles of 2^%d", logn, i, pp.grid_x, t);
        if (t > plan.tile_log || p.c < 0 || p.d < 0 || p.c > lowbits || (uint64_t)pp.grid_x << t != n) return;   // no index map to walk

        // the index map, one input bit at a time: every bit of (tile_id, e) lands on one bit of its own, together all logn bits
        uint64_t img_tile[32] = {}, img_e[32] = {}, cover = 0, tL, tH;
        for (int b = 0; b < logn - t; b++) {
            gl_ntt_tile_split(p, lowbits, 1ULL << b, &tL, &tH);
            img_tile[b] = gl_ntt_global_index(p, lowbits, tL, tH, 0);
        }
        for (int b = 0; b < t; b++) img_e[b] = gl_ntt_global_index(p, lowbits, 0, 0, 1u << b);
        CHECK(gl_ntt_global_index(p, lowbits, 0, 0, 0) == 0, "logn %d pass %d: element 0 of tile 0", logn, i);
        for (int b = 0; b < logn; b++) {
            const uint64_t im = b < t ? img_e[b] : img_tile[b - t];
            CHECK(im && !(im & (im - 1)) && !(cover & im), "logn %d pass %d: input bit %d -> %llx", logn, i, b, (unsigned long long)im);
            cover |= im;
        }
        CHECK(cover == n - 1, "logn %d pass %d: image bits %llx", logn, i, (unsigned long long)cover);
        auto by_bits = [&](uint64_t tile_id, uint32_t e) {
            uint64_t r = 0;
            for (int b = 0; b < t; b++) r |= (e >> b & 1) ? img_e[b] : 0;
            for (int b = 0; b < logn - t; b++) r |= (tile_id >> b & 1) ? img_tile[b] : 0;
            return r;
        };
        for (int q = 0; q < 64; q++) {      // ... and the map is the OR of its bits' images
            const uint64_t tile_id = rng() & (pp.grid_x - 1);
            const uint32_t e = (uint32_t)rng() & (tile_n - 1);
            gl_ntt_tile_split(p, lowbits, tile_id, &tL, &tH);
            CHECK(gl_ntt_global_index(p, lowbits, tL, tH, e) == by_bits(tile_id, e), "logn %d pass %d tile %llu e %u", logn, i,
                  (unsigned long long)tile_id, e);
        }
        // the kernel's zero-skip condition => exactly the elements e < tile_n / 8 of every tile are input below 2^log_in
        const bool zskip = p.s0 == 0 && p.d == 0 && logn - p.log_in == 3 && p.gsz[0] >= 3;
        if (zskip) {
            for (int b = 0; b < t; b++)
                CHECK((img_e[b] >> p.log_in != 0) == (b >= t - 3), "logn %d pass %d: element bit %d -> %llx, log_in %d", logn, i, b,
                      (unsigned long long)img_e[b], p.log_in);
            for (int b = 0; b < logn - t; b++)
                CHECK(img_tile[b] >> p.log_in == 0, "logn %d pass %d: tile bit %d -> %llx, log_in %d", logn, i, b,
                      (unsigned long long)img_tile[b], p.log_in);
        }
        if (logn <= 16) {                   // exhaustively
            std::vector<uint8_t> seen(n, 0);
            long bad = 0;
            for (uint64_t tile_id = 0; tile_id < pp.grid_x; tile_id++) {
                gl_ntt_tile_split(p, lowbits, tile_id, &tL, &tH);
                for (uint32_t e = 0; e < tile_n; e++) {
                    const uint64_t g = gl_ntt_global_index(p, lowbits, tL, tH, e);
                    if (g >= n || seen[g]) {
                        bad++;
                        continue;
                    }
                    seen[g] = 1;
                    if (zskip && (g < (1ULL << p.log_in)) != (e < tile_n / 8)) bad++;
                }
            }
            CHECK(bad == 0, "logn %d log_in %d pass %d: %ld elements off the bijection / the zero-skip eighth", logn, log_in, i, bad);
        }
        s += p.k;
    }
    CHECK(s == logn, "logn %d: windows sum to %d", logn, s);
    // launch order: DIF as laid out; DIT walks the passes backwards, and the first / last launch keep their roles
    for (int ii = 0; ii < np; ii++)
        for (int dit = 0; dit < 2; dit++) {
            int idx = -1;
            const ntt_pass q = gl_ntt_plan_launch_pass(&plan, ii, dit != 0, &idx);
            CHECK(idx == (dit ? np - 1 - ii : ii) && q.s0 == plan.pass[idx].p.s0 && q.k == plan.pass[idx].p.k && q.goff[0] == plan.pass[idx].p.goff[0],
                  "logn %d launch %d dit %d: pass %d", logn, ii, dit, idx);
            CHECK(q.log_in == (ii == 0 ? log_in : logn) && q.scale_shift == (ii == 0 && load_shift ? GL_SCALE_LO_LOG : 0) &&
                      q.out_scale == (ii == np - 1 ? n_inv : 1),
                  "logn %d launch %d dit %d: log_in %d scale_shift %d", logn, ii, dit, q.log_in, q.scale_shift);
        }
    CHECK(off == plan.table_elems, "logn %d: blocks end at %llu, table_elems %llu", logn, (unsigned long long)off,
          (unsigned long long)plan.table_elems);
}

static void check_all_plans() {
    const int pins[3] = {0, 12, 13};
    for (int logn = 1; logn <= ZKLC_GL_MAX_LOG; logn++)
        for (int dl : {0, 1, 3})
            for (int pin : pins)
                for (int radix2 = 0; radix2 < 2; radix2++)
                    if (logn - dl >= 0) check_plan(logn, logn - dl, pin, radix2 != 0);
    gl_ntt_plan plan;
    CHECK(!gl_ntt_make_plan(0, 0, false, 0, true, false, 1, &plan), "logn 0 accepted");
    CHECK(!gl_ntt_make_plan(-1, -1, false, 0, true, false, 1, &plan), "logn -1 accepted");
    CHECK(!gl_ntt_make_plan(ZKLC_GL_MAX_LOG + 1, 3, false, 0, true, false, 1, &plan), "logn 25 accepted");
    CHECK(!gl_ntt_make_plan(10, 11, false, 0, true, false, 1, &plan), "log_in > logn accepted");
    CHECK(!gl_ntt_make_plan(10, 10, false, 0, true, false, 1, nullptr), "null plan accepted");
    CHECK(gl_ntt_make_plan(ZKLC_GL_MAX_LOG, ZKLC_GL_MAX_LOG, false, 0, true, false, 1, &plan), "logn 24 refused");
}

// ---------------------------------------------------------------- b. the plan on the CPU
#define POISON 0x0123456789ABCDEFULL      // canonical; stands where the kernel's LDS or table holds nothing defined

// one group of a tile, as gl_ntt_group_lds does it (without the LDS padding, which is a matter of banks only)
template <int G, bool DIT, bool INV, int ZP, bool UNIT, bool LEAN>
static void emu_group(u64 *tile, const u64 *gtab, u64 nj, u64 J, u32 base, int pb_low) {
    constexpr int M = 1 << G;
    u64 x[M], t[M] = {};
    if (!UNIT)
        for (int m = 1; m < M; m++) t[m - 1] = gtab[gl_ntt_group_table_index((u32)m, nj, J)];
    for (int m = 0; m < (M >> ZP); m++) x[m] = tile[base | ((u32)m << pb_low)];
    for (int m = (M >> ZP); m < M; m++) x[m] = 0;
    gl_ntt_group_regs<G, DIT, INV, ZP, UNIT, LEAN>(x, t);
    for (int m = 0; m < M; m++) tile[base | ((u32)m << pb_low)] = x[m];
}

// One launch of gl_ntt_pass_g4_kernel<DIT, INV, LEAN> for one transform.  The choice of a group's form (zero-aware, unit, the
// compare-with-p at a shift by 0) MIRRORS the kernel's, which stays where it is; every form returns the same canonical values, so
// agreement with the plain transform is what is asserted.
template <bool DIT, bool INV, bool LEAN>
static void emu_pass(const ntt_pass &p, const u64 *tab, const u64 *scale_hi, const u64 *scale_lo, const u64 *src, u64 *dst) {
    const int tile_log = p.k + p.c + p.d, lowbits = gl_ntt_lowbits(p);
    const u32 tile_n = 1u << tile_log;
    bool zskip = false;
    if (!DIT) zskip = p.s0 == 0 && p.d == 0 && p.logn - p.log_in == 3 && p.gsz[0] >= 3 && p.zskip_ok;
    const u32 load_n = zskip ? tile_n >> 3 : tile_n;
    std::vector<u64> tile(tile_n);
    for (u64 tile_id = 0; tile_id < (1ULL << (p.logn - tile_log)); tile_id++) {
        u64 tileL, tileH;
        gl_ntt_tile_split(p, lowbits, tile_id, &tileL, &tileH);
        for (u32 e = 0; e < tile_n; e++) {
            if (e >= load_n) {
                tile[e] = POISON;
                continue;
            }
            const u64 g = gl_ntt_global_index(p, lowbits, tileL, tileH, e);
            u64 v = g < (1ULL << p.log_in) ? src[g] : 0;
            if (p.scale_shift && g < (1ULL << p.log_in))
                v = gl_mul(v, gl_mul(scale_hi[g >> p.scale_shift], scale_lo[g & ((1u << p.scale_shift) - 1)]));
            tile[e] = v;
        }
        for (int gg = 0; gg < p.ng; gg++) {
            const int gi_ = DIT ? (p.ng - 1 - gg) : gg;
            const int g = p.gsz[gi_];
            int t0 = 0;
            for (int q = 0; q < gi_; q++) t0 += p.gsz[q];
            const int mg = p.k - g - t0, pb_low = p.c + mg;
            const u64 nj = 1ULL << (mg + lowbits);
            const u64 *gtab = tab + p.goff[gi_];
            for (u32 gi = 0; gi < tile_n >> g; gi++) {
                const u32 base = gl_ntt_group_base(gi, pb_low, g);
                const u64 J = gl_ntt_group_J(p, lowbits, tileL, base, mg);
                u64 *tl = tile.data();
                if (LEAN && nj == 1) {
                    if (!DIT && zskip && gi_ == 0) {
                        if (g == 4) emu_group<4, DIT, INV, DIT ? 0 : 3, true, true>(tl, gtab, nj, J, base, pb_low);
                        else emu_group<3, DIT, INV, DIT ? 0 : 3, true, true>(tl, gtab, nj, J, base, pb_low);
                    } else if (g == 4) emu_group<4, DIT, INV, 0, true, true>(tl, gtab, nj, J, base, pb_low);
                    else if (g == 3) emu_group<3, DIT, INV, 0, true, true>(tl, gtab, nj, J, base, pb_low);
                    else if (g == 2) emu_group<2, DIT, INV, 0, true, true>(tl, gtab, nj, J, base, pb_low);
                    else emu_group<1, DIT, INV, 0, true, true>(tl, gtab, nj, J, base, pb_low);
                } else if (!DIT && zskip && gi_ == 0) {
                    if (g == 4) emu_group<4, DIT, INV, DIT ? 0 : 3, false, LEAN>(tl, gtab, nj, J, base, pb_low);
                    else emu_group<3, DIT, INV, DIT ? 0 : 3, false, LEAN>(tl, gtab, nj, J, base, pb_low);
                } else if (g == 4) emu_group<4, DIT, INV, 0, false, LEAN && DIT>(tl, gtab, nj, J, base, pb_low);
                else if (g == 3) emu_group<3, DIT, INV, 0, false, LEAN>(tl, gtab, nj, J, base, pb_low);
                else if (g == 2) emu_group<2, DIT, INV, 0, false, LEAN>(tl, gtab, nj, J, base, pb_low);
                else emu_group<1, DIT, INV, 0, false, LEAN>(tl, gtab, nj, J, base, pb_low);
            }
        }
        for (u32 e = 0; e < tile_n; e++)
            dst[gl_ntt_global_index(p, lowbits, tileL, tileH, e)] = p.out_scale != 1 ? gl_mul(tile[e], p.out_scale) : tile[e];
    }
}

struct transform {
    int logn, log_in;
    bool dit, inverse, lean, zskip_ok;
    int pin;
    u64 shift;      // coset shift of the load scale, 0 = none
};

static std::vector<u64> powers(u64 base, u64 count) {
    std::vector<u64> r(count);
    u64 x = 1;
    for (u64 i = 0; i < count; i++, x = gl_mul(x, base)) r[i] = x;
    return r;
}

static std::vector<u64> test_input(u64 count) {
    std::vector<u64> a(count);
    for (u64 &v : a) v = rng() % GL_P;
    const u64 edge[5] = {0, 1, GL_P - 1, 0xFFFFFFFFULL, 1ULL << 32};
    for (u64 i = 0; i < 5 && i < count; i++) a[(i * 7) % count] = edge[i];      // distinct places whenever count > 4
    return a;
}

// plain radix-2 transforms in place; wpow[i] = w^i.  DIF: natural in -> bit-reversed out; DIT: bit-reversed in -> natural out
static void ref_dif(std::vector<u64> &a, int logn, const std::vector<u64> &wpow) {
    const u64 n = 1ULL << logn;
    for (int s = 0; s < logn; s++) {
        const u64 h = n >> (s + 1);
        for (u64 blk = 0; blk < n; blk += 2 * h)
            for (u64 j = 0; j < h; j++) {
                const u64 u = a[blk + j], v = a[blk + j + h];
                a[blk + j] = gl_add(u, v);
                a[blk + j + h] = gl_mul(gl_sub(u, v), wpow[j << s]);
            }
    }
}
static void ref_dit(std::vector<u64> &a, int logn, const std::vector<u64> &wpow) {
    const u64 n = 1ULL << logn;
    for (int s = logn - 1; s >= 0; s--) {
        const u64 h = n >> (s + 1);
        for (u64 blk = 0; blk < n; blk += 2 * h)
            for (u64 j = 0; j < h; j++) {
                const u64 u = a[blk + j], v = gl_mul(a[blk + j + h], wpow[j << s]);
                a[blk + j] = gl_add(u, v);
                a[blk + j + h] = gl_sub(u, v);
            }
    }
}
static u64 bitrev(u64 i, int bits) {
    u64 r = 0;
    for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
    return r;
}
// the plain transforms against the definition  X_i = sum_j a_j w^(i j)
static void check_reference() {
    for (int logn = 1; logn <= 6; logn++) {
        const u64 n = 1ULL << logn;
        const std::vector<u64> wpow = powers(gl_root_of_unity((u32)logn), n), a = test_input(n);
        std::vector<u64> dif = a, dit(n);
        for (u64 j = 0; j < n; j++) dit[bitrev(j, logn)] = a[j];
        ref_dif(dif, logn, wpow);
        ref_dit(dit, logn, wpow);
        for (u64 i = 0; i < n; i++) {
            u64 x = 0;
            for (u64 j = 0; j < n; j++) x = gl_add(x, gl_mul(a[j], wpow[(i * j) & (n - 1)]));
            CHECK(dif[bitrev(i, logn)] == x && dit[i] == x, "plain transforms, logn %d index %llu", logn, (unsigned long long)i);
        }
    }
}

static long transforms_run = 0;
static void run_transform(const transform &c) {
    const int logn = c.logn;
    const u64 n = 1ULL << logn, n_in = 1ULL << c.log_in;
    u64 w = gl_root_of_unity((u32)logn);
    if (c.inverse) w = gl_inv(w);
    const u64 n_inv = c.inverse ? gl_inv(n % GL_P) : 1;
    gl_ntt_plan plan;
    const bool ok = gl_ntt_make_plan(logn, c.log_in, false, c.pin, c.zskip_ok, c.shift != 0, n_inv, &plan);
    CHECK(ok, "plan of logn %d", logn);
    if (!ok) return;
    const std::vector<u64> wpow = powers(w, n);
    // the group table as gl_group_twiddle_kernel fills it: entry (m, J) of every group's block
    std::vector<u64> tab(plan.table_elems, POISON);
    for (int i = 0; i < plan.n_passes; i++) {
        const ntt_pass &p = plan.pass[i].p;
        int sf = p.s0;
        for (int j = 0; j < p.ng; sf += p.gsz[j++]) {
            const int g = p.gsz[j];
            const u64 nj = 1ULL << (logn - sf - g);
            for (u32 m = 1; m < (1u << g); m++)
                for (u64 J = 0; J < nj; J++) {
                    const u64 at = p.goff[j] + gl_ntt_group_table_index(m, nj, J), ex = gl_ntt_group_table_exponent(m, g, J, sf);
                    if (at >= plan.table_elems || ex >= n || tab[at] != POISON) {
                        CHECK(false, "logn %d pass %d group %d: table entry (%u, %llu) at %llu, exponent %llu", logn, i, j, m,
                              (unsigned long long)J, (unsigned long long)at, (unsigned long long)ex);
                        return;
                    }
                    tab[at] = wpow[ex];
                }
        }
    }
    std::vector<u64> scale_hi, scale_lo;
    if (c.shift) {
        scale_lo = powers(c.shift, 1ULL << GL_SCALE_LO_LOG);
        scale_hi = powers(gl_pow(c.shift, 1ULL << GL_SCALE_LO_LOG), c.log_in > GL_SCALE_LO_LOG ? n_in >> GL_SCALE_LO_LOG : 1);
    }
    const std::vector<u64> in = test_input(n_in);
    std::vector<u64> out(n, POISON);
    for (int ii = 0; ii < plan.n_passes; ii++) {      // the launch loop of gl_ntt_run
        int i;
        const ntt_pass p = gl_ntt_plan_launch_pass(&plan, ii, c.dit, &i);
        const u64 *src = ii == 0 ? in.data() : out.data();
        const u64 *sh = scale_hi.data(), *sl = scale_lo.data();
        switch ((c.dit ? 4 : 0) | (c.inverse ? 2 : 0) | (c.lean ? 1 : 0)) {
        case 0: emu_pass<false, false, false>(p, tab.data(), sh, sl, src, out.data()); break;
        case 1: emu_pass<false, false, true>(p, tab.data(), sh, sl, src, out.data()); break;
        case 2: emu_pass<false, true, false>(p, tab.data(), sh, sl, src, out.data()); break;
        case 3: emu_pass<false, true, true>(p, tab.data(), sh, sl, src, out.data()); break;
        case 4: emu_pass<true, false, false>(p, tab.data(), sh, sl, src, out.data()); break;
        case 5: emu_pass<true, false, true>(p, tab.data(), sh, sl, src, out.data()); break;
        case 6: emu_pass<true, true, false>(p, tab.data(), sh, sl, src, out.data()); break;
        default: emu_pass<true, true, true>(p, tab.data(), sh, sl, src, out.data()); break;
        }
    }
    // the same transform the plain way: pad, scale by shift^i, transform, scale by 1/n
    std::vector<u64> ref(n, 0);
    u64 sp = 1;
    for (u64 i = 0; i < n_in; i++) {
        ref[i] = c.shift ? gl_mul(in[i], sp) : in[i];
        if (c.shift) sp = gl_mul(sp, c.shift);
    }
    if (c.dit) ref_dit(ref, logn, wpow);
    else ref_dif(ref, logn, wpow);
    long bad = 0;
    for (u64 i = 0; i < n; i++) bad += out[i] != (c.inverse ? gl_mul(ref[i], n_inv) : ref[i]);
    CHECK(bad == 0, "logn %d log_in %d dit %d inverse %d lean %d zskip_ok %d pin %d (%d passes, tile 2^%d): %ld of %llu values differ",
          logn, c.log_in, c.dit, c.inverse, c.lean, c.zskip_ok, c.pin, plan.n_passes, plan.tile_log, bad, (unsigned long long)n);
    transforms_run++;
}

int main() {
    check_all_plans();
    check_reference();
    if (failures) {      // a plan that breaks its conditions is not run
        std::printf("ntt plan host: %ld FAILURES\n", failures);
        return 1;
    }
    const int pins[3] = {0, 12, 13};
    for (int pin : pins)
        for (int lean = 0; lean < 2; lean++) {
            for (int logn = 1; logn <= 16; logn++)
                for (int mode = 0; mode < 4; mode++)      // forward DIF, inverse DIF, forward DIT, inverse DIT
                    run_transform({logn, logn, (mode & 2) != 0, (mode & 1) != 0, lean != 0, true, pin, 0});
            for (int k = 0; k <= 13; k++)                 // 8x LDE with a coset shift: the general first group and the zero-aware one
                for (int zskip_ok = 0; zskip_ok < 2; zskip_ok++) run_transform({k + 3, k, false, false, lean != 0, zskip_ok != 0, pin, 7});
        }
    // three passes: the smallest plan under a pinned 2^12 tile in both builds, the smallest default one (2^23) in the plain build
    run_transform({21, 21, false, false, true, true, 12, 0});
    run_transform({21, 21, false, false, false, true, 12, 0});
#if !defined(__SANITIZE_ADDRESS__)
    run_transform({23, 23, false, false, true, true, 0, 0});
#endif
    if (failures) {
        std::printf("ntt plan host: %ld FAILURES\n", failures);
        return 1;
    }
    std::printf("plans checked: %ld, transforms run: %ld\n", plans_checked, transforms_run);
    std::printf("ntt plan host: ok\n");
    return 0;
}
