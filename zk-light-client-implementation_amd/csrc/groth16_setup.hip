// The scalar stage of groth16.Setup on gfx950 + C ABI (groth16_setup.cuh).  Per call, on one stream:
//   setup_index_kernel<G, false>   the transposed index, pass 1: the rows of one length bin of the resident system (the bins and row
//                                  lists of r1cs_eval), every term counted under its column (matrix, wire) with integer atomics.  The
//                                  lanes of a wave that share the first open lane's column are counted by ONE atomic, for up to
//                                  SETUP_AGG_ROUNDS leaders (the constant and the public wires: every lane of a wave on one column);
//                                  the lanes left over add by themselves.
//   setup_scan_*_kernel            exclusive scan of the 3 n_wires counts (tiles of 2048 in LDS, the tile sums by one workgroup), and
//                                  with its last pass the columns binned by length: lists for 1 / 8 / 64 lanes per column and the
//                                  long columns with their segments, filled through per-wave ballots and one atomic per bin and wave.
//   -- the host reads the five list sizes (the only wait of the call) --
//   setup_index_kernel<G, true>    pass 2: every term to its place in its column, the wire field replaced by the constraint index.
//                                  The order inside a column is whatever the atomics give; the sums below are canonical, so it shows
//                                  in no output.
//   setup_powers_kernel            one lane per run of SETUP_RUN exponents: tau^e into the transform's buffer, z in regular form
//   (zklc_bn254_fr_ntt_dev)        the inverse transform of the powers: L_j = (1/n) sum_k tau^k w^(-jk), no inversion, no special case
//   setup_cols_kernel<1|8|64>      the row-sum lanes of r1cs_eval.cuh over a column, L in the witness's place, butterfly of __shfl_xor
//   setup_segs_kernel              a wave per segment of SETUP_SEG_TERMS terms of a long column, partial sums into the workspace
//   setup_long_kernel              one lane per long column: the sum of its partial sums
//   setup_combine_kernel           one lane per wire: k from a_t, b_t, c_t; a_t, b_t, k into regular form
#include "groth16_setup.cuh"
#include "zklc_internal.h"

#define SETUP_LANES 256u
#define SETUP_SCAN_ITEMS 8u
#define SETUP_SCAN_TILE (SETUP_LANES * SETUP_SCAN_ITEMS)
#define SETUP_MAX_GRID 0x7fffffffull
// the head of the workspace: columns in bins 0..3, segments, as the device counted them (what zklc_groth16_setup_plan gives)
#define SETUP_N_COUNTERS 8u

ZKLC_D u64 setup_shfl64(u64 v, u32 src) {
    const u32 lo = (u32)__shfl((int)(u32)v, (int)src, 64), hi = (u32)__shfl((int)(u32)(v >> 32), (int)src, 64);
    return (u64)hi << 32 | lo;
}
ZKLC_D u64 setup_lanes_below() { return (1ull << (threadIdx.x & 63u)) - 1; }

// SCATTER = false: cursor[key] += 1 per term.  SCATTER = true: cursor[key] (the column's start after the scan) hands out places.
template <u32 G, bool SCATTER>
__global__ void __launch_bounds__(SETUP_LANES)
setup_index_kernel(const u64 *__restrict__ terms, const u64 *__restrict__ row_ptr, const u32 *__restrict__ perm, u64 n_rows, u64 nc,
                   u64 n_wires, unsigned long long *__restrict__ cursor, u64 *__restrict__ tterms) {
    const u64 slot = ((u64)blockIdx.x * SETUP_LANES + threadIdx.x) / G;
    const u32 sub = threadIdx.x % G, lane = threadIdx.x & 63u;
    u64 begin = 0, len = 0, m = 0;
    u32 j = 0;
    if (slot < n_rows) {
        const u64 row = perm[slot];
        begin = row_ptr[row];
        len = row_ptr[row + 1] - begin;
        m = row / nc;
        j = (u32)(row % nc);
    }
    const u64 mine = len > sub ? (len - sub + G - 1) / G : 0;       // this lane's terms: begin + sub + it G
    for (u64 it = 0;; it++) {
        const bool act = it < mine;
        const u64 open = __ballot(act);                             // the same in every lane: the loop is uniform over the wave
        if (!open) break;
        u64 term = 0, key = 0, pos = 0;
        if (act) {
            term = terms[begin + sub + it * G];
            key = setup_key(m, n_wires, term);
        }
        bool done = !act;
        u64 rem = open;
        for (u32 r = 0; r < SETUP_AGG_ROUNDS && rem; r++) {
            const u32 leader = (u32)__ffsll((unsigned long long)rem) - 1;
            const u64 lkey = setup_shfl64(key, leader);
            const u64 same = __ballot(!done && key == lkey);        // the leader among them
            u64 base = 0;
            if (lane == leader) base = atomicAdd(cursor + lkey, (unsigned long long)__popcll(same));
            if (SCATTER) base = setup_shfl64(base, leader);
            if ((same >> lane) & 1) {
                pos = base + (u64)__popcll(same & setup_lanes_below());
                done = true;
            }
            rem &= ~same;
        }
        if (!done) pos = atomicAdd(cursor + key, 1ull);
        if (SCATTER && act) tterms[pos] = setup_transposed_term(term, j);
    }
}

// pass 1 of the scan: ptr[i] = the exclusive sum of count[..i) inside i's tile; tile_sum[tile] = the tile's total
__global__ void __launch_bounds__(SETUP_LANES)
setup_scan_tiles_kernel(const u64 *__restrict__ count, u64 n_items, u64 *__restrict__ ptr, u64 *__restrict__ tile_sum) {
    __shared__ u64 sh[SETUP_LANES];
    const u64 first = ((u64)blockIdx.x * SETUP_LANES + threadIdx.x) * SETUP_SCAN_ITEMS;
    u64 v[SETUP_SCAN_ITEMS], s = 0;
    for (u32 i = 0; i < SETUP_SCAN_ITEMS; i++) {
        v[i] = first + i < n_items ? count[first + i] : 0;
        s += v[i];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (u32 off = 1; off < SETUP_LANES; off <<= 1) {               // inclusive scan of the lanes' sums
        const u64 add = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    u64 run = sh[threadIdx.x] - s;
    for (u32 i = 0; i < SETUP_SCAN_ITEMS; i++) {
        if (first + i < n_items) ptr[first + i] = run;
        run += v[i];
    }
    if (threadIdx.x == SETUP_LANES - 1) tile_sum[blockIdx.x] = sh[threadIdx.x];
}

// pass 2: one workgroup, tile_sum -> its exclusive scan, 256 tiles at a time with a running carry
__global__ void __launch_bounds__(SETUP_LANES) setup_scan_sums_kernel(u64 *__restrict__ tile_sum, u64 n_tiles) {
    __shared__ u64 sh[SETUP_LANES];
    u64 carry = 0;
    for (u64 base = 0; base < n_tiles; base += SETUP_LANES) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < n_tiles ? tile_sum[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (u32 off = 1; off < SETUP_LANES; off <<= 1) {
            const u64 add = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n_tiles) tile_sum[i] = carry + sh[threadIdx.x] - v;
        carry += sh[SETUP_LANES - 1];
        __syncthreads();                                            // sh is written again by the next round
    }
}

// where the scan's last pass files the columns: lists[b] (capacity n_keys each) for bins 0..2; the long columns as
// key | first segment << 32, their segments as key | index in the column << 32
struct setup_lists {
    u32 *bin[3];
    u64 *long_cols, *segs;
    u64 long_cap, seg_cap;
};

// pass 3: col_ptr and cursor complete (cursor held the counts), and every column filed under its bin
__global__ void __launch_bounds__(SETUP_LANES)
setup_scan_finish_kernel(unsigned long long *__restrict__ cursor, u64 *__restrict__ col_ptr, const u64 *__restrict__ tile_sum, u64 n_keys,
                         unsigned long long *__restrict__ counters, setup_lists lists) {
    const u64 i = (u64)blockIdx.x * SETUP_LANES + threadIdx.x;
    const u32 lane = threadIdx.x & 63u;
    const bool in_range = i <= n_keys;                              // item n_keys: the end of the last column
    u64 len = 0;
    if (in_range) {
        len = i < n_keys ? cursor[i] : 0;
        const u64 p = col_ptr[i] + tile_sum[i / SETUP_SCAN_TILE];
        col_ptr[i] = p;
        cursor[i] = p;
    }
    const bool col = i < n_keys;
    const u32 bin = setup_bin_of(len);
    for (u32 b = 0; b < 4; b++) {
        const u64 same = __ballot(col && bin == b);                 // the same in every lane
        if (same) {
            const u32 leader = (u32)__ffsll((unsigned long long)same) - 1;
            u64 base = 0;
            if (lane == leader) base = atomicAdd(counters + b, (unsigned long long)__popcll(same));
            base = setup_shfl64(base, leader);
            const u64 pos = base + (u64)__popcll(same & setup_lanes_below());
            if ((same >> lane) & 1) {
                if (b < 3) {
                    lists.bin[b][pos] = (u32)i;
                } else {                                            // lists sized for the worst case; the bounds cost nothing
                    const u64 n_seg = setup_segments(len), seg0 = atomicAdd(counters + 4, (unsigned long long)n_seg);
                    if (pos < lists.long_cap) lists.long_cols[pos] = i | seg0 << 32;
                    for (u64 sidx = 0; sidx < n_seg && seg0 + sidx < lists.seg_cap; sidx++) lists.segs[seg0 + sidx] = i | sidx << 32;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(SETUP_LANES)
setup_powers_kernel(const setup_consts c, u64 n, u32 *__restrict__ pw, u32 *__restrict__ z) {
    const u64 run = (u64)blockIdx.x * SETUP_LANES + threadIdx.x;
    setup_powers_lane(c, n, run, pw, z);
}

template <u32 G>
__global__ void __launch_bounds__(SETUP_LANES)
setup_cols_kernel(const u64 *__restrict__ tterms, const u64 *__restrict__ col_ptr, const u32 *__restrict__ list, u64 n_cols,
                  const u32 *__restrict__ coeffs, const u32 *__restrict__ L, u32 *__restrict__ abc_t) {
    const u64 slot = ((u64)blockIdx.x * SETUP_LANES + threadIdx.x) / G;
    const u32 sub = threadIdx.x % G;
    const bool live = slot < n_cols;                                // a group is live or not as a whole: G divides the workgroup
    u64 key = 0, begin = 0, end = 0;
    if (live) {
        key = list[slot];
        begin = col_ptr[key];
        end = col_ptr[key + 1];
    }
    r1cs_el s = r1cs_row_sum(tterms, begin, end, sub, G, L, coeffs);
    for (u32 off = G >> 1; off; off >>= 1) {
        r1cs_el o;
        for (int i = 0; i < 8; i++) o.w[i] = (u32)__shfl_xor((int)s.w[i], (int)off, 64);
        s = r1cs_add(s, o);
    }
    if (live && sub == 0) r1cs_store(abc_t + 8 * key, s);
}

__global__ void __launch_bounds__(SETUP_LANES)
setup_segs_kernel(const u64 *__restrict__ tterms, const u64 *__restrict__ col_ptr, const u64 *__restrict__ segs, u64 n_segs,
                  const u32 *__restrict__ coeffs, const u32 *__restrict__ L, u32 *__restrict__ partial) {
    const u64 seg = ((u64)blockIdx.x * SETUP_LANES + threadIdx.x) / 64;
    const u32 sub = threadIdx.x & 63u;
    const bool live = seg < n_segs;
    u64 begin = 0, end = 0;
    if (live) {
        const u64 d = segs[seg], key = (u32)d;
        begin = col_ptr[key] + (d >> 32) * SETUP_SEG_TERMS;
        end = begin + SETUP_SEG_TERMS < col_ptr[key + 1] ? begin + SETUP_SEG_TERMS : col_ptr[key + 1];
    }
    r1cs_el s = r1cs_row_sum(tterms, begin, end, sub, 64, L, coeffs);
    for (u32 off = 32; off; off >>= 1) {
        r1cs_el o;
        for (int i = 0; i < 8; i++) o.w[i] = (u32)__shfl_xor((int)s.w[i], (int)off, 64);
        s = r1cs_add(s, o);
    }
    if (live && sub == 0) r1cs_store(partial + 8 * seg, s);
}

__global__ void __launch_bounds__(SETUP_LANES)
setup_long_kernel(const u64 *__restrict__ col_ptr, const u64 *__restrict__ long_cols, u64 n_long, const u32 *__restrict__ partial,
                  u32 *__restrict__ abc_t) {
    const u64 i = (u64)blockIdx.x * SETUP_LANES + threadIdx.x;
    if (i >= n_long) return;
    const u64 d = long_cols[i], key = (u32)d, seg0 = d >> 32, n_seg = setup_segments(col_ptr[key + 1] - col_ptr[key]);
    r1cs_el s = r1cs_zero();
    for (u64 k = 0; k < n_seg; k++) s = r1cs_add(s, r1cs_load(partial + 8 * (seg0 + k)));
    r1cs_store(abc_t + 8 * key, s);
}

__global__ void __launch_bounds__(SETUP_LANES)
setup_combine_kernel(const setup_consts c, u64 n_wires, u32 n_public, const u32 *__restrict__ abc_t, u32 *__restrict__ a_t,
                     u32 *__restrict__ b_t, u32 *__restrict__ k) {
    const u64 i = (u64)blockIdx.x * SETUP_LANES + threadIdx.x;
    if (i < n_wires) setup_combine_lane(c, i, n_wires, n_public, abc_t, a_t, b_t, k);
}

// ---- the workspace: offsets in bytes, every part on a 256-byte boundary ----
struct setup_layout {
    u64 counters, cursor, col_ptr, tile_sum, bin[3], long_cols, segs, tterms, L, ntt, abc_t, partial, total;
    u64 n_keys, n_tiles, long_cap, seg_cap, ntt_bytes;
};
static setup_layout setup_make_layout(const zklc_r1cs *s, u64 n) {
    setup_layout l;
    u64 at = 0;
    auto take = [&](u64 bytes) {
        const u64 o = at;
        at += (bytes + 255) & ~255ull;
        return o;
    };
    u32 log_n = 0;
    while ((1ull << log_n) < n) log_n++;
    l.n_keys = 3 * s->n_wires;
    l.n_tiles = (l.n_keys + 1 + SETUP_SCAN_TILE - 1) / SETUP_SCAN_TILE;
    l.long_cap = s->nnz / SETUP_SEG_TERMS + 1;                      // a long column has more than SETUP_SEG_TERMS terms
    l.seg_cap = 2 * (s->nnz / SETUP_SEG_TERMS) + 1;                 // and ceil(len / SEG) <= 2 len / SEG segments
    l.ntt_bytes = zklc_bn254_fr_ntt_workspace_bytes(log_n);
    l.counters = take(SETUP_N_COUNTERS * 8);
    l.cursor = take((l.n_keys + 1) * 8);
    l.col_ptr = take((l.n_keys + 1) * 8);
    l.tile_sum = take(l.n_tiles * 8);
    for (int b = 0; b < 3; b++) l.bin[b] = take(l.n_keys * 4);
    l.long_cols = take(l.long_cap * 8);
    l.segs = take(l.seg_cap * 8);
    l.tterms = take((s->nnz ? s->nnz : 1) * 8);
    l.L = take(n * 32);
    l.ntt = take(l.ntt_bytes);
    l.abc_t = take(l.n_keys * 32);
    l.partial = take(l.seg_cap * 32);
    l.total = at;
    return l;
}

extern "C" uint64_t zklc_groth16_setup_workspace_bytes(const zklc_r1cs *s, uint64_t n) {
    uint32_t log_n;
    if (!s || setup_check_sizes(s, 0, n, &log_n) != ZKLC_OK) return 0;
    return setup_make_layout(s, n).total;
}

// device events around the stages of the calling thread's last zklc_groth16_setup_scalars_dev: transposition (with the call's one
// wait), powers, Lagrange values, column sums, combination
#define SETUP_N_EVENTS 6
struct setup_events {
    hipEvent_t ev[SETUP_N_EVENTS] = {};
    int device = -1;
    bool recorded = false;
};
static thread_local setup_events setup_last;
static hipError_t setup_events_for(int device) {
    setup_last.recorded = false;
    if (setup_last.device == device) return hipSuccess;
    for (auto &e : setup_last.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    setup_last.device = -1;
    for (auto &e : setup_last.ev) {
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
    }
    setup_last.device = device;
    return hipSuccess;
}

extern "C" uint32_t zklc_groth16_setup_last_timings(double *out_ms, uint32_t cap) {
    if (!out_ms || !setup_last.recorded) return 0;
    if (hipEventSynchronize(setup_last.ev[SETUP_N_EVENTS - 1]) != hipSuccess) return 0;
    uint32_t k = 0;
    for (; k + 1 < SETUP_N_EVENTS && k < cap; k++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, setup_last.ev[k], setup_last.ev[k + 1]) != hipSuccess) break;
        out_ms[k] = ms;
    }
    return k;
}

static unsigned setup_blocks(u64 lanes) { return (unsigned)((lanes + SETUP_LANES - 1) / SETUP_LANES); }

template <bool SCATTER>
static void setup_index_launch(hipStream_t st, const zklc_r1cs *s, unsigned long long *cursor, u64 *tterms) {
    const u64 *terms = (const u64 *)s->d_terms, *row_ptr = (const u64 *)s->d_row_ptr;
    const u32 *perm = (const u32 *)s->d_perm;
    const u64 r0 = s->bin_rows[0], r1 = s->bin_rows[1], r2 = s->bin_rows[2], nc = s->n_constraints, nw = s->n_wires;
    const dim3 block(SETUP_LANES);
    if (r0) hipLaunchKernelGGL((setup_index_kernel<1, SCATTER>), dim3(setup_blocks(r0)), block, 0, st, terms, row_ptr, perm, r0, nc, nw,
                               cursor, tterms);
    if (r1) hipLaunchKernelGGL((setup_index_kernel<8, SCATTER>), dim3(setup_blocks(r1 * 8)), block, 0, st, terms, row_ptr, perm + r0, r1,
                               nc, nw, cursor, tterms);
    if (r2) hipLaunchKernelGGL((setup_index_kernel<64, SCATTER>), dim3(setup_blocks(r2 * 64)), block, 0, st, terms, row_ptr,
                               perm + r0 + r1, r2, nc, nw, cursor, tterms);
}

extern "C" int32_t zklc_groth16_setup_scalars_dev(zklc_ctx *ctx, void *stream, const zklc_r1cs *s, const uint64_t *toxic,
                                                  uint32_t n_public, uint64_t n, uint64_t *d_a_t, uint64_t *d_b_t, uint64_t *d_k,
                                                  uint64_t *d_z, void *d_workspace, uint64_t workspace_bytes) {
    uint32_t log_n = 0;
    if (!ctx || !s || s->device != ctx->device || setup_check_sizes(s, n_public, n, &log_n) != ZKLC_OK) return ZKLC_ERR_INVALID_ARG;
    if (!toxic || !d_a_t || !d_b_t || !d_k || !d_z || !d_workspace) return ZKLC_ERR_INVALID_ARG;
    if (((uintptr_t)d_a_t | (uintptr_t)d_b_t | (uintptr_t)d_k | (uintptr_t)d_z | (uintptr_t)d_workspace) & 15 || (uintptr_t)toxic & 7)
        return ZKLC_ERR_INVALID_ARG;
    const setup_layout l = setup_make_layout(s, n);
    if (workspace_bytes < l.total) return ZKLC_ERR_INVALID_ARG;
    const u64 nw = s->n_wires;
    if (setup_blocks(s->bin_rows[0]) > SETUP_MAX_GRID || (s->bin_rows[1] * 8 + 255) / 256 > SETUP_MAX_GRID ||
        (s->bin_rows[2] * 64 + 255) / 256 > SETUP_MAX_GRID || (l.n_keys * 64 + 255) / 256 > SETUP_MAX_GRID ||
        (l.seg_cap * 64 + 255) / 256 > SETUP_MAX_GRID)
        return ZKLC_ERR_INVALID_ARG;
    setup_consts c;
    if (!setup_prepare(toxic, log_n, &c)) {
        setup_wipe(&c, sizeof c);
        return ZKLC_ERR_INVALID_ARG;
    }
    // from here on the constants are wiped on every way out
    struct wiper {
        setup_consts *c;
        ~wiper() { setup_wipe(c, sizeof *c); }
    } wipe_on_exit = {&c};
    ZKLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = zklc_pick_stream(ctx, stream);
    char *ws = (char *)d_workspace;
    unsigned long long *counters = (unsigned long long *)(ws + l.counters), *cursor = (unsigned long long *)(ws + l.cursor);
    u64 *col_ptr = (u64 *)(ws + l.col_ptr), *tile_sum = (u64 *)(ws + l.tile_sum), *tterms = (u64 *)(ws + l.tterms);
    u32 *L = (u32 *)(ws + l.L), *abc_t = (u32 *)(ws + l.abc_t), *partial = (u32 *)(ws + l.partial);
    const setup_lists lists = {{(u32 *)(ws + l.bin[0]), (u32 *)(ws + l.bin[1]), (u32 *)(ws + l.bin[2])}, (u64 *)(ws + l.long_cols),
                               (u64 *)(ws + l.segs), l.long_cap, l.seg_cap};
    const dim3 block(SETUP_LANES);
    ZKLC_HIP(ctx, setup_events_for(ctx->device));
    hipEvent_t *ev = setup_last.ev;
    ZKLC_HIP(ctx, hipEventRecord(ev[0], st));
    // the transposed index, up to the sizes of its lists
    ZKLC_HIP(ctx, hipMemsetAsync(counters, 0, SETUP_N_COUNTERS * 8, st));
    ZKLC_HIP(ctx, hipMemsetAsync(cursor, 0, (l.n_keys + 1) * 8, st));
    setup_index_launch<false>(st, s, cursor, tterms);
    hipLaunchKernelGGL(setup_scan_tiles_kernel, dim3((unsigned)l.n_tiles), block, 0, st, (const u64 *)cursor, l.n_keys + 1, col_ptr, tile_sum);
    hipLaunchKernelGGL(setup_scan_sums_kernel, dim3(1), block, 0, st, tile_sum, l.n_tiles);
    hipLaunchKernelGGL(setup_scan_finish_kernel, dim3(setup_blocks(l.n_keys + 1)), block, 0, st, cursor, col_ptr, (const u64 *)tile_sum,
                       l.n_keys, counters, lists);
    ZKLC_HIP(ctx, hipGetLastError());
    u64 h[5] = {0, 0, 0, 0, 0};
    ZKLC_HIP(ctx, zklc_readback_async(h, counters, sizeof h, st));
    ZKLC_HIP(ctx, zklc_stream_wait(st));
    if (h[0] + h[1] + h[2] + h[3] != l.n_keys || h[3] > l.long_cap || h[4] > l.seg_cap) {
        ctx->last_err = "groth16 setup: the column lists contradict the system";
        return ZKLC_ERR_HIP;
    }
    setup_index_launch<true>(st, s, cursor, tterms);
    ZKLC_HIP(ctx, hipEventRecord(ev[1], st));
    // powers, z, and the Lagrange values in the powers' place
    hipLaunchKernelGGL(setup_powers_kernel, dim3(setup_blocks((n + SETUP_RUN - 1) / SETUP_RUN)), block, 0, st, c, n, L, (u32 *)d_z);
    ZKLC_HIP(ctx, hipGetLastError());
    ZKLC_HIP(ctx, hipEventRecord(ev[2], st));
    const int32_t rc = zklc_bn254_fr_ntt_dev(ctx, st, (uint64_t *)L, log_n, ZKLC_NTT_INVERSE, 0, ws + l.ntt, l.ntt_bytes);
    if (rc != ZKLC_OK) return rc;
    ZKLC_HIP(ctx, hipEventRecord(ev[3], st));
    // the per-wire sums
    const u32 *coeffs = (const u32 *)s->d_coeffs;
    if (h[0]) hipLaunchKernelGGL((setup_cols_kernel<1>), dim3(setup_blocks(h[0])), block, 0, st, (const u64 *)tterms, (const u64 *)col_ptr,
                                 (const u32 *)lists.bin[0], h[0], coeffs, (const u32 *)L, abc_t);
    if (h[1]) hipLaunchKernelGGL((setup_cols_kernel<8>), dim3(setup_blocks(h[1] * 8)), block, 0, st, (const u64 *)tterms,
                                 (const u64 *)col_ptr, (const u32 *)lists.bin[1], h[1], coeffs, (const u32 *)L, abc_t);
    if (h[2]) hipLaunchKernelGGL((setup_cols_kernel<64>), dim3(setup_blocks(h[2] * 64)), block, 0, st, (const u64 *)tterms,
                                 (const u64 *)col_ptr, (const u32 *)lists.bin[2], h[2], coeffs, (const u32 *)L, abc_t);
    if (h[3]) {
        hipLaunchKernelGGL(setup_segs_kernel, dim3(setup_blocks(h[4] * 64)), block, 0, st, (const u64 *)tterms, (const u64 *)col_ptr,
                           (const u64 *)lists.segs, h[4], coeffs, (const u32 *)L, partial);
        hipLaunchKernelGGL(setup_long_kernel, dim3(setup_blocks(h[3])), block, 0, st, (const u64 *)col_ptr, (const u64 *)lists.long_cols,
                           h[3], (const u32 *)partial, abc_t);
    }
    ZKLC_HIP(ctx, hipEventRecord(ev[4], st));
    hipLaunchKernelGGL(setup_combine_kernel, dim3(setup_blocks(nw)), block, 0, st, c, nw, n_public, (const u32 *)abc_t, (u32 *)d_a_t,
                       (u32 *)d_b_t, (u32 *)d_k);
    ZKLC_HIP(ctx, hipGetLastError());
    ZKLC_HIP(ctx, hipEventRecord(ev[5], st));
    setup_last.recorded = true;
    return ZKLC_OK;
}
