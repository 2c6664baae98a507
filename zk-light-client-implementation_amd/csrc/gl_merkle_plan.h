// Launch plan of a Goldilocks Merkle commitment (zklc_gl_merkle_commit_strided): which kernel hashes which levels, in plain C++ with
// no HIP dependency, so that the host test (tests/merkle_tail_host) can walk every tree shape without a device.
//
// Level 0 is the leaf digests (2^log_leaves of them), level j has 2^(log_leaves - j) digests; the levels 0 .. log_leaves - cap_height
// are stored one after the other, four words per digest (zklc_gl_merkle_tree_words).  A launch produces the levels
// first_level .. first_level + n_levels - 1 from the level first_level - 1.
#pragma once
#include <stdint.h>

enum gl_merkle_kernel_kind : uint32_t {
    GL_MERKLE_LEVEL = 0,         // gl_merkle_level_kernel: one lane per parent, one level, 256 threads
    GL_MERKLE_TAIL = 1,          // gl_merkle_tail_kernel<T>: one lane per parent, a workgroup hashes 2T digests down level by level
    GL_MERKLE_LEVEL_COOP = 2,    // gl_merkle_level_coop_kernel: one 16-lane group per parent, one level
    GL_MERKLE_SUBTREE_COOP = 3,  // gl_merkle_subtree_coop_kernel: 16-lane groups, a workgroup hashes 32 digests down, <= 5 levels
};
enum gl_merkle_leaf_kind : uint32_t {
    GL_MERKLE_LEAVES_LANE = 0,   // gl_hash_leaves_kernel: one lane per leaf
    GL_MERKLE_LEAVES_COOP = 1,   // gl_hash_leaves_coop_kernel: one 16-lane group per leaf
};
enum gl_merkle_mode : uint32_t {
    GL_MERKLE_MODE_TAIL = 0,     // default: the tail kernel takes over from the per-level kernel at 2^14 parents and hands the levels
                                 // below 2^tail_min_log parents to the cooperative kernels; leaves as in GL_MERKLE_MODE_COOP
    GL_MERKLE_MODE_COOP = 1,     // ZKLC_MERKLE_TAIL=coop: cooperative kernels for every level and leaf array of <= 2^14 nodes
    GL_MERKLE_MODE_LANE = 2,     // ZKLC_NO_COOP_POSEIDON: the per-level lane kernels only
    GL_MERKLE_MODE_FULL = 3,     // ZKLC_MERKLE_TAIL=full: lane-per-permutation everywhere down to 16 parents / 64 leaves
};

// Why the default stops where it does (measured): one wave alone on a SIMD takes ~43 us for a lane-per-permutation level
// and ~19 us for a cooperative one, whatever the level's size.  Only where the cooperative groups stand several waves deep per SIMD
// -- the subtree launch over 2^15 children: four deep, all 16 groups of a workgroup running all five levels -- is the lane form
// also the faster one.  Below 2^12 parents the cooperative form is latency-bound, half the lane form's time, and a tree's few
// remaining permutations cost little either way.
#define GL_MERKLE_COOP_MAX_NODES (1u << 14)   // above this many parents the per-level kernel fills the chip: nothing to fuse
#define GL_MERKLE_TAIL_START_PARENTS (1u << 14)  // the default's tail launch starts at the hand-over from the per-level kernel only
#define GL_MERKLE_TAIL_MIN_LOG 12u            // ... and runs down to this many parents (log2)
#define GL_MERKLE_TAIL_MIN_PARENTS 16u        // GL_MERKLE_MODE_FULL: below, a partly filled wave costs more than the cooperative groups
#define GL_MERKLE_LANE_MIN_LEAVES 64u         // GL_MERKLE_MODE_FULL: below one wave of leaves the cooperative leaf kernel stays
#define GL_MERKLE_TAIL_MAX_LEVELS 11          // log2(2 * 1024): the largest workgroup
#define GL_MERKLE_MAX_LAUNCHES 32             // log_leaves <= 30: at most one launch per level

struct gl_merkle_launch {
    uint32_t kind;                                     // gl_merkle_kernel_kind
    uint32_t first_level;                              // first level produced, >= 1
    uint32_t n_levels;                                 // levels produced, >= 1
    uint32_t grid;                                     // workgroups
    uint32_t threads;                                  // threads per workgroup
    uint32_t n_children;                               // digests of level first_level - 1
    uint64_t off[GL_MERKLE_TAIL_MAX_LEVELS + 1];       // word offset of level first_level - 1 + j in the tree, j = 0 .. n_levels
};
struct gl_merkle_plan {
    uint32_t leaf_kind;                                // gl_merkle_leaf_kind
    uint32_t leaf_grid;                                // workgroups of 256 threads
    uint32_t n;                                        // launches after the leaf launch
    gl_merkle_launch launch[GL_MERKLE_MAX_LAUNCHES];
};

static inline uint32_t gl_merkle_log2(uint32_t x) {
    uint32_t l = 0;
    while ((1u << l) < x) l++;
    return l;
}

// word offset of level `level` of a tree of 2^log_leaves leaves (the layout of zklc_gl_merkle_tree_words)
static inline uint64_t gl_merkle_level_offset(uint32_t log_leaves, uint32_t level) {
    uint64_t words = 0;
    for (uint32_t l = 0; l < level; l++) words += 4ULL << (log_leaves - l);
    return words;
}

// `T` = threads of a tail workgroup (256, 512 or 1024); `fused` = false keeps one launch per level (ZKLC_MERKLE_FUSED=0);
// `tail_min_log`: GL_MERKLE_MODE_TAIL's last level has 2^tail_min_log parents (4 .. 14).  Returns false on arguments no tree has.
static inline bool gl_merkle_make_plan(uint32_t log_leaves, uint32_t cap_height, uint32_t T, uint32_t mode, bool fused,
                                       uint32_t tail_min_log, gl_merkle_plan *plan) {
    if (!plan || log_leaves > 30 || cap_height > log_leaves) return false;
    if (T != 256 && T != 512 && T != 1024) return false;
    if (mode > GL_MERKLE_MODE_FULL || tail_min_log < 4 || tail_min_log > 14) return false;
    const uint32_t n = 1u << log_leaves;
    const uint32_t total = log_leaves - cap_height;
    const bool coop_leaves = mode == GL_MERKLE_MODE_LANE   ? false
                             : mode == GL_MERKLE_MODE_FULL ? n < GL_MERKLE_LANE_MIN_LEAVES
                                                           : n <= GL_MERKLE_COOP_MAX_NODES;
    plan->leaf_kind = coop_leaves ? GL_MERKLE_LEAVES_COOP : GL_MERKLE_LEAVES_LANE;
    plan->leaf_grid = coop_leaves ? (n + 15) / 16 : (n + 255) / 256;
    plan->n = 0;
    const uint32_t tail_levels = gl_merkle_log2(2 * T);
    for (uint32_t l = 0; l < total;) {
        const uint32_t parents = n >> (l + 1);
        gl_merkle_launch *L = &plan->launch[plan->n++];
        L->first_level = l + 1;
        L->n_children = 2 * parents;
        uint32_t nlev = 1;
        if (mode == GL_MERKLE_MODE_LANE || parents > GL_MERKLE_COOP_MAX_NODES) {
            L->kind = GL_MERKLE_LEVEL;
        } else if (fused && mode == GL_MERKLE_MODE_TAIL && parents >= GL_MERKLE_TAIL_START_PARENTS) {
            // the hand-over from the per-level kernel: 2^14 parents down to 2^tail_min_log, or to the cap
            L->kind = GL_MERKLE_TAIL;
            nlev = gl_merkle_log2(parents) - tail_min_log + 1;
            if (nlev > tail_levels) nlev = tail_levels;
            if (nlev > total - l) nlev = total - l;
        } else if (mode == GL_MERKLE_MODE_FULL && parents >= GL_MERKLE_TAIL_MIN_PARENTS) {
            if (fused) {
                // everything from 2^14 parents down to the cap (or to one digest per workgroup, where a further launch joins the
                // workgroups' roots)
                L->kind = GL_MERKLE_TAIL;
                nlev = total - l < tail_levels ? total - l : tail_levels;
            } else {
                L->kind = GL_MERKLE_LEVEL;
            }
        } else if (fused && parents >= 16 && total - l >= 2) {
            // the cooperative levels in groups of up to five per launch: a workgroup hashes 32 digests down to one
            L->kind = GL_MERKLE_SUBTREE_COOP;
            nlev = total - l < 5 ? total - l : 5;
            while (nlev > 1 && ((2 * parents) >> nlev) == 0) nlev--;
        } else {
            L->kind = GL_MERKLE_LEVEL_COOP;
        }
        L->n_levels = nlev;
        switch (L->kind) {
        case GL_MERKLE_LEVEL:
            L->threads = 256;
            L->grid = (parents + 255) / 256;
            break;
        case GL_MERKLE_TAIL:
            L->threads = T;
            L->grid = (parents + T - 1) / T;
            break;
        case GL_MERKLE_LEVEL_COOP:
            L->threads = 256;
            L->grid = (parents + 15) / 16;
            break;
        default:
            L->threads = 256;
            L->grid = (2 * parents + 31) / 32;
            break;
        }
        uint64_t off = gl_merkle_level_offset(log_leaves, l);
        for (uint32_t j = 0; j <= nlev; j++) {
            L->off[j] = off;
            off += 4ULL << (log_leaves - l - j);
        }
        for (uint32_t j = nlev + 1; j <= GL_MERKLE_TAIL_MAX_LEVELS; j++) L->off[j] = 0;
        l += nlev;
    }
    return true;
}

// two-to-one permutations whose results a launch writes (for the accounting of instructions per result)
static inline uint64_t gl_merkle_launch_permutations(const gl_merkle_launch *L) {
    uint64_t p = 0;
    for (uint32_t j = 1; j <= L->n_levels; j++) p += L->n_children >> j;
    return p;
}
