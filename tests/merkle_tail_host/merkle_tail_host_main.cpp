// Stand-alone check of csrc/gl_merkle_plan.h (no HIP, no Python): for every log_leaves 0..24, cap_height 0..log_leaves, tail
// workgroup T in {256, 512, 1024}, every mode, several last levels of the default's tail and both settings of `fused`, the plan must
// produce every level
// 1 .. log_leaves - cap_height exactly once and in order, at the word offsets of zklc_gl_merkle_tree_words, with grids that cover
// all children and no empty launch.  The "written" counters below are an array of exactly log_leaves - cap_height + 1 levels, so that
// a level past the cap is an out-of-bounds access the sanitizers report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gl_merkle_plan.h"

// the layout as zklc_gl_merkle_tree_words (csrc/goldilocks.hip) states it
static uint64_t tree_words(uint32_t log_leaves, uint32_t cap_height) {
    uint64_t words = 0;
    for (uint32_t l = 0; l <= log_leaves - cap_height; l++) words += 4ULL << (log_leaves - l);
    return words;
}

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

static uint32_t children_per_group(const gl_merkle_launch &L) {
    switch (L.kind) {
    case GL_MERKLE_LEVEL: return 2 * L.threads;
    case GL_MERKLE_TAIL: return 2 * L.threads;
    case GL_MERKLE_LEVEL_COOP: return 2 * (L.threads / 16);
    default: return 32;
    }
}

static void check_tree(uint32_t log_leaves, uint32_t cap, uint32_t T, uint32_t mode, bool fused, uint32_t min_log, uint64_t *perms,
                       uint64_t *launches) {
    gl_merkle_plan plan;
    const bool ok = gl_merkle_make_plan(log_leaves, cap, T, mode, fused, min_log, &plan);
    CHECK(ok, "log %u cap %u T %u mode %u", log_leaves, cap, T, mode);
    if (!ok) return;
    const uint32_t total = log_leaves - cap, n = 1u << log_leaves;
    const uint64_t words = tree_words(log_leaves, cap);
    std::vector<uint32_t> written(total + 1, 0);                // how often each level of the tree was produced
    // leaves
    const uint32_t per_leaf_group = plan.leaf_kind == GL_MERKLE_LEAVES_COOP ? 16 : 256;
    CHECK(plan.leaf_grid >= 1 && (uint64_t)plan.leaf_grid * per_leaf_group >= n && (uint64_t)(plan.leaf_grid - 1) * per_leaf_group < n,
          "leaf grid %u for %u leaves", plan.leaf_grid, n);
    if (mode == GL_MERKLE_MODE_FULL)
        CHECK((plan.leaf_kind == GL_MERKLE_LEAVES_LANE) == (n >= 64), "leaf kind %u for %u leaves", plan.leaf_kind, n);
    if (mode == GL_MERKLE_MODE_TAIL || mode == GL_MERKLE_MODE_COOP)
        CHECK((plan.leaf_kind == GL_MERKLE_LEAVES_COOP) == (n <= GL_MERKLE_COOP_MAX_NODES), "leaf kind %u for %u leaves", plan.leaf_kind, n);
    if (mode == GL_MERKLE_MODE_LANE) CHECK(plan.leaf_kind == GL_MERKLE_LEAVES_LANE, "leaf kind %u", plan.leaf_kind);
    written[0] = 1;
    CHECK(plan.n <= GL_MERKLE_MAX_LAUNCHES, "%u launches", plan.n);
    uint32_t next_level = 1;
    for (uint32_t k = 0; k < plan.n; k++) {
        const gl_merkle_launch &L = plan.launch[k];
        CHECK(L.n_levels >= 1 && L.grid >= 1, "empty launch %u (log %u cap %u T %u)", k, log_leaves, cap, T);
        CHECK(L.first_level == next_level, "launch %u starts at level %u, expected %u", k, L.first_level, next_level);
        CHECK(L.first_level + L.n_levels - 1 <= total, "launch %u runs past the cap", k);
        if (L.n_levels < 1 || L.first_level != next_level || L.first_level + L.n_levels - 1 > total) return;
        CHECK(L.n_children == n >> (L.first_level - 1), "launch %u: %u children", k, L.n_children);
        const uint32_t per = children_per_group(L);
        // the grid covers every child and its last workgroup is not empty
        CHECK((uint64_t)L.grid * per >= L.n_children && (uint64_t)(L.grid - 1) * per < L.n_children, "launch %u: grid %u x %u for %u",
              k, L.grid, per, L.n_children);
        // a workgroup can hash its children down n_levels times, and a level of the launch is never empty
        CHECK((per >> L.n_levels) >= 1 || L.kind == GL_MERKLE_LEVEL || L.kind == GL_MERKLE_LEVEL_COOP, "launch %u: %u levels from %u",
              k, L.n_levels, per);
        CHECK((L.n_children >> L.n_levels) >= 1, "launch %u: level of no digests", k);
        if (L.kind == GL_MERKLE_LEVEL || L.kind == GL_MERKLE_LEVEL_COOP) CHECK(L.n_levels == 1, "per-level kernel with %u levels", L.n_levels);
        if (L.kind == GL_MERKLE_SUBTREE_COOP) CHECK(L.n_levels <= 5 && L.threads == 256, "subtree launch %u", k);
        if (L.kind == GL_MERKLE_TAIL) {
            CHECK(L.threads == T && L.n_levels <= GL_MERKLE_TAIL_MAX_LEVELS, "tail launch %u: %u threads", k, L.threads);
            CHECK((mode == GL_MERKLE_MODE_TAIL || mode == GL_MERKLE_MODE_FULL) && fused, "tail kernel under mode %u", mode);
            CHECK(L.n_children / 2 <= GL_MERKLE_COOP_MAX_NODES && L.n_children / 2 >= 16, "tail launch of %u children", L.n_children);
            if (mode == GL_MERKLE_MODE_TAIL) {
                // the default: only at the hand-over, and never below 2^min_log parents
                CHECK(L.n_children / 2 == GL_MERKLE_TAIL_START_PARENTS, "default tail launch of %u children", L.n_children);
                CHECK((L.n_children >> L.n_levels) >= (1u << min_log), "default tail down to %u parents", L.n_children >> L.n_levels);
            }
        }
        if (mode == GL_MERKLE_MODE_COOP || mode == GL_MERKLE_MODE_LANE) CHECK(L.kind != GL_MERKLE_TAIL, "tail under mode %u", mode);
        if (mode == GL_MERKLE_MODE_LANE) CHECK(L.kind == GL_MERKLE_LEVEL, "kind %u under the lane mode", L.kind);
        if (!fused) CHECK(L.n_levels == 1, "%u levels in a launch with fused off", L.n_levels);
        if (L.n_children / 2 > GL_MERKLE_COOP_MAX_NODES) CHECK(L.kind == GL_MERKLE_LEVEL, "kind %u for %u parents", L.kind, L.n_children / 2);
        // the hand-over: under `full` everything from 2^14 down to 16 parents is the tail kernel's, by default the launch at 2^14
        if (mode == GL_MERKLE_MODE_FULL && fused && L.n_children / 2 <= GL_MERKLE_COOP_MAX_NODES && L.n_children / 2 >= 16)
            CHECK(L.kind == GL_MERKLE_TAIL, "kind %u for %u parents", L.kind, L.n_children / 2);
        if (mode == GL_MERKLE_MODE_TAIL && fused && L.n_children / 2 == GL_MERKLE_TAIL_START_PARENTS)
            CHECK(L.kind == GL_MERKLE_TAIL, "kind %u at the hand-over", L.kind);
        // offsets: level first_level - 1 + j at the layout's place; the children were written before, the parents are written once
        for (uint32_t j = 0; j <= L.n_levels; j++) {
            const uint32_t level = L.first_level - 1 + j;
            uint64_t want = 0;
            for (uint32_t l = 0; l < level; l++) want += 4ULL << (log_leaves - l);
            CHECK(L.off[j] == want, "launch %u level %u at word %llu, layout says %llu", k, level, (unsigned long long)L.off[j],
                  (unsigned long long)want);
            if (L.off[j] != want) return;
            // the level lies inside the tree and does not overlap its neighbour
            CHECK(L.off[j] + (4ULL << (log_leaves - level)) <= words, "level %u ends past the tree", level);
            if (j == 0)
                CHECK(written[level] == 1, "level %u read before it is written", level);
            else
                CHECK(written[level]++ == 0, "level %u written twice", level);
        }
        *perms += gl_merkle_launch_permutations(&L);
        next_level = L.first_level + L.n_levels;
    }
    *launches += plan.n;
    CHECK(next_level == total + 1, "levels end at %u of %u", next_level - 1, total);
    for (uint32_t l = 0; l <= total; l++)
        CHECK(written[l] == 1, "level %u written %u times (log %u cap %u T %u mode %u)", l, written[l], log_leaves, cap, T, mode);
}

int main() {
    // arguments no tree has
    gl_merkle_plan plan;
    CHECK(!gl_merkle_make_plan(31, 0, 256, GL_MERKLE_MODE_TAIL, true, 12, &plan), "log_leaves 31 accepted");
    CHECK(!gl_merkle_make_plan(5, 6, 256, GL_MERKLE_MODE_TAIL, true, 12, &plan), "cap above the leaves accepted");
    CHECK(!gl_merkle_make_plan(5, 0, 128, GL_MERKLE_MODE_TAIL, true, 12, &plan), "T = 128 accepted");
    CHECK(!gl_merkle_make_plan(5, 0, 256, GL_MERKLE_MODE_TAIL, true, 3, &plan), "last level of 8 parents accepted");
    CHECK(!gl_merkle_make_plan(5, 0, 256, GL_MERKLE_MODE_TAIL, true, 15, &plan), "last level above the hand-over accepted");
    CHECK(!gl_merkle_make_plan(5, 0, 256, 4, true, 12, &plan), "mode 4 accepted");
    CHECK(!gl_merkle_make_plan(5, 0, 256, GL_MERKLE_MODE_TAIL, true, 12, nullptr), "no plan accepted");
    const uint32_t Ts[3] = {256, 512, 1024};
    const uint32_t mins[5] = {GL_MERKLE_TAIL_MIN_LOG, 4, 10, 13, 14};
    uint64_t trees = 0;
    for (uint32_t log_leaves = 0; log_leaves <= 24; log_leaves++)
        for (uint32_t cap = 0; cap <= log_leaves; cap++)
            for (uint32_t T : Ts)
                for (uint32_t mode = 0; mode < 4; mode++)
                    for (uint32_t mi = 0; mi < (mode == GL_MERKLE_MODE_TAIL ? 5u : 1u); mi++)
                        for (int fused = 0; fused < 2; fused++) {
                            uint64_t perms = 0, launches = 0;
                            check_tree(log_leaves, cap, T, mode, fused != 0, mins[mi], &perms, &launches);
                            // every plan hashes the same tree: 2^log_leaves - 2^cap_height two-to-one permutations
                            CHECK(perms == (1ULL << log_leaves) - (1ULL << cap), "%llu permutations", (unsigned long long)perms);
                            trees++;
                        }
    // dispatches: with the cap heights the provers use (0 .. 4 below 2^15 leaves leave the tail kernel out; 4 above), the default
    // plan launches no more kernels than the cooperative one
    for (uint32_t log_leaves = 4; log_leaves <= 24; log_leaves++) {
        gl_merkle_plan coop;
        gl_merkle_make_plan(log_leaves, 4, 256, GL_MERKLE_MODE_TAIL, true, GL_MERKLE_TAIL_MIN_LOG, &plan);
        gl_merkle_make_plan(log_leaves, 4, 256, GL_MERKLE_MODE_COOP, true, GL_MERKLE_TAIL_MIN_LOG, &coop);
        CHECK(plan.n <= coop.n, "2^%u leaves, cap 4: %u launches against %u", log_leaves, plan.n, coop.n);
    }
    // the default at the hand-over, 2^17 leaves, cap 4: two per-level launches, the tail kernel for 2^14, 2^13 and 2^12 parents in 64
    // workgroups, then the cooperative subtrees for 2^11 .. 2^7 and 2^6 .. 2^4
    gl_merkle_make_plan(17, 4, 256, GL_MERKLE_MODE_TAIL, true, GL_MERKLE_TAIL_MIN_LOG, &plan);
    CHECK(plan.n == 5 && plan.launch[0].kind == GL_MERKLE_LEVEL && plan.launch[1].kind == GL_MERKLE_LEVEL && plan.launch[2].kind == GL_MERKLE_TAIL &&
              plan.launch[2].first_level == 3 && plan.launch[2].n_levels == 3 && plan.launch[2].grid == 64 &&
              plan.launch[3].kind == GL_MERKLE_SUBTREE_COOP && plan.launch[3].n_levels == 5 && plan.launch[4].kind == GL_MERKLE_SUBTREE_COOP &&
              plan.launch[4].n_levels == 3,
          "hand-over at 2^17 leaves");
    // a tree of 2^14 leaves never sees the tail kernel by default
    gl_merkle_make_plan(14, 4, 256, GL_MERKLE_MODE_TAIL, true, GL_MERKLE_TAIL_MIN_LOG, &plan);
    CHECK(plan.n == 2 && plan.launch[0].kind == GL_MERKLE_SUBTREE_COOP && plan.launch[1].kind == GL_MERKLE_SUBTREE_COOP, "2^14 leaves");
    // ZKLC_MERKLE_TAIL=full: 2^15 digests, cap 4, is one tail launch at T = 1024 (T = 256: nine levels, then a single workgroup for
    // the last two); with cap 0 the single workgroup goes on to the root
    gl_merkle_make_plan(15, 4, 1024, GL_MERKLE_MODE_FULL, true, 12, &plan);
    CHECK(plan.n == 1 && plan.launch[0].kind == GL_MERKLE_TAIL && plan.launch[0].n_levels == 11 && plan.launch[0].grid == 16, "2^15 cap 4 T 1024");
    gl_merkle_make_plan(15, 0, 256, GL_MERKLE_MODE_FULL, true, 12, &plan);
    CHECK(plan.n == 2 && plan.launch[1].kind == GL_MERKLE_TAIL && plan.launch[1].grid == 1 && plan.launch[1].n_levels == 6, "2^15 cap 0 T 256");
    gl_merkle_make_plan(15, 4, 256, GL_MERKLE_MODE_FULL, true, 12, &plan);
    CHECK(plan.n == 2 && plan.launch[0].n_levels == 9 && plan.launch[0].grid == 64 && plan.launch[1].n_levels == 2 && plan.launch[1].grid == 1,
          "2^15 cap 4 T 256");
    if (failures) {
        std::printf("merkle tail host: %ld failures\n", failures);
        return 1;
    }
    std::printf("merkle tail host: ok (%llu plans)\n", (unsigned long long)trees);
    return 0;
}
