#pragma once
// controller_common.hip.h — what the two controller loops share (controller.hip: one action per node, one successor per (node,
// observation); controller_stoch.hip: drawn from candidates): the limits, what a narrow table holds for a refused entry, the
// straight-code table staging, and the refusals of the episode arguments both entry points read alike.
#include "kernels_common.hip.h"

namespace pomdp {

constexpr uint32_t CTRL_MAX_NODES = 4096, CTRL_MAX_EDGES = 16384;      // the header's limits: 4 KB + 32 KB of LDS
// what the narrow tables hold for an entry the contract refuses: an action that does not fit a byte (255 is out of range for
// every env, so it stays the invalid action it was — as_tape's rule for a tape byte) and a successor outside [0, n_nodes)
constexpr uint32_t CTRL_NO_ACTION = 0xFFu, CTRL_NO_NODE = 0xFFFFu;

// dst[i] = narrow(src[i]), i < count <= ROWS * BLOCK, by the whole workgroup: thread tid takes entries tid, tid + 256, ...  Straight
// code, no loop: eight rows of 256 entries at a time, their eight loads in flight together (a thread past the table's end reads
// its last entry and stores nothing), and a group that lies past the end is skipped, so a small table costs a few branches.
template <int ROWS, class T, class F>
static __device__ __forceinline__ void stage_narrow(T *dst, const int32_t *__restrict__ src, uint32_t count, F narrow)
{
    constexpr int G = 8;
    static_assert(ROWS % G == 0, "whole groups");
#pragma unroll
    for (int g = 0; g < ROWS / G; ++g) {
        const uint32_t base = (uint32_t)(g * G * BLOCK);
        if (base < count) {                                                     // workgroup-uniform
            uint32_t v[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t i = base + (uint32_t)(j * BLOCK) + threadIdx.x;
                v[j] = (uint32_t)src[i < count ? i : count - 1u];
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const uint32_t i = base + (uint32_t)(j * BLOCK) + threadIdx.x;
                if (i < count) dst[i] = (T)narrow(v[j]);
            }
        }
    }
}

} // namespace pomdp

// the env's observation count from its params (what a controller's `next` has a column for); 0 = unknown env
static inline int64_t env_obs_count(int env, const void *params)
{
    switch (env) {
    case POMDP_ENV_ROCK: return 3;
    case POMDP_ENV_TAG: return (int64_t)((const pomdp_tag_params *)params)->obs_cells + 1;
    case POMDP_ENV_BATTLESHIP: return 2;
    case POMDP_ENV_TIGER: return 3;
    case POMDP_ENV_NETWORK: return 3;
    default: return 0;
    }
}

// What both controller entry points refuse of `a` and k_steps, after their own checks of the controller (all POMDP_E_BADARG):
// everything pomdp_finish_episodes refuses, a tape, and params the env's kernels are not built for.  0 = fine.
static inline int controller_episode_args_check(const pomdp_episode_args *a, int64_t k_steps)
{
    if (!a || !a->params || !a->state || !a->done || k_steps < 0 || bad_range(a->n, a->lane0) || (a->lane0 & 3u) || a->tape)
        return POMDP_E_BADARG;
    const int64_t n = a->n;
    if (a->layout == POMDP_LAYOUT_RETURNS) {
        const pomdp_return_stats *st = a->stats;
        if (!st || !st->acc || !st->cnt || st->pitch < n || !(st->discount == st->discount)) return POMDP_E_BADARG;
    } else if (a->layout == POMDP_LAYOUT_PACKED || a->layout == POMDP_LAYOUT_NARROW) {
        if (!a->traj || a->pitch < n || (a->layout == POMDP_LAYOUT_NARROW && a->pitch % 4 != 0)) return POMDP_E_BADARG;
        // a Packed record (and a Narrow plane) keeps the observation in a byte: Tag's "opponent seen" value is a ctor argument
        if (a->env == POMDP_ENV_TAG && (uint32_t)((const pomdp_tag_params *)a->params)->obs_cells > 255u) return POMDP_E_BADPARAMS;
    } else {
        return POMDP_E_BADARG;                                          // frozen mode has no 13-byte layouts
    }
    return dispatch_env(a->env, a->params, [](auto, const auto &) { return 0; });
}
