// heuristic_collect.hip — the heuristic-policy loop with a row per step (pomdp_heuristic_collect): heuristic_steps_kernel of
// heuristic_impl.hip.h instantiated with the record sinks, HeurPackedRows and HeurNarrowRows.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "heuristic_impl.hip.h"

extern "C" {

int pomdp_heuristic_collect(int env, const void *params, uint32_t *state, const pomdp_rock_belief *b, const pomdp_history *h,
                            int32_t *prev_ob, int32_t *action, int32_t *ob, void *reward, uint8_t *done,
                            const pomdp_returns *returns, void *traj, int64_t pitch, int layout, int64_t n, uint64_t seed,
                            uint32_t lane0, uint64_t t0, int64_t k_steps, int flags, void *stream)
{
    const int K = history_rocks(env, params);
    if (!heuristic_args_ok(K, params, state, b, h, prev_ob, action, ob, reward, done, returns, n, lane0, k_steps)) return POMDP_E_BADARG;
    if (!traj || pitch < n || (layout != POMDP_LAYOUT_PACKED && layout != POMDP_LAYOUT_NARROW)) return POMDP_E_BADARG;
    if (layout == POMDP_LAYOUT_NARROW && ((pitch & 3) || pitch > HEUR_NARROW_MAX_PITCH)) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        if (layout == POMDP_LAYOUT_PACKED)
            return launch_heuristic_steps<E, HeurPackedRows>(p, state, b, h, K, prev_ob, action, ob, reward, done, returns, n, seed, lane0,
                                                             t0, k_steps, flags, stream, HeurPackedRows::Arg{(uint8_t *)traj, pitch});
        return launch_heuristic_steps<E, HeurNarrowRows>(p, state, b, h, K, prev_ob, action, ob, reward, done, returns, n, seed, lane0,
                                                         t0, k_steps, flags, stream, HeurNarrowRows::Arg{(uint8_t *)traj, pitch});
    });
}

} // extern "C"
