// planner_common.hip.h — what the planner's translation units (planner.hip, planner_preferred.hip) share: the rollout loops'
// view of _generate_legal(), the policy tables, and the host-side argument checks.
#pragma once
#include "kernels_common.hip.h"

namespace pomdp {

// envs whose _generate_preferred reads extra LDS tables fill them with Env::stage_policy
template <class Env, class = void> struct HasPolicyTables : std::false_type {};
template <class Env> struct HasPolicyTables<Env, std::void_t<decltype(&Env::stage_policy)>> : std::true_type {};
template <class Env>
static __device__ __forceinline__ void stage_policy_tables(typename Env::Shared &sh, const typename Env::Params &p)
{
    if constexpr (HasPolicyTables<Env>::value) Env::stage_policy(sh, p, (int)threadIdx.x);
}

// _generate_legal() as the rollout loop uses it — the list's length, then its idx-th entry: envs that derive both from one
// intermediate form (Env::Legal, Env::legal_set, Env::legal_pick) compute it once per step, the others go through
// legal_count / legal_nth
template <class Env, class = void> struct LegalOf {
    struct Set { int count; };
    static __device__ __forceinline__ Set make(const typename Env::Shared &sh, const typename Env::Params &p,
                                               const typename Env::State &st, bool skip)
    {
        return Set{skip ? 0 : Env::legal_count(sh, p, st)};
    }
    static __device__ __forceinline__ int pick(const typename Env::Shared &sh, const typename Env::Params &p,
                                               const typename Env::State &st, const Set &, int idx)
    {
        return Env::legal_nth(sh, p, st, idx);
    }
};
template <class Env> struct LegalOf<Env, std::void_t<typename Env::Legal>> {
    using Set = typename Env::Legal;
    static __device__ __forceinline__ Set make(const typename Env::Shared &sh, const typename Env::Params &p,
                                               const typename Env::State &st, bool skip)
    {
        if (skip) return Set{};
        return Env::legal_set(sh, p, st);
    }
    static __device__ __forceinline__ int pick(const typename Env::Shared &sh, const typename Env::Params &,
                                               const typename Env::State &, const Set &L, int idx)
    {
        return Env::legal_pick(sh, L, idx);
    }
};

// RockSample's rollouts read the lane step from the (position, action) table of the fused loops, built once per launch
// (2.61 -> 2.73e11 steps/s on (15,15), 2.72 -> 2.80e11 on (7,8))
template <class Env, class = void> struct ROLLOUT_TAB : std::false_type {};
template <class Env> struct ROLLOUT_TAB<Env, typename std::enable_if<Env::QUAD_SENSOR && Env::QUAD_TAB>::type> : std::true_type {};

static inline bool belief_ok(const pomdp_rock_belief *b)
{
    return b && b->count && b->measured && b->lkv && b->lkw && b->prob_valuable && b->check_ok;
}
static inline bool history_ok(const pomdp_history *h, bool rock)
{
    if (!(h && h->size && h->last_action && h->last_ob && (!rock || (h->total_sample && h->total_move && h->move_ok)))) return false;
    if (h->max_size < -1 || h->max_size > 0x7FFFFFFE) return false;           // any window the caller has a (max_size + 1) x n byte ring for
    return h->max_size < 0 || !rock || (h->ring && h->head);                   // a bounded RockSample history keeps its window
}

} // namespace pomdp

static inline bool plan_out_ok(const pomdp_plan_out *o, int n_act)
{
    return o && o->q && o->visits && o->best && n_act >= 1 && n_act <= 255 && o->stride >= n_act;
}

