// planner_common.hip.h — what the planner's translation units (planner.hip, planner_preferred.hip, heuristic_collect.hip) share:
// the rollout loops' view of _generate_legal() and their step key, the policy tables, a fresh episode's side statistics and
// History, what a CHECK adds to the two history sums, the all-null belief, and the host side's argument checks and planning
// front end (plan_with).  The CHECK's likelihood update itself is RockEnv::check_update (envs/rock.hip.h).
#pragma once
#include "kernels_common.hip.h"

namespace pomdp {

// envs whose _generate_preferred is a policy of its own (RockSample's heuristic, Tag); for the others it is the legal list
template <class Env> struct has_policy : std::integral_constant<bool, Env::HAS_ROCKS || std::is_same<Env, TagEnv>::value> {};

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

// the key of call counter t: key0 with its counter words replaced
static __device__ __forceinline__ RngKey key_at(RngKey key, uint64_t t) { key.t_lo = (uint32_t)t; key.t_hi = (uint32_t)(t >> 32); return key; }

// the number of rocks an env's params describe; 0 for the envs without rocks
static __host__ __device__ __forceinline__ int rock_count(const pomdp_rock_params &p) { return p.num_rocks; }
template <class P> static __host__ __device__ __forceinline__ int rock_count(const P &) { return 0; }

// a new episode's side statistics: a fresh Rock object (rock.py:81-86) in entry k = j * n + i of every per-rock array.  A
// fresh rock passes the test of rock.py:371: its bit of check_ok is set.  (The loop over the rocks stays with the caller:
// inside an inlined helper it changes the order of the blocks belief_reset_kernel compiles to.)
static __device__ __forceinline__ void belief_fresh_rock(const pomdp_rock_belief &b, int64_t k)
{
    b.count[k] = 0; b.measured[k] = 0; b.lkv[k] = 1.; b.lkw[k] = 1.; b.prob_valuable[k] = .5;
}
// a new, empty History: no record, both sums of every rock 0 (so total_move >= 0 holds for all of them)
static __device__ __forceinline__ void history_fresh_rock(const pomdp_history &h, int64_t k)
{
    h.total_sample[k] = 0; h.total_move[k] = 0;
}
static __device__ __forceinline__ void history_fresh(const pomdp_history &h, int K, int64_t n, int64_t i)
{
    h.size[i] = 0; h.last_action[i] = -1; h.last_ob[i] = -1;
    for (int j = 0; j < K; ++j) history_fresh_rock(h, (int64_t)j * n + i);
    if (K) h.move_ok[i] = (1u << K) - 1u;
    if (h.head) h.head[i] = 0;
}

// the two sums over CHECK-j transitions (rock.py:303-310, 327-334): what one transition (action CHECK j, next observation,
// observation before it BAD or not) contributes to total_sample[j] (ds) and total_move[j] (dm) when it is added (sign = 1) or,
// when a bounded history drops it, taken out again (sign = -1).  The caller adds a non-zero contribution to the sum, wherever
// it keeps it, and sets the derived bit of its copy of move_ok from the new sum — bit 16 + j: total_sample[j] > 0
// (rock.py:311), bit j: total_move[j] >= 0 (rock.py:335).  (The two `if`s stay with the callers: inside an inlined helper
// they change the text rollout_preferred_kernel compiles to.)
static __device__ __forceinline__ int check_ds(int next_ob, int sign = 1) { return sign * ((next_ob == 2) - (next_ob == 1)); }
static __device__ __forceinline__ int check_dm(int next_ob, bool prev_bad, int sign = 1)
{
    return sign * (next_ob == 2 ? 1 : (prev_bad ? -1 : 0));
}
static __device__ __forceinline__ uint32_t with_bit(uint32_t word, uint32_t bit, bool on) { return on ? (word | bit) : (word & ~bit); }

static const pomdp_rock_belief NO_BELIEF = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // an env without rocks

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

// a planning step (pomdp_plan, pomdp_plan_preferred): everything is checked before anything is enqueued, then rollout()
// fills sim_ret / sim_first_action and pomdp_plan_reduce turns them into `out`
template <class Rollout>
static inline int plan_with(int env, const void *params, int64_t n_roots, int64_t sims_per_root, double *sim_ret,
                            int32_t *sim_first_action, const pomdp_plan_out *out, void *stream, Rollout rollout)
{
    if (!params || !out) return POMDP_E_BADARG;
    int rc = dispatch_env(env, params, [](auto, const auto &) { return 0; });   // POMDP_E_BADPARAMS / unknown env
    if (rc) return rc;
    const int n_act = (int)env_action_count(env, params);
    if (n_roots > 0x7FFFFFFF || !plan_out_ok(out, n_act)) return POMDP_E_BADARG;
    rc = rollout();
    if (rc) return rc;
    return pomdp_plan_reduce(sim_ret, sim_first_action, n_roots, sims_per_root, n_act, out, stream);
}
