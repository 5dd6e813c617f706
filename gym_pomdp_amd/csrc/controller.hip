// controller.hip — closed-loop policies inside the frozen-lane fused loop (pomdp_controller_episodes): a finite-state
// controller — an action per node, a successor node per (node, observation) — staged into LDS once per workgroup, a lane's node
// in a register next to its state.  The loop is episodes.hip's general one (one lane per thread, any n, every env) with the
// policy's action read from LDS at the lane's node and the node advanced on the step's own observation; same draws, same
// sinks (Packed, Narrow, EpisodeReturns).
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "controller_common.hip.h"
#include <cstring>

namespace pomdp {

struct ControllerRef {
    const int32_t *action, *next;
    int32_t *node;
    uint32_t n_nodes, n_obs;
    uint32_t *err;           // device counter of refused entries met by live lanes (may be nullptr)
};

// the launch's dynamic LDS: a halfword per successor and a byte per node — what the controller needs, not what the largest
// would (36 KB, four workgroups per CU: a 128-node controller leaves the CU to the registers' eight waves per SIMD)
static inline unsigned ctrl_lds_bytes(const ControllerRef &c) { return (2u * c.n_nodes * c.n_obs + c.n_nodes + 15u) & ~15u; }

// k_steps consecutive pomdp_<env>_step(flags = 0) calls at t0 + s, lane i taking action[node_i] and then moving to
// next[node_i][ob].  `done` and `node` are read when the launch starts and written when it ends.  Every lane of a wave runs
// the env's lane step (it may hold wave-cooperative draws); a frozen lane's result is discarded.  A wave whose lanes are all
// frozen skips the lane step (record sinks: only the constant rows are left to store) or leaves the loop (returns sink).
// A lane whose incoming node is outside [0, n_nodes) never reads the tables: its action byte is CTRL_NO_ACTION on every step.
// The tables are read from global memory BEFORE the loop only (fused_impl.hip.h: a loop that holds a load waits for the
// previous step's stores in every iteration); the loop reads one LDS byte and one LDS halfword per step.
// out0, out1, rec, discount_bits: as episodes_kernel.
template <class Env, class L>
__global__ __launch_bounds__(BLOCK) void controller_kernel(uint32_t *__restrict__ state, uint8_t *__restrict__ done,
                                                           void *__restrict__ out0, void *__restrict__ out1, uint64_t discount_bits,
                                                           int64_t n, RngKey key0, uint32_t lane0, int k_steps, int64_t rec,
                                                           const typename Env::Params p, ControllerRef c)
{
    constexpr bool RETS = L::ID == LAYOUT_RETURNS;
    __shared__ typename Env::Shared sh;
    extern __shared__ __align__(16) uint8_t ctrl_lds[];                         // ctrl_lds_bytes(): the successors, then the actions
    uint16_t *const nxt = reinterpret_cast<uint16_t *>(ctrl_lds);
    uint8_t *const act = ctrl_lds + 2u * (c.n_nodes * c.n_obs);
    const uint32_t wg0 = blockIdx.x * (uint32_t)BLOCK;
    const uint32_t last = (uint32_t)((uint64_t)(n - 1) - wg0);
    const uint32_t rel = threadIdx.x;
    const bool in_range = rel <= last;
    const uint32_t rc = in_range ? rel : last;                                  // threads past n read lane n - 1
    __builtin_assume(rc < (uint32_t)BLOCK);
    const uint32_t glane = lane0 + wg0 + rel;
    uint32_t *const state_w = state + wg0;
    typename Env::State st;
    Env::load(st, state_w, n, rc);
    bool frozen = !in_range || ld_stream(done + wg0 + rc) != 0;
    const uint32_t q_in = (uint32_t)ld_stream(c.node + wg0 + rc);
    using Out = typename std::conditional<RETS, EpisodeReturns<Env, 1>, LaneOut<L, typename Env::Reward, 1>>::type;
    Out out = [&]() {
        if constexpr (RETS) return Out(reinterpret_cast<double *>(out0) + wg0, reinterpret_cast<uint32_t *>(out1) + wg0, discount_bits, rec);
        else return Out(out0, nullptr, nullptr, nullptr, rec, wg0);
    }();
    if constexpr (RETS) out.begin(0, rc);
    // the tables, narrowed on the way in (the host keeps n_nodes and n_nodes * n_obs within the arrays)
    const uint32_t n_nodes = c.n_nodes, n_obs = c.n_obs;
    stage_narrow<CTRL_MAX_NODES / BLOCK>(act, c.action, n_nodes, [](uint32_t a) { return a < CTRL_NO_ACTION ? a : CTRL_NO_ACTION; });
    stage_narrow<CTRL_MAX_EDGES / BLOCK>(nxt, c.next, n_nodes * n_obs, [=](uint32_t v) { return v < n_nodes ? v : CTRL_NO_NODE; });
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const bool q_ok = q_in < n_nodes;
    uint32_t q = q_ok ? q_in : 0u;
    const uint32_t n_act = (uint32_t)Env::n_actions(p);
    const uint64_t t0 = ((uint64_t)key0.t_hi << 32) | key0.t_lo;
    uint32_t n_bad = 0;
    const LoopPrio prio(k_steps);
    wait_loads();
#pragma unroll 1
    for (int seg = 0, s = 0; seg < 4; ++seg)                                    // four priority segments (LoopPrio)
    for (const int seg_end = prio.segment(seg); s < seg_end; ++s) {
        if constexpr (RETS) {
            if (__ballot(!frozen) == 0) { s = k_steps; break; }                 // wave-uniform: nothing left to add up
        }
        RngKey key = key0;
        key.t_lo = (uint32_t)(t0 + (uint64_t)s); key.t_hi = (uint32_t)((t0 + (uint64_t)s) >> 32);
        const uint32_t a = q_ok ? (uint32_t)act[q] : CTRL_NO_ACTION;
        uint32_t record = a | (1u << 24);                                       // a frozen lane's row: (ob, reward, done) = (0, 0, 1)
        const bool live = !frozen;
        if (__ballot(live) != 0) {                                              // wave-uniform
            const bool valid = a < n_act;
            typename Env::State nx = st;
            int o, d;
            typename Env::Reward r;
            Env::step(sh, p, nx, valid ? (int)a : 0, key, glane, o, r, d);
            if (live) {
                if (valid) {
                    st = nx;
                    record = pack_record(a, (uint32_t)o & 0xFFu, Env::reward_code(r), (uint32_t)(d != 0));
                    frozen = d != 0;
                    // an observation the table has no column for (Tag built with obs_cells < 28) finds no successor
                    const uint32_t to = (uint32_t)o < n_obs ? (uint32_t)nxt[q * n_obs + (uint32_t)o] : CTRL_NO_NODE;
                    if (to != CTRL_NO_NODE) q = to;
                    else ++n_bad;                                               // the step stands, the node stays, counted
                } else {
                    record = a;                                                 // a refused action: untouched, (0, 0, 0), counted
                    ++n_bad;
                }
            }
        }
        if constexpr (RETS) out.put(0, record, live);
        else if (in_range) out.put_record(0, rel, record);
        if constexpr (!RETS) out.next_row();
    }
    if (in_range) {
        Env::store(st, state_w, n, rel, false);
        done[wg0 + rel] = frozen ? 1 : 0;
        if (q_ok) c.node[wg0 + rel] = (int32_t)q;
        if constexpr (RETS) out.finish(0, rel);
    }
    if (n_bad && c.err) atomicAdd(c.err, n_bad);
}

// one launch of up to pomdp_fuse_max() steps
template <class Env, class L>
static int launch_controller(const typename Env::Params &p, uint32_t *state, uint8_t *done, void *out0, void *out1, uint64_t dbits,
                             int64_t n, uint64_t seed, uint32_t lane0, uint64_t t, int k, int64_t rec, const ControllerRef &c,
                             void *stream)
{
    char lname[32];
    snprintf(lname, sizeof lname, ", %s", L::NAME);
    note_fused("controller_kernel", Env::NAME, lname);
    hipLaunchKernelGGL((controller_kernel<Env, L>), dim3(blocks_for(n)), dim3(BLOCK), ctrl_lds_bytes(c), (hipStream_t)stream, state, done, out0, out1,
                       dbits, n, make_key(seed, t), lane0, k, rec, p, c);
    return (int)hipGetLastError();
}

} // namespace pomdp

extern "C" {

int pomdp_controller_episodes(const pomdp_episode_args *a, const pomdp_controller *c, uint64_t t0, int64_t k_steps, void *stream)
{
    if (!c || !c->action || !c->next || !c->node) return POMDP_E_BADARG;
    if (c->n_nodes < 1 || c->n_nodes > (int32_t)CTRL_MAX_NODES || c->n_obs < 1 ||
        (int64_t)c->n_nodes * c->n_obs > (int64_t)CTRL_MAX_EDGES)
        return POMDP_E_BADARG;
    int rc = controller_episode_args_check(a, k_steps);
    if (rc) return rc;
    const int64_t n = a->n;
    const bool rets = a->layout == POMDP_LAYOUT_RETURNS;
    if ((int64_t)c->n_obs != env_obs_count(a->env, a->params)) return POMDP_E_BADARG;
    if (k_steps == 0 || n == 0) return 0;
    uint64_t dbits = 0;
    if (rets) memcpy(&dbits, &a->stats->discount, 8);
    const ControllerRef ref = {c->action, c->next, c->node, (uint32_t)c->n_nodes, (uint32_t)c->n_obs, a->err};
    const int64_t row_bytes = 4 * a->pitch;                            // Packed: pitch records; Narrow: four planes of pitch bytes
    const int64_t FUSE_MAX = fuse_max();
    for (int64_t s = 0; s < k_steps; s += FUSE_MAX) {
        const int k = (int)(k_steps - s < FUSE_MAX ? k_steps - s : FUSE_MAX);
        rc = dispatch_env(a->env, a->params, [&](auto tag, const auto &p) {
            using E = typename decltype(tag)::Env;
            const uint64_t t = t0 + (uint64_t)s;
            if (rets)
                return launch_controller<E, Returns<E>>(p, a->state, a->done, a->stats->acc, a->stats->cnt, dbits, n, a->seed, a->lane0, t,
                                                        k, a->stats->pitch, ref, stream);
            void *base = reinterpret_cast<uint8_t *>(a->traj) + s * row_bytes;
            if (a->layout == POMDP_LAYOUT_PACKED)
                return launch_controller<E, Packed>(p, a->state, a->done, base, nullptr, 0, n, a->seed, a->lane0, t, k, a->pitch, ref, stream);
            return launch_controller<E, Narrow>(p, a->state, a->done, base, nullptr, 0, n, a->seed, a->lane0, t, k, a->pitch, ref, stream);
        });
        if (rc) return rc;
    }
    return 0;
}

} // extern "C"
