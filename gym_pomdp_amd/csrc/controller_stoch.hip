// controller_stoch.hip — stochastic finite-state controllers inside the frozen-lane fused loop (pomdp_stoch_controller_episodes):
// node q DRAWS its action among B candidates and its successor among D candidates per observation, per lane and per step, from
// the lane's own Philox block of stream CONTROLLER (word 0 the action draw, word 1 the successor draw).  A pick is a count: the
// number of the row's thresholds the draw exceeds — integer compares against LDS words, any threshold values.  The loop is
// controller.hip's (one lane per thread, any n, every env; same env draws, same sinks, same priority ladder) with the block and
// the two counted picks added; the tables live in the launch's dynamic LDS, sized by need.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "controller_common.hip.h"
#include <cstring>

namespace pomdp {

// What one launch may stage, in rows of BLOCK entries (stage_narrow is straight code: its size is fixed here).  With the
// footprint F = K B + 4 K (B - 1) + 2 K O D + 4 K O (D - 1) <= 36864, K <= 4096 and B, D, O >= 1:
//   candidate actions     K B       <= (F + 2 K) / 5 <= 9011    (F >= 5 K B - 4 K + 2 K O)
//   action thresholds     K (B - 1) <= F / 5         <= 7372
//   candidate successors  K O D     <= (F - 1) / 2   <= 18431
//   successor thresholds  K O (D-1) <= (F - 3) / 6   <= 6143    (F >= K + 6 K O (D - 1) + 2 K O)
// The host refuses what does not fit (it cannot happen within the footprint; the check keeps the kernel's bound in sight).
constexpr int STOCH_ACT_ROWS = 40, STOCH_ATHR_ROWS = 32, STOCH_NEXT_ROWS = 72, STOCH_NTHR_ROWS = 24;
constexpr int64_t STOCH_MAX_BYTES = POMDP_STOCH_CONTROLLER_MAX_BYTES;

struct StochControllerRef {
    const int32_t *action, *next;
    const uint32_t *action_thr, *next_thr;
    int32_t *node;
    uint32_t n_nodes, n_obs, n_act_cand, n_next_cand;
    uint32_t *err;           // device counter of refused entries met by live lanes (may be nullptr)
};

// the table footprint of the header: thresholds as words, successors as halfwords, actions as bytes
static inline int64_t stoch_lds_bytes(int64_t K, int64_t O, int64_t B, int64_t D)
{
    return (K * B + 4 * K * (B - 1) + 2 * K * O * D + 4 * K * O * (D - 1) + 15) & ~(int64_t)15;
}

// controller_kernel's loop with the action and the successor drawn: per step every lane computes block 0 of stream CONTROLLER
// at (seed, its global lane, t0 + s) — counter words 0 and 3 fixed for the launch, 1 and 2 wave-uniform: philox4x32_10_fixed,
// round 3's launch-fixed product hoisted per stretch of one counter high word — and counts the thresholds of its node's row
// that word 0 exceeds; after the env's step it counts those of the (node, observation) row that word 1 exceeds.  The candidate
// loops are run-time loops over LDS with launch-uniform trip counts (B - 1, D - 1): nothing is indexed in registers.  A frozen
// lane still draws its action (its record carries the byte); a lane on no node reads row 0 and discards it.
// All tables are read from global memory BEFORE the loop only; out0, out1, rec, discount_bits: as episodes_kernel.
template <class Env, class L>
__global__ __launch_bounds__(BLOCK) void stoch_controller_kernel(uint32_t *__restrict__ state, uint8_t *__restrict__ done,
                                                                 void *__restrict__ out0, void *__restrict__ out1, uint64_t discount_bits,
                                                                 int64_t n, RngKey key0, uint32_t lane0, int k_steps, int64_t rec,
                                                                 const typename Env::Params p, StochControllerRef c)
{
    constexpr bool RETS = L::ID == LAYOUT_RETURNS;
    __shared__ typename Env::Shared sh;
    // stoch_lds_bytes(): the action thresholds, the successor thresholds, the successors, the actions (widest entries first)
    extern __shared__ __align__(16) uint8_t stoch_lds[];
    const uint32_t n_nodes = c.n_nodes, n_obs = c.n_obs, n_b = c.n_act_cand, n_d = c.n_next_cand;
    const uint32_t n_bt = n_b - 1u, n_dt = n_d - 1u;                            // thresholds per row
    const uint32_t rows = n_nodes * n_obs;
    uint32_t *const athr = reinterpret_cast<uint32_t *>(stoch_lds);
    uint32_t *const nthr = athr + n_nodes * n_bt;
    uint16_t *const nxt = reinterpret_cast<uint16_t *>(nthr + rows * n_dt);
    uint8_t *const act = reinterpret_cast<uint8_t *>(nxt + rows * n_d);
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
    // the tables, narrowed on the way in (the host keeps every count within its rows; a table of no entries is never read)
    stage_narrow<STOCH_ATHR_ROWS>(athr, reinterpret_cast<const int32_t *>(c.action_thr), n_nodes * n_bt, [](uint32_t v) { return v; });
    stage_narrow<STOCH_NTHR_ROWS>(nthr, reinterpret_cast<const int32_t *>(c.next_thr), rows * n_dt, [](uint32_t v) { return v; });
    stage_narrow<STOCH_NEXT_ROWS>(nxt, c.next, rows * n_d, [=](uint32_t v) { return v < n_nodes ? v : CTRL_NO_NODE; });
    stage_narrow<STOCH_ACT_ROWS>(act, c.action, n_nodes * n_b, [](uint32_t a) { return a < CTRL_NO_ACTION ? a : CTRL_NO_ACTION; });
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const bool q_ok = q_in < n_nodes;
    uint32_t q = q_ok ? q_in : 0u;
    const uint32_t n_act = (uint32_t)Env::n_actions(p);
    const uint64_t t0 = ((uint64_t)key0.t_hi << 32) | key0.t_lo;
    PhiloxFixed fx = philox_fixed(glane, (uint32_t)POMDP_STREAM_CONTROLLER << 24, key0.k1);
    uint32_t n_bad = 0;
    const LoopPrio prio(k_steps);
    wait_loads();
#pragma unroll 1
    for (int seg = 0, s = 0; seg < 4; ++seg) {                                  // four priority segments (LoopPrio)
        const int seg_end = prio.segment(seg);
#pragma unroll 1
        while (s < seg_end) {                                                   // stretches of one counter high word (philox_hoist)
            const uint64_t ts = t0 + (uint64_t)s;
            philox_hoist(fx, (uint32_t)(ts >> 32), key0.k0);
            const int end = stretch_end(s, seg_end, (uint32_t)ts);
#pragma unroll 1
            for (; s < end; ++s) {
                if constexpr (RETS) {
                    if (__ballot(!frozen) == 0) { s = k_steps; break; }         // wave-uniform: nothing left to add up
                }
                RngKey key = key0;
                key.t_lo = (uint32_t)(t0 + (uint64_t)s); key.t_hi = (uint32_t)((t0 + (uint64_t)s) >> 32);
                const uint4 u = philox4x32_10_fixed(fx, key.t_lo, key.t_hi, key.k0, key.k1);
                uint32_t ia = 0;                                                // the action pick: thresholds of row q passed by u.x
                {
                    const uint32_t *const row = athr + q * n_bt;
                    for (uint32_t j = 0; j < n_bt; ++j) ia += u.x > row[j] ? 1u : 0u;
                }
                const uint32_t a = q_ok ? (uint32_t)act[q * n_b + ia] : CTRL_NO_ACTION;
                uint32_t record = a | (1u << 24);                               // a frozen lane's row: (ob, reward, done) = (0, 0, 1)
                const bool live = !frozen;
                if (__ballot(live) != 0) {                                      // wave-uniform
                    const bool valid = a < n_act;
                    typename Env::State nx = st;
                    int o, d;
                    typename Env::Reward r;
                    Env::step(sh, p, nx, valid ? (int)a : 0, key, glane, o, r, d);
                    // the successor pick, by every lane of the wave on a row that exists: an observation the table has no column
                    // for (Tag built with obs_cells < 28) reads column 0 and finds no successor
                    const bool column = (uint32_t)o < n_obs;
                    const uint32_t e = q * n_obs + (column ? (uint32_t)o : 0u);
                    uint32_t in = 0;
                    {
                        const uint32_t *const row = nthr + e * n_dt;
                        for (uint32_t j = 0; j < n_dt; ++j) in += u.y > row[j] ? 1u : 0u;
                    }
                    const uint32_t to = column ? (uint32_t)nxt[e * n_d + in] : CTRL_NO_NODE;
                    if (live) {
                        if (valid) {
                            st = nx;
                            record = pack_record(a, (uint32_t)o & 0xFFu, Env::reward_code(r), (uint32_t)(d != 0));
                            frozen = d != 0;
                            if (to != CTRL_NO_NODE) q = to;
                            else ++n_bad;                                       // the step stands, the node stays, counted
                        } else {
                            record = a;                                         // a refused action: untouched, (0, 0, 0), counted
                            ++n_bad;
                        }
                    }
                }
                if constexpr (RETS) out.put(0, record, live);
                else if (in_range) out.put_record(0, rel, record);
                if constexpr (!RETS) out.next_row();
            }
        }
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
static int launch_stoch_controller(const typename Env::Params &p, uint32_t *state, uint8_t *done, void *out0, void *out1, uint64_t dbits,
                                   int64_t n, uint64_t seed, uint32_t lane0, uint64_t t, int k, int64_t rec, const StochControllerRef &c,
                                   void *stream)
{
    char lname[32];
    snprintf(lname, sizeof lname, ", %s", L::NAME);
    note_fused("stoch_controller_kernel", Env::NAME, lname);
    const unsigned lds = (unsigned)stoch_lds_bytes(c.n_nodes, c.n_obs, c.n_act_cand, c.n_next_cand);
    hipLaunchKernelGGL((stoch_controller_kernel<Env, L>), dim3(blocks_for(n)), dim3(BLOCK), lds, (hipStream_t)stream, state, done, out0,
                       out1, dbits, n, make_key(seed, t), lane0, k, rec, p, c);
    return (int)hipGetLastError();
}

} // namespace pomdp

extern "C" {

int pomdp_stoch_controller_episodes(const pomdp_episode_args *a, const pomdp_stoch_controller *c, uint64_t t0, int64_t k_steps,
                                    void *stream)
{
    if (!c || !c->action || !c->next || !c->node) return POMDP_E_BADARG;
    if (c->n_nodes < 1 || c->n_nodes > (int32_t)CTRL_MAX_NODES || c->n_obs < 1) return POMDP_E_BADARG;
    // a count past the footprint on its own is refused before the products below are formed
    if (c->n_act_cand < 1 || c->n_act_cand > STOCH_MAX_BYTES || c->n_next_cand < 1 || c->n_next_cand > STOCH_MAX_BYTES)
        return POMDP_E_BADARG;
    if ((c->n_act_cand > 1 && !c->action_thr) || (c->n_next_cand > 1 && !c->next_thr)) return POMDP_E_BADARG;
    const int64_t K = c->n_nodes, O = c->n_obs, B = c->n_act_cand, D = c->n_next_cand;
    if (stoch_lds_bytes(K, O, B, D) > STOCH_MAX_BYTES) return POMDP_E_BADARG;
    if (K * B > STOCH_ACT_ROWS * BLOCK || K * (B - 1) > STOCH_ATHR_ROWS * BLOCK || K * O * D > STOCH_NEXT_ROWS * BLOCK ||
        K * O * (D - 1) > STOCH_NTHR_ROWS * BLOCK)
        return POMDP_E_BADARG;
    int rc = controller_episode_args_check(a, k_steps);
    if (rc) return rc;
    const int64_t n = a->n;
    const bool rets = a->layout == POMDP_LAYOUT_RETURNS;
    if (O != env_obs_count(a->env, a->params)) return POMDP_E_BADARG;
    if (k_steps == 0 || n == 0) return 0;
    uint64_t dbits = 0;
    if (rets) memcpy(&dbits, &a->stats->discount, 8);
    const StochControllerRef ref = {c->action, c->next, c->action_thr, c->next_thr, c->node, (uint32_t)K, (uint32_t)O, (uint32_t)B,
                                    (uint32_t)D, a->err};
    const int64_t row_bytes = 4 * a->pitch;                            // Packed: pitch records; Narrow: four planes of pitch bytes
    const int64_t FUSE_MAX = fuse_max();
    for (int64_t s = 0; s < k_steps; s += FUSE_MAX) {
        const int k = (int)(k_steps - s < FUSE_MAX ? k_steps - s : FUSE_MAX);
        rc = dispatch_env(a->env, a->params, [&](auto tag, const auto &p) {
            using E = typename decltype(tag)::Env;
            const uint64_t t = t0 + (uint64_t)s;
            if (rets)
                return launch_stoch_controller<E, Returns<E>>(p, a->state, a->done, a->stats->acc, a->stats->cnt, dbits, n, a->seed,
                                                              a->lane0, t, k, a->stats->pitch, ref, stream);
            void *base = reinterpret_cast<uint8_t *>(a->traj) + s * row_bytes;
            if (a->layout == POMDP_LAYOUT_PACKED)
                return launch_stoch_controller<E, Packed>(p, a->state, a->done, base, nullptr, 0, n, a->seed, a->lane0, t, k, a->pitch,
                                                          ref, stream);
            return launch_stoch_controller<E, Narrow>(p, a->state, a->done, base, nullptr, 0, n, a->seed, a->lane0, t, k, a->pitch, ref,
                                                      stream);
        });
        if (rc) return rc;
    }
    return 0;
}

} // extern "C"
