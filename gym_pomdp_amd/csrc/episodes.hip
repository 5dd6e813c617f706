// episodes.hip — episodes played to their end (ABI 15): the masked reset (pomdp_reset_where) and the frozen-lane fused loops
// (pomdp_finish_episodes).  Without auto-reset a lane whose episode ended does not step again: it keeps its state and every
// later step of the call reports (ob, reward, done) = (0, 0, 1) for it, as pomdp_<env>_step(flags = 0) does.  Only the
// 4-byte sinks (Packed, Narrow) and a returns sink that books live steps only.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "kernels_common.hip.h"
#include <cstring>

namespace pomdp {

// ---- masked reset -----------------------------------------------------------------------------------------------------------
// A lane with where[i] != 0 starts exactly the episode reset_kernel deals it at the same (seed, lane, t) — Env::reset per lane,
// RockSample's quad-shared RESET block and BattleShip's RESET / NEXT boards included — and has its done flag cleared; every
// other lane keeps its state and done flag and reports ob = -1 (no env observes -1).  where == nullptr: every lane.
template <class Env>
__global__ __launch_bounds__(BLOCK) void reset_where_kernel(const typename Env::Params p, uint32_t *__restrict__ state,
                                                            int32_t *__restrict__ ob, uint8_t *__restrict__ done,
                                                            const uint8_t *__restrict__ where, int64_t n, RngKey key, uint32_t lane0)
{
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const bool fresh = !where || where[i] != 0;
    int o = -1;
    if (fresh) {
        typename Env::State st;
        o = Env::reset(sh, p, st, key, lane0 + (uint32_t)i);
        Env::store(st, state, n, (uint32_t)i, true);
        if (done) done[i] = 0;
    }
    if (ob) ob[i] = o;
}

// the returns sink of these loops: EpisodeReturns (traj_out.hip.h), shared with controller.hip

// ---- the general frozen-lane loop: one lane per thread, any n, every env ----------------------------------------------------
// k_steps consecutive pomdp_<env>_step(flags = 0) calls at t0 + s with the synthetic policy's actions of t0 + s (TAPE: row s of
// the caller's tape), the lane's state in registers between its steps.  `done` is read when the launch starts and written when
// it ends.  Every lane of a wave runs the env's lane step (it may hold wave-cooperative draws); a frozen lane's result is
// discarded.  A wave whose lanes are all frozen skips the lane step (record sinks: only the constant rows are left to store,
// with the policy's action in them) or leaves the loop (returns sink).
// out0: the trajectory's base (Packed, Narrow) or the statistics' double rows (Returns); out1: their int32 rows; rec: the row
// pitch in lanes; discount_bits: the returns sink's discount as its bit pattern.
template <class Env, class L, bool TAPE>
__global__ __launch_bounds__(BLOCK) void episodes_kernel(uint32_t *__restrict__ state, uint8_t *__restrict__ done,
                                                         void *__restrict__ out0, void *__restrict__ out1, uint64_t discount_bits,
                                                         int64_t n, RngKey key0, uint32_t lane0, int k_steps, int64_t rec,
                                                         const typename Env::Params p, TapeRef tape)
{
    constexpr bool RETS = L::ID == LAYOUT_RETURNS;
    __shared__ typename Env::Shared sh;
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
    using Out = typename std::conditional<RETS, EpisodeReturns<Env, 1>, LaneOut<L, typename Env::Reward, 1>>::type;
    Out out = [&]() {
        if constexpr (RETS) return Out(reinterpret_cast<double *>(out0) + wg0, reinterpret_cast<uint32_t *>(out1) + wg0, discount_bits, rec);
        else return Out(out0, nullptr, nullptr, nullptr, rec, wg0);
    }();
    if constexpr (RETS) out.begin(0, rc);
    typename std::conditional<TAPE, TapeColumn<uint8_t>, NoColumn>::type col(tape, wg0 + rc, k_steps);
    uint32_t a_tape = col.first;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
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
        if constexpr (TAPE) col.request(s);                                     // the row of step s + 1
        RngKey key = key0;
        key.t_lo = (uint32_t)(t0 + (uint64_t)s); key.t_hi = (uint32_t)((t0 + (uint64_t)s) >> 32);
        const uint32_t a = TAPE ? a_tape : (uint32_t)synthetic_action(key, glane, n_act);
        uint32_t record = (a & 0xFFu) | (1u << 24);                             // a frozen lane's row: (ob, reward, done) = (0, 0, 1)
        const bool live = !frozen;
        if (__ballot(live) != 0) {                                              // wave-uniform
            const bool valid = !TAPE || a < n_act;
            typename Env::State nx = st;
            int o, d;
            typename Env::Reward r;
            Env::step(sh, p, nx, valid ? (int)a : 0, key, glane, o, r, d);
            if (live) {
                if (valid) {
                    st = nx;
                    record = pack_record(a, (uint32_t)o & 0xFFu, Env::reward_code(r), (uint32_t)(d != 0));
                    frozen = d != 0;
                } else {
                    record = a & 0xFFu;                                         // an out-of-range byte: untouched, (0, 0, 0), counted
                    ++n_bad;
                }
            }
        }
        if constexpr (RETS) out.put(0, record, live);
        else if (in_range) out.put_record(0, rel, record);
        if constexpr (!RETS) out.next_row();
        if constexpr (TAPE) a_tape = col.nxt;
    }
    if (in_range) {
        Env::store(st, state_w, n, rel, false);
        done[wg0 + rel] = frozen ? 1 : 0;
        if constexpr (RETS) out.finish(0, rel);
    }
    if (TAPE && n_bad && tape.err) atomicAdd(tape.err, n_bad);
}

// ---- RockSample / StochasticRock, a quad of consecutive lanes per thread ----------------------------------------------------
// The frozen-lane form of steps_quad_kernel: the quad's sensor block (StochasticRock: and its gate block) and its policy block
// are the thread's own, the lane step is the table-driven step_rec.  A step that ends a RockSample episode — leaving the board,
// or sampling where there is nothing to sample (rock.py:139-141, 160-169) — changes nothing in the state, so the state the
// reference's frozen step() leaves is the one the step started from: it goes in where step_rec takes the fresh episode, and no
// reset words are drawn at all.  The thread's four done flags travel as one word, its outputs as 16-byte stores (Packed,
// Narrow) or in registers (Returns: read and written once, 16 bytes at a time).  Full workgroups of 1024 lanes, 16-byte-aligned
// state and statistics.
template <class Env, class L, class Pol>
__global__ __launch_bounds__(BLOCK) void episodes_quad_kernel(uint32_t *__restrict__ state, uint8_t *__restrict__ done,
                                                              void *__restrict__ out0, void *__restrict__ out1, uint64_t discount_bits,
                                                              int64_t n, RngKey key0, uint32_t lane0, int k_steps, int64_t rec,
                                                              const typename Env::Params p, TapeRef tape)
{
    constexpr bool RETS = L::ID == LAYOUT_RETURNS;
    constexpr int W = Env::WORDS;
    using S = typename Env::S;
    __shared__ typename Env::Shared sh;
    __shared__ typename Env::RecTab tab;
    const uint32_t n_act = (uint32_t)Env::n_actions(p);
    const uint32_t l0 = blockIdx.x * (uint32_t)(4 * BLOCK) + 4u * threadIdx.x, glane0 = lane0 + l0;
    // the policy of step s is that of call counter t0 + s: SyntheticQuad::begin(s) with akey0 = key0 (its block's round-3
    // product stays in the step: this loop does not run as stretches)
    typename lanes_policy<Pol, 4, false>::type pol(tape, l0, glane0, key0, key0, n_act, k_steps);
    using Out = typename std::conditional<RETS, EpisodeReturns<Env, 4>, QuadOut<L>>::type;
    Out out = [&]() {
        if constexpr (RETS) return Out(reinterpret_cast<double *>(out0), reinterpret_cast<uint32_t *>(out1), discount_bits, rec);
        else return Out(out0, nullptr, nullptr, nullptr, rec, l0);
    }();
    typename Env::State st[4];
    bool frozen[4];
    uint32_t a_cur[4] = {0, 0, 0, 0};
    {
        const u32x4 lo = ld_stream4(state + l0);
        u32x4 hi = {0, 0, 0, 0};
        if (W == 2) hi = ld_stream4(state + n + l0);
        const uint32_t dn = ld_stream(reinterpret_cast<const uint32_t *>(done + l0));
        if constexpr (Pol::TAPE) {
            const u32x4 f = pol.first();
#pragma unroll
            for (int j = 0; j < 4; ++j) a_cur[j] = f[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st[j].s = (S)((uint64_t)lo[j] | ((uint64_t)hi[j] << 32));
            frozen[j] = ((dn >> (8 * j)) & 0xFFu) != 0u;
        }
        if constexpr (RETS) out.begin4(l0);
    }
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    Env::build_rec_tab(tab, sh, p, (int)threadIdx.x);
    __syncthreads();
    const uint64_t t0 = ((uint64_t)key0.t_hi << 32) | key0.t_lo;
    uint32_t n_bad = 0;
    const LoopPrio prio(k_steps);
    wait_loads();
#pragma unroll 1
    for (int seg = 0, s = 0; seg < 4; ++seg)                                    // four priority segments (LoopPrio)
    for (const int seg_end = prio.segment(seg); s < seg_end; ++s) {
        const bool any_live = !(frozen[0] && frozen[1] && frozen[2] && frozen[3]);
        if constexpr (RETS) {
            if (__ballot(any_live) == 0) { s = k_steps; break; }                // wave-uniform: nothing left to add up
        }
        RngKey key = key0;
        key.t_lo = (uint32_t)(t0 + (uint64_t)s); key.t_hi = (uint32_t)((t0 + (uint64_t)s) >> 32);
        uint32_t a_nx[4];
        pol.begin(s, a_nx);                                                     // Synthetic: the actions of step s; Tape: asks for row s + 1
        if constexpr (!Pol::TAPE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a_cur[j] = a_nx[j];
        }
        uint32_t recs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) recs[j] = a_cur[j] | (1u << 24);            // a frozen lane's row: (ob, reward, done) = (0, 0, 1)
        if (__ballot(any_live) != 0) {                                          // wave-uniform: the quad's blocks and the lane steps
            constexpr uint32_t SENSOR_BLOCK = Env::SENSOR_BLOCK;
            const uint4 sw = philox4x32_10(glane0 >> 2, key.t_lo, key.t_hi, ((uint32_t)POMDP_STREAM_STEP << 24) | SENSOR_BLOCK, key.k0, key.k1);
            const uint32_t H[4] = {sw.x, sw.y, sw.z, sw.w};
            bool acts[4] = {true, true, true, true};
            if constexpr (Env::STOCHASTIC) {                                    // the action is applied iff binomial(1, p_move) says so
                const uint4 gw = Env::quad_block(key, glane0, 0u);
                const uint32_t G[4] = {gw.x, gw.y, gw.z, gw.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acts[j] = Env::k53_le(G[j], (uint32_t)(p.act_thr >> 26), (uint32_t)p.act_thr & Env::LO_MASK,
                                          [&]() { return Env::elem(Env::quad_block(key, glane0, 1u), (uint32_t)j); }) != (p.act_gt != 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t lane = glane0 + (uint32_t)j;
                const bool valid = !Pol::TAPE || a_cur[j] < n_act;
                S sj = st[j].s;
                uint32_t r;
                Env::step_rec(sh, tab, sj, valid ? a_cur[j] : 0u, H[j], st[j].s, r,
                              [&]() { return Env::elem(Env::quad_block(key, lane, SENSOR_BLOCK + 1u), (uint32_t)j); });
                if constexpr (Env::STOCHASTIC) {                                // the gate said no (rock.py:443): nothing happens
                    sj = acts[j] ? sj : st[j].s;
                    r = acts[j] ? r : a_cur[j];
                }
                if constexpr (Pol::TAPE) {                                      // an out-of-range byte: untouched, (0, 0, 0), counted
                    sj = valid ? sj : st[j].s;
                    r = valid ? r : a_cur[j];
                    n_bad += (uint32_t)(valid || frozen[j] ? 0 : 1);
                }
                st[j].s = frozen[j] ? st[j].s : sj;
                recs[j] = frozen[j] ? recs[j] : r;
            }
        }
        if constexpr (RETS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) out.put(j, recs[j], !frozen[j]);
        } else {
            out.put_records(recs, a_nx);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) frozen[j] = (recs[j] >> 24) != 0u;
        if constexpr (Pol::TAPE) {
            pol.end(s, a_nx);                                                   // the row of step s + 1, asked for when step s began
#pragma unroll
            for (int j = 0; j < 4; ++j) a_cur[j] = a_nx[j];
        }
    }
    pol.count_bad(n_bad);
    st_stream4(state + l0, (uint32_t)st[0].s, (uint32_t)st[1].s, (uint32_t)st[2].s, (uint32_t)st[3].s);
    if (W == 2)
        st_stream4(state + n + l0, (uint32_t)((uint64_t)st[0].s >> 32), (uint32_t)((uint64_t)st[1].s >> 32),
                   (uint32_t)((uint64_t)st[2].s >> 32), (uint32_t)((uint64_t)st[3].s >> 32));
    st_stream(reinterpret_cast<uint32_t *>(done + l0),
              (uint32_t)frozen[0] | ((uint32_t)frozen[1] << 8) | ((uint32_t)frozen[2] << 16) | ((uint32_t)frozen[3] << 24));
    if constexpr (RETS) out.finish4(l0);
}

// the envs with a quad-per-thread frozen loop: RockSample and StochasticRock (the table-driven step_rec)
template <class Env, class = void> struct rock_quad_of : std::false_type {};
template <class Env> struct rock_quad_of<Env, std::enable_if_t<Env::QUAD_TAB>> : std::true_type {};

// ---- launchers --------------------------------------------------------------------------------------------------------------
template <class Env>
static int launch_reset_where(const typename Env::Params &p, uint32_t *state, int32_t *ob, uint8_t *done, const uint8_t *where,
                              int64_t n, uint64_t seed, uint32_t lane0, uint64_t t, void *stream)
{
    hipLaunchKernelGGL(reset_where_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, ob, done, where, n,
                       make_key(seed, t), lane0);
    return (int)hipGetLastError();
}

// one launch of up to pomdp_fuse_max() steps: the quad loop where RockSample's batch qualifies for steps_quad_kernel's gates
// (full workgroups of 1024 lanes from QUAD_MIN_ROCK / QUAD_MIN_STOCHROCK lanes, 16 steps per launch, aligned columns), the
// general loop otherwise
template <class Env, class L>
static int launch_episodes_l(const typename Env::Params &p, uint32_t *state, uint8_t *done, void *out0, void *out1, uint64_t dbits,
                             int64_t n, uint64_t seed, uint32_t lane0, uint64_t t, int k, int64_t rec, TapeRef tape, void *stream)
{
    const bool taped = tape.base != nullptr;
    char lname[32];
    snprintf(lname, sizeof lname, ", %s%s", L::NAME, taped ? ", Tape" : "");
    const RngKey key = make_key(seed, t);
    if constexpr (rock_quad_of<Env>::value) {
        bool quad_ok = n % (4 * BLOCK) == 0 && n >= (Env::STOCHASTIC ? QUAD_MIN_STOCHROCK : QUAD_MIN_ROCK) && k >= 16 &&
                       Env::tab_ok(p) && (reinterpret_cast<uintptr_t>(state) & 15u) == 0 &&
                       (reinterpret_cast<uintptr_t>(done) & 3u) == 0 && rec % 4 == 0;
        if (L::ID == POMDP_LAYOUT_PACKED) quad_ok = quad_ok && (reinterpret_cast<uintptr_t>(out0) & 15u) == 0;
        if (L::ID == POMDP_LAYOUT_NARROW) quad_ok = quad_ok && (reinterpret_cast<uintptr_t>(out0) & 3u) == 0;
        if (L::ID == LAYOUT_RETURNS) quad_ok = quad_ok && ((reinterpret_cast<uintptr_t>(out0) | reinterpret_cast<uintptr_t>(out1)) & 15u) == 0;
        if (taped) quad_ok = quad_ok && (reinterpret_cast<uintptr_t>(tape.base) & 3u) == 0 && tape.stride % 4 == 0;
        if (quad_ok) {
            note_fused("episodes_quad_kernel", Env::NAME, lname);
            const dim3 qgrid((unsigned)(n / (4 * BLOCK)));
            if (taped)
                hipLaunchKernelGGL((episodes_quad_kernel<Env, L, TapeQuad>), qgrid, dim3(BLOCK), 0, (hipStream_t)stream, state, done, out0,
                                   out1, dbits, n, key, lane0, k, rec, p, tape);
            else
                hipLaunchKernelGGL((episodes_quad_kernel<Env, L, SyntheticQuad>), qgrid, dim3(BLOCK), 0, (hipStream_t)stream, state, done,
                                   out0, out1, dbits, n, key, lane0, k, rec, p, tape);
            return (int)hipGetLastError();
        }
    }
    note_fused("episodes_kernel", Env::NAME, lname);
    if (taped)
        hipLaunchKernelGGL((episodes_kernel<Env, L, true>), dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, state, done, out0,
                           out1, dbits, n, key, lane0, k, rec, p, tape);
    else
        hipLaunchKernelGGL((episodes_kernel<Env, L, false>), dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, state, done, out0,
                           out1, dbits, n, key, lane0, k, rec, p, tape);
    return (int)hipGetLastError();
}

} // namespace pomdp

extern "C" {

int pomdp_reset_where(int env, const void *params, uint32_t *state, int32_t *ob, uint8_t *done, const uint8_t *where, int64_t n,
                      uint64_t seed, uint32_t lane0, uint64_t t, void *stream)
{
    if (!params || !state || bad_range(n, lane0)) return POMDP_E_BADARG;
    const int rc = dispatch_env(env, params, [](auto, const auto &) { return 0; });
    if (rc) return rc;
    if (n == 0) return 0;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_reset_where<E>(p, state, ob, done, where, n, seed, lane0, t, stream);
    });
}

int pomdp_finish_episodes(const pomdp_episode_args *a, uint64_t t0, int64_t k_steps, void *stream)
{
    if (!a || !a->params || !a->state || !a->done || k_steps < 0 || bad_range(a->n, a->lane0) || (a->lane0 & 3u))
        return POMDP_E_BADARG;
    const int64_t n = a->n;
    const bool rets = a->layout == POMDP_LAYOUT_RETURNS;
    if (rets) {
        const pomdp_return_stats *st = a->stats;
        if (!st || !st->acc || !st->cnt || st->pitch < n || !(st->discount == st->discount)) return POMDP_E_BADARG;
    } else if (a->layout == POMDP_LAYOUT_PACKED || a->layout == POMDP_LAYOUT_NARROW) {
        if (!a->traj || a->pitch < n || (a->layout == POMDP_LAYOUT_NARROW && a->pitch % 4 != 0)) return POMDP_E_BADARG;
    } else {
        return POMDP_E_BADARG;                                          // frozen mode has no 13-byte layouts
    }
    if (a->tape && (!a->tape->actions || a->tape->stride < n)) return POMDP_E_BADARG;
    // a Packed record (and a Narrow plane) keeps the observation in a byte: Tag's "opponent seen" value is a ctor argument
    if (!rets && a->env == POMDP_ENV_TAG && (uint32_t)((const pomdp_tag_params *)a->params)->obs_cells > 255u) return POMDP_E_BADPARAMS;
    int rc = dispatch_env(a->env, a->params, [](auto, const auto &) { return 0; });
    if (rc) return rc;
    if (k_steps == 0 || n == 0) return 0;
    uint64_t dbits = 0;
    if (rets) memcpy(&dbits, &a->stats->discount, 8);
    const int64_t row_bytes = 4 * a->pitch;                            // Packed: pitch records; Narrow: four planes of pitch bytes
    const int64_t FUSE_MAX = fuse_max();
    for (int64_t s = 0; s < k_steps; s += FUSE_MAX) {
        const int c = (int)(k_steps - s < FUSE_MAX ? k_steps - s : FUSE_MAX);
        const TapeRef tape = a->tape ? TapeRef{a->tape->actions + s * a->tape->stride, a->tape->stride, a->err} : NO_TAPE;
        rc = dispatch_env(a->env, a->params, [&](auto tag, const auto &p) {
            using E = typename decltype(tag)::Env;
            const uint64_t t = t0 + (uint64_t)s;
            if (rets)
                return launch_episodes_l<E, Returns<E>>(p, a->state, a->done, a->stats->acc, a->stats->cnt, dbits, n, a->seed, a->lane0, t,
                                                        c, a->stats->pitch, tape, stream);
            void *base = reinterpret_cast<uint8_t *>(a->traj) + s * row_bytes;
            if (a->layout == POMDP_LAYOUT_PACKED)
                return launch_episodes_l<E, Packed>(p, a->state, a->done, base, nullptr, 0, n, a->seed, a->lane0, t, c, a->pitch, tape, stream);
            return launch_episodes_l<E, Narrow>(p, a->state, a->done, base, nullptr, 0, n, a->seed, a->lane0, t, c, a->pitch, tape, stream);
        });
        if (rc) return rc;
    }
    return 0;
}

} // extern "C"
