// planner_preferred.hip — rollouts under the env's preferred-action policy (pomdp_rollout_preferred / pomdp_plan_preferred): the
// simulations of a POMCP-style planner pick from _generate_preferred(history), each carrying its own copy of the policy's inputs.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
// A translation unit of its own: the uniform rollout_kernel of planner.hip compiles exactly as it did without this file.
#include "kernels_common.hip.h"
#include "planner_common.hip.h"

namespace pomdp {

// rollout_kernel under the env's preferred-action policy (include/pomdp_hip.h: pomdp_rollout_preferred): the same lanes,
// words, step and return, with the list of step k being _generate_preferred(history) of the SIMULATION's own statistics and
// history.  Lane i belongs to root r = i / sims_per_root and starts from state column i / sims_per_col (true states:
// sims_per_col = sims_per_root; P particles per root: sims_per_root / P) and from root r's policy words, which it then
// keeps private, in registers, as heuristic_steps_kernel keeps a lane's: the derived words check_ok / move_ok, size,
// last action / observation, prev_ob — Env::preferred_mask reads nothing else.
// The per-rock arrays (count, measured, lkv, lkw and the two history sums — prob_valuable only enters the policy through its
// check_ok bit and is a function of lkv / lkw, so it is not carried) change on a CHECK only and do not fit in registers:
// copy on first touch.  Bit j of `touched` says that the simulation owns entry (j, i) of the workspace; a CHECK of rock j
// reads root r's entry while the bit is clear and its own afterwards, and always writes its own.  The workspace starts
// uninitialised and the roots' arrays are only read.  A simulation reads only what it wrote itself, in program order: plain
// loads and stores, no fence.  Loads and stores share one counter on gfx9 — this loop stores on CHECK steps only, and a
// CHECK's loads wait for the simulation's earlier stores, which is the read-modify-write's own dependency.
// Inactive lanes keep executing the step (the quad's blocks travel by quad_transpose4) and discard it; the exit is
// wave-uniform, as in rollout_kernel.
template <class Env>
__global__ __launch_bounds__(BLOCK) void rollout_preferred_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                                  int64_t n_roots, int64_t sims_per_root, int64_t sims_per_col,
                                                                  int depth, double discount, pomdp_rock_belief b, pomdp_history h,
                                                                  const int32_t *__restrict__ prev_ob, int4 *ws_stat,
                                                                  double *ws_lkv, double *ws_lkw, RngKey key0, uint32_t lane0,
                                                                  double *__restrict__ ret, int32_t *__restrict__ n_steps,
                                                                  int32_t *__restrict__ first_action, int32_t *__restrict__ last_ob,
                                                                  uint8_t *__restrict__ terminated)
{
#pragma clang fp contract(off)
    __shared__ typename Env::Shared sh;
    constexpr bool TAB = ROLLOUT_TAB<Env>::value;
    constexpr bool REC = TAB;
    __shared__ typename step_tab_of<Env, TAB>::type tab;
    Env::stage(sh, p, (int)threadIdx.x);
    stage_policy_tables<Env>(sh, p);
    __syncthreads();
    if constexpr (TAB) {
        Env::build_rec_tab(tab, sh, p, (int)threadIdx.x);
        __syncthreads();
    }
    const int K = rock_count(p);
    const int64_t n = n_roots * sims_per_root;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in_range = i < n;
    const int64_t ic = in_range ? i : n - 1;                   // memory index only: threads past n read simulation n - 1's words
    const int64_t root = ic / sims_per_root;
    typename Env::State st;
    Env::load(st, state, n_roots * (sims_per_root / sims_per_col), (uint32_t)(ic / sims_per_col));
    int hsize = h.size[root], la = h.last_action[root], lo = h.last_ob[root], pob = 0;
    uint32_t ck = 0, mv = 0, touched = 0;
    if constexpr (Env::HAS_ROCKS) { ck = b.check_ok[root]; mv = h.move_ok[root]; pob = prev_ob[root]; }
    const uint32_t lane = lane0 + (uint32_t)i;                 // the UNCLAMPED index: the quad element of a ragged last quad
    double acc = 0.0, disc = 1.0;
    int k = 0, d = 0, o = 0, first = -1;
    bool active = in_range, live_wave = true;
    const uint64_t t0 = ((uint64_t)key0.t_hi << 32) | key0.t_lo;
    for (int base = 0; base < depth && live_wave; base += 4) {
        const uint4 pw = stream_block(key0, lane, POMDP_STREAM_ROLLOUT, (uint32_t)(base >> 2));
        uint4 sq = make_uint4(0, 0, 0, 0);
        if constexpr (Env::QUAD_SENSOR || quad_word_env<Env>::value) {   // this lane's share: the quad's STEP block of step base + (lane & 3)
            const uint64_t te = t0 + (uint64_t)base + (uint64_t)(lane & 3u);
            RngKey ke = key0;
            ke.t_lo = (uint32_t)te; ke.t_hi = (uint32_t)(te >> 32);
            sq = quad_transpose4(Env::quad_block(ke, lane, 0u), lane & 3u);   // .J: this lane's word of step base + J
        }
        auto one_step = [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const int step = base + J;
            if (step >= depth || !live_wave) return;
            // _generate_preferred(history): the mask in ascending action order, or — empty — _generate_legal()
            const uint32_t m = Env::preferred_mask(sh, p, st, h, n_roots, (uint32_t)root, ck, mv, hsize, la, lo);
            const auto L = LegalOf<Env>::make(sh, p, st, m != 0u);
            const int count = m ? __popc(m) : L.count;
            active = active && !d && count > 0;
            if (!__any(active)) { live_wave = false; return; }           // wave-uniform exit
            const RngKey key = key_at(key0, t0 + (uint64_t)step);
            const uint32_t w = comp<J>(pw);
            const int idx = (int)__umulhi(w, (uint32_t)(count > 0 ? count : 1));
            const int a = m ? nth_set_bit(m, idx) : LegalOf<Env>::pick(sh, p, st, L, idx);
            typename Env::State nx = st;
            int o2, d2;
            double r;
            if constexpr (Env::QUAD_SENSOR) {      // every lane runs it (the broadcasts need the whole quad); inactive lanes discard
                if constexpr (REC) {
                    uint32_t rec;
                    Env::step_rec(sh, tab, nx.s, (uint32_t)a, comp<J>(sq), nx.s, rec,
                                  [&]() { return Env::elem(Env::quad_block(key, lane, 1u), lane & 3u); });
                    o2 = (int)__builtin_amdgcn_ubfe(rec, 8u, 8u);
                    r = (double)(int32_t)__builtin_amdgcn_sbfe(rec, 16u, 8u);
                    d2 = (int)(rec >> 24);
                }
                else Env::step_with_H(sh, p, nx, a, key, lane, comp<J>(sq), o2, r, d2);
            } else if constexpr (quad_word_env<Env>::value) {          // Tag: the lane's word of the quad's block
                Env::step_w(sh, p, nx, a, key, lane, comp<J>(sq), o2, r, d2);
            } else {
                Env::step(sh, p, nx, a, key, lane, o2, r, d2);
            }
            if (active) {
                st = nx; o = o2; d = d2;
                if (step == 0) first = a;
                const double term = disc * r;
                acc = acc + term;
                disc = disc * discount;
                k = step + 1;
                // history.append(Transition(prev_ob, a, r, o2, d2)) and the side statistics, on the simulation's own copies
                la = a; lo = o2;
                hsize += (int)(hsize != 0x7FFFFFFF);
                if constexpr (Env::HAS_ROCKS) {
                    if (a >= 5 && a < 5 + K) {                           // an executed CHECK of rock j
                        const int j = a - 5;
                        const uint32_t bit = 1u << j;
                        const int64_t kr = (int64_t)j * n_roots + root, ks = (int64_t)j * n + i;
                        int cnt, meas, ts, tm;
                        double lkv, lkw;
                        if (touched & bit) {
                            const int4 v = ws_stat[ks];
                            cnt = v.x; meas = v.y; ts = v.z; tm = v.w;
                            lkv = ws_lkv[ks]; lkw = ws_lkw[ks];
                        } else {
                            cnt = b.count[kr]; meas = b.measured[kr]; ts = h.total_sample[kr]; tm = h.total_move[kr];
                            lkv = b.lkv[kr]; lkw = b.lkw[kr];
                        }
                        // the history's two sums and Env::belief_update, on the private entry
                        const int ds = check_ds(o2), dm = check_dm(o2, pob == 1);
                        if (ds) { ts += ds; mv = with_bit(mv, bit << 16, ts > 0); }
                        if (dm) { tm += dm; mv = with_bit(mv, bit, tm >= 0); }
                        if (o2 != 0 && !d2) {                            // CHECK does not move: st is where the reading was taken
                            const auto u = Env::check_update(Env::sensor_eff(sh, p, st, j & 15), o2, lkv, cnt, lkw);
                            meas += 1; cnt = u.count; lkv = u.lkv; lkw = u.lkw;
                            ck = with_bit(ck, bit, Env::check_ok(meas, cnt, u.pv));
                        }
                        ws_stat[ks] = make_int4(cnt, meas, ts, tm);
                        ws_lkv[ks] = lkv; ws_lkw[ks] = lkw;
                        touched |= bit;
                    }
                    pob = o2;
                }
            }
        };
        one_step(std::integral_constant<int, 0>{});
        one_step(std::integral_constant<int, 1>{});
        one_step(std::integral_constant<int, 2>{});
        one_step(std::integral_constant<int, 3>{});
    }
    if (in_range) {
        ret[i] = acc;
        first_action[i] = first;
        if (n_steps) n_steps[i] = k;                          // kernel arguments: wave-uniform
        if (last_ob) last_ob[i] = o;
        if (terminated) terminated[i] = (uint8_t)d;
    }
}

// the arguments are checked by the entry point
template <class Env>
static int launch_rollout_preferred(const typename Env::Params &p, const uint32_t *state, int64_t n_roots, int n_particles,
                                    int64_t sims, int depth, double discount, const pomdp_rock_belief *b, const pomdp_history *h,
                                    const int32_t *prev_ob, void *workspace, uint64_t seed, uint32_t lane0, uint64_t t0,
                                    double *ret, int32_t *n_steps, int32_t *first_action, int32_t *last_ob, uint8_t *terminated,
                                    void *stream)
{
    const int64_t n = n_roots * sims;
    if (n == 0) return 0;
    const int64_t cells = Env::HAS_ROCKS ? n * rock_count(p) : 0;          // workspace: int4 [K][n], then lkv, lkw double [K][n]
    int4 *const ws_stat = (int4 *)workspace;
    double *const ws_lkv = (double *)(ws_stat + cells);
    hipLaunchKernelGGL(rollout_preferred_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, n_roots,
                       sims, sims / n_particles, depth, discount, (Env::HAS_ROCKS && b) ? *b : NO_BELIEF, *h, prev_ob, ws_stat, ws_lkv,
                       ws_lkv + cells, make_key(seed, t0), lane0, ret, n_steps, first_action, last_ob, terminated);
    return (int)hipGetLastError();
}

} // namespace pomdp

extern "C" {

int64_t pomdp_rollout_preferred_workspace(int env, const void *params, int64_t n_roots, int64_t sims_per_root)
{
    if (env != POMDP_ENV_ROCK || !params || n_roots < 0 || sims_per_root < 0) return 0;
    return 32 * (int64_t)((const pomdp_rock_params *)params)->num_rocks * n_roots * sims_per_root;
}

int pomdp_rollout_preferred(int env, const void *params, const uint32_t *state, int64_t n_roots, int n_particles,
                            int64_t sims_per_root, int depth, double discount, const pomdp_rock_belief *b,
                            const pomdp_history *h, const int32_t *prev_ob, void *workspace, uint64_t seed, uint32_t lane0,
                            uint64_t t0, double *ret, int32_t *n_steps, int32_t *first_action, int32_t *last_ob,
                            uint8_t *terminated, void *stream)
{
    const bool rock = env == POMDP_ENV_ROCK;
    if (!params || !state || !ret || !first_action || n_roots < 0 || n_particles < 1 || sims_per_root < n_particles ||
        sims_per_root % n_particles || depth < 0 || bad_range(n_roots * sims_per_root, lane0) || (lane0 & 3u))
        return POMDP_E_BADARG;
    if (!history_ok(h, rock) || h->max_size != -1) return POMDP_E_BADARG;     // a simulation would have to carry the window
    if (rock && (!belief_ok(b) || !prev_ob || !workspace || ((uintptr_t)workspace & 15u))) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        if constexpr (has_policy<E>::value) {
            return launch_rollout_preferred<E>(p, state, n_roots, n_particles, sims_per_root, depth, discount, b, h, prev_ob,
                                               workspace, seed, lane0, t0, ret, n_steps, first_action, last_ob, terminated, stream);
        } else {                                                   // the preferred list is the legal list: the uniform kernel
            return pomdp_rollout(env, params, state, n_roots * n_particles, sims_per_root / n_particles, depth, discount, 0, seed,
                                 lane0, t0, ret, n_steps, first_action, last_ob, terminated, stream);
        }
    });
}

int pomdp_plan_preferred(int env, const void *params, const uint32_t *state, int64_t n_roots, int n_particles,
                         int64_t sims_per_root, int depth, double discount, const pomdp_rock_belief *b, const pomdp_history *h,
                         const int32_t *prev_ob, void *workspace, uint64_t seed, uint32_t lane0, uint64_t t0, double *sim_ret,
                         int32_t *sim_first_action, const pomdp_plan_out *out, void *stream)
{
    return plan_with(env, params, n_roots, sims_per_root, sim_ret, sim_first_action, out, stream, [&]() {
        return pomdp_rollout_preferred(env, params, state, n_roots, n_particles, sims_per_root, depth, discount, b, h, prev_ob,
                                       workspace, seed, lane0, t0, sim_ret, nullptr, sim_first_action, nullptr, nullptr, stream);
    });
}

} // extern "C"
