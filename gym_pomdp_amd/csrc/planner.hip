// planner.hip — planner hooks: _generate_legal, _compute_prob, fused rollouts, side statistics, History, _generate_preferred, the heuristic-policy loop (heuristic_impl.hip.h).
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "kernels_common.hip.h"
#include "planner_common.hip.h"
#include "heuristic_impl.hip.h"

namespace pomdp {

// ---------------------------------------------------------------------------
// planner hooks: _generate_legal and random rollouts
// ---------------------------------------------------------------------------
template <class Env>
__global__ __launch_bounds__(BLOCK) void legal_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                      int32_t *__restrict__ list, int32_t *__restrict__ len, int64_t n,
                                                      int stride)
{
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    typename Env::State st;
    Env::load(st, state, n, i);
    const int c = Env::legal_count(sh, p, st);
    len[i] = c;
    for (int k = 0; k < stride; ++k) list[i * stride + k] = k < c ? Env::legal_nth(sh, p, st, k) : -1;
}

template <class Env>
__global__ __launch_bounds__(BLOCK) void prob_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                     const int32_t *__restrict__ action, const int32_t *__restrict__ ob,
                                                     double *__restrict__ out, int64_t n)
{
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    typename Env::State st;
    Env::load(st, state, n, i);
    const int a = action[i];
    out[i] = (unsigned)a < (unsigned)Env::n_actions(p) ? Env::compute_prob(sh, p, st, a, ob[i]) : 0.0;
}

// ---------------------------------------------------------------------------
// heuristic-policy support: side statistics, history sums, _generate_preferred
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void belief_reset_kernel(pomdp_rock_belief b, int K, const uint8_t *__restrict__ where,
                                                             int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (where && !where[i])) return;
    for (int j = 0; j < K; ++j) belief_fresh_rock(b, (int64_t)j * n + i);
    b.check_ok[i] = (1u << K) - 1u;
}

__global__ __launch_bounds__(BLOCK) void belief_refresh_kernel(pomdp_rock_belief b, int K, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t m = 0;
    for (int j = 0; j < K; ++j) {
        const int64_t k = (int64_t)j * n + i;
        m |= (uint32_t)RockEnv<1>::check_ok(b.measured[k], b.count[k], b.prob_valuable[k]) << j;
    }
    b.check_ok[i] = m;
}

template <class Env>
__global__ __launch_bounds__(BLOCK) void belief_update_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                              const int32_t *__restrict__ action, const int32_t *__restrict__ ob,
                                                              const uint8_t *__restrict__ done, pomdp_rock_belief b, int64_t n,
                                                              int auto_reset)
{
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (done[i]) {
        if (auto_reset) {
            for (int j = 0; j < p.num_rocks; ++j) belief_fresh_rock(b, (int64_t)j * n + i);
            b.check_ok[i] = (1u << p.num_rocks) - 1u;
        }
        return;
    }
    const int a = action[i], o = ob[i];
    if (a <= 4 || a >= 5 + p.num_rocks || o == 0) return;                      // not an executed CHECK
    typename Env::State st;
    Env::load(st, state, n, (uint32_t)i);
    uint32_t ck = b.check_ok[i];
    Env::belief_update(sh, p, st, a, o, b, n, (uint32_t)i, ck);
    b.check_ok[i] = ck;
}

template <class Env>
__global__ __launch_bounds__(BLOCK) void select_target_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                              pomdp_rock_belief b, int32_t *__restrict__ target, int64_t n)
{
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    typename Env::State st;
    Env::load(st, state, n, (uint32_t)i);
    target[i] = Env::select_target(sh, p, st, b, n, (uint32_t)i);
}

__global__ __launch_bounds__(BLOCK) void history_clear_kernel(pomdp_history h, int K, const uint8_t *__restrict__ where, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || (where && !where[i])) return;
    history_fresh(h, K, n, i);
}

// rock.py:541-544 History.append + the sums _generate_preferred takes over the records (rock.py:303-310, 327-334)
__global__ __launch_bounds__(BLOCK) void history_append_kernel(pomdp_history h, int K, const int32_t *__restrict__ observation,
                                                               const int32_t *__restrict__ action,
                                                               const int32_t *__restrict__ next_observation,
                                                               const uint8_t *__restrict__ done, int64_t n, int auto_reset)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (done[i] && auto_reset) {                                               // next episode: a new, empty History
        history_fresh(h, K, n, i);
        return;
    }
    const int a = action[i], o = next_observation[i];
    // append() takes any int32 (37 & 31 is CHECK 0; 4 << 5 is the BAD bit): the window keeps what the sums take from the
    // record — an action that is no action of this env as a non-CHECK (31), a next observation that is no CHECK result as 0
    const int wa = (a >= 0 && a < 5 + K) ? a : 31, wo = (o == 1 || o == 2) ? o : 0;
    int hsize = h.size[i], head = h.head ? h.head[i] : 0;
    uint32_t mv = K ? h.move_ok[i] : 0u;
    history_push(h, K, wa, wo, observation[i], n, (uint32_t)i, hsize, head, mv);
    h.size[i] = hsize; h.last_action[i] = a; h.last_ob[i] = o;
    if (K) h.move_ok[i] = mv;
    if (h.head) h.head[i] = head;
}

template <class Env>
__global__ __launch_bounds__(BLOCK) void preferred_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                          pomdp_rock_belief b, pomdp_history h, int32_t *__restrict__ list,
                                                          int32_t *__restrict__ len, int64_t n, int stride)
{
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    stage_policy_tables<Env>(sh, p);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    typename Env::State st;
    Env::load(st, state, n, (uint32_t)i);
    uint32_t m = Env::preferred_mask(sh, p, st, b, h, n, (uint32_t)i);
    if (m) {                                                                   // ascending action order
        const int c = __popc(m);
        len[i] = c;
        for (int k = 0; k < stride; ++k) {
            int a = -1;
            if (k < c) { a = __ffs((int)m) - 1; m &= m - 1u; }
            list[i * stride + k] = a;
        }
    } else {                                                                   // _generate_legal()
        const int c = Env::legal_count(sh, p, st);
        len[i] = c;
        for (int k = 0; k < stride; ++k) list[i * stride + k] = k < c ? Env::legal_nth(sh, p, st, k) : -1;
    }
}

// the caller's np.random.choice(list): the synthetic policy's word of the lane picks the element
__global__ __launch_bounds__(BLOCK) void pick_actions_kernel(const int32_t *__restrict__ list, const int32_t *__restrict__ len,
                                                             int stride, int32_t *__restrict__ action, int64_t n, RngKey key,
                                                             uint32_t lane0)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t lane = lane0 + (uint32_t)i, e = lane & 3u;
    const uint4 w = stream_block(key, lane >> 2, POMDP_STREAM_ACTION, 0u);
    const uint32_t word = e == 0 ? w.x : e == 1 ? w.y : e == 2 ? w.z : w.w;
    const int c = len[i];
    action[i] = c > 0 ? list[i * stride + (int64_t)__umulhi(word, (uint32_t)c)] : -1;
}

// Lane i simulates from root state column i / sims_per_root for up to `depth` steps: the state lives in registers
// and nothing is written but the per-lane results.  Random words, four steps at a time:
//   - the policy pick of step k is word k of the lane's ROLLOUT stream at t0: one Philox block per four steps;
//   - the env draws come from stream STEP at t0 + k, as in step().  RockSample's STEP block is shared by the four
//     lanes of a quad, so lane e of a quad computes the block of step 4 g + e and the words travel by DPP
//     quad-broadcast: one block per lane per four steps instead of four.
// The discounted return accumulates in IEEE double with separate multiply and add (so a CPU restatement reproduces
// it bit-for-bit).
template <class Env>
__global__ __launch_bounds__(BLOCK) void rollout_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                        int64_t n_roots, int64_t sims_per_root, int depth,
                                                        double discount, int all_actions, RngKey key0, uint32_t lane0,
                                                        double *__restrict__ ret, int32_t *__restrict__ n_steps,
                                                        int32_t *__restrict__ first_action, int32_t *__restrict__ last_ob,
                                                        uint8_t *__restrict__ terminated)
{
#pragma clang fp contract(off) // the discounted return must not be fused into FMAs (hipcc defaults to contract=fast)
    __shared__ typename Env::Shared sh;
    constexpr bool TAB = ROLLOUT_TAB<Env>::value;            // RockSample: the (position, action) table of the fused loops,
    constexpr bool REC = TAB;                                // whose lane step yields the packed record (step_rec)
    __shared__ typename step_tab_of<Env, TAB>::type tab;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
    if constexpr (TAB) {
        Env::build_rec_tab(tab, sh, p, (int)threadIdx.x);
        __syncthreads();
    }
    const int64_t n = n_roots * sims_per_root;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in_range = i < n;
    const int64_t ic = in_range ? i : n - 1;
    typename Env::State st;
    Env::load(st, state, n_roots, (uint32_t)(ic / sims_per_root));
    const uint32_t lane = lane0 + (uint32_t)i;
    const int n_act = Env::n_actions(p);
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
            const auto L = LegalOf<Env>::make(sh, p, st, all_actions != 0);
            const int count = all_actions ? n_act : L.count;
            active = active && !d && count > 0;
            if (!__any(active)) { live_wave = false; return; }           // wave-uniform exit
            const RngKey key = key_at(key0, t0 + (uint64_t)step);
            const uint32_t w = comp<J>(pw);
            const int idx = (int)__umulhi(w, (uint32_t)(count > 0 ? count : 1));
            const int a = all_actions ? idx : LegalOf<Env>::pick(sh, p, st, L, idx);
            typename Env::State nx = st;
            int o2, d2;
            double r;
            if constexpr (Env::QUAD_SENSOR) {      // every lane runs it (the broadcasts need the whole quad); inactive lanes discard
                if constexpr (REC) {
                    // a simulation stops at its terminal step, so the state after one is never read: no fresh episode to pass
                    uint32_t rec;
                    Env::step_rec(sh, tab, nx.s, (uint32_t)a, comp<J>(sq), nx.s, rec,
                                  [&]() { return Env::elem(Env::quad_block(key, lane, 1u), lane & 3u); });
                    o2 = (int)__builtin_amdgcn_ubfe(rec, 8u, 8u);
                    r = (double)(int32_t)__builtin_amdgcn_sbfe(rec, 16u, 8u);
                    d2 = (int)(rec >> 24);
                }
                else Env::step_with_H(sh, p, nx, a, key, lane, comp<J>(sq), o2, r, d2);
            } else if constexpr (quad_word_env<Env>::value) {          // Tiger, Tag: the lane's word of the quad's block
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

// The planning step's reduction (include/pomdp_hip.h: pomdp_plan): one workgroup per root turns the root's simulations into
// visits / mean return per first action and picks the best one.  The order of the float64 additions is part of the
// contract — chunks of 64 simulations by index, simulation-index order within a chunk, chunk order across chunks, each sum
// starting from +0.0 — so the layout follows it: the root's returns and first actions are staged through LDS a tile of
// PLAN_TILE = 16 chunks at a time; the tile's (chunk, action) pairs are dealt out one per thread, each walking its chunk in
// index order (an addition of nothing leaves the sum alone, which is what skipping a simulation means, and a sum that
// started at +0.0 is never -0.0); the per-chunk sums go through LDS and thread a adds them in chunk order into its running
// total across tiles.  No atomics, no cross-workgroup traffic.  LDS is sized by the action count (dynamic: 13 KB for
// RockSample(15,15)'s 20 actions), so that a CU holds eight roots at once — configs[4]'s 2048 roots are one round of
// workgroups; a chunk's returns sit 65 doubles apart so that threads on different chunks read different banks.
constexpr int PLAN_CHUNKS = 16, PLAN_TILE = PLAN_CHUNKS * POMDP_PLAN_CHUNK, PLAN_ROW = POMDP_PLAN_CHUNK + 1;
static inline size_t plan_lds_bytes(int n_act)
{
    return sizeof(double) * (PLAN_CHUNKS * PLAN_ROW + (size_t)PLAN_CHUNKS * n_act + n_act) + sizeof(int32_t) * n_act +
           PLAN_TILE + (size_t)PLAN_CHUNKS * n_act;
}
__global__ __launch_bounds__(BLOCK) void plan_reduce_kernel(const double *__restrict__ ret, const int32_t *__restrict__ first_action,
                                                            int64_t sims, int n_act, pomdp_plan_out out)
{
#pragma clang fp contract(off)
    extern __shared__ double plan_lds[];
    double *const r_lds = plan_lds;                                        // [PLAN_CHUNKS][PLAN_ROW]
    double *const part = r_lds + PLAN_CHUNKS * PLAN_ROW;                   // [PLAN_CHUNKS][n_act]
    double *const q_lds = part + PLAN_CHUNKS * n_act;                      // [n_act]
    int32_t *const n_lds = reinterpret_cast<int32_t *>(q_lds + n_act);     // [n_act]
    uint8_t *const a_lds = reinterpret_cast<uint8_t *>(n_lds + n_act);     // [PLAN_TILE]; 255: no step taken / out of range
    uint8_t *const cnt = a_lds + PLAN_TILE;                                // [PLAN_CHUNKS][n_act], <= 64 each
    const int64_t root = blockIdx.x;
    const int tid = (int)threadIdx.x;
    const double *const rr = ret + root * sims;
    const int32_t *const fa = first_action + root * sims;
    double total = 0.0;                                      // thread a < n_act: action a
    int32_t visits = 0;
    for (int64_t base = 0; base < sims; base += PLAN_TILE) {
        const int tile = (int)(sims - base < PLAN_TILE ? sims - base : PLAN_TILE);
        for (int j = tid; j < tile; j += BLOCK) {
            r_lds[(j >> 6) * PLAN_ROW + (j & 63)] = rr[base + j];
            const int32_t f = fa[base + j];
            a_lds[j] = (uint8_t)((uint32_t)f < (uint32_t)n_act ? f : 255);
        }
        __syncthreads();
        const int n_chunks = (tile + POMDP_PLAN_CHUNK - 1) / POMDP_PLAN_CHUNK;
        for (int item = tid; item < n_chunks * n_act; item += BLOCK) {
            const int c = item / n_act, a = item - c * n_act;
            const int len = tile - c * POMDP_PLAN_CHUNK < POMDP_PLAN_CHUNK ? tile - c * POMDP_PLAN_CHUNK : POMDP_PLAN_CHUNK;
            const double *const rc = r_lds + c * PLAN_ROW;
            const uint8_t *const ac = a_lds + c * POMDP_PLAN_CHUNK;
            double p = 0.0;
            int k = 0;
            for (int j = 0; j < len; ++j) {
                const bool hit = (int)ac[j] == a;
                const double with = p + rc[j];
                p = hit ? with : p;
                k += (int)hit;
            }
            part[c * n_act + a] = p;
            cnt[c * n_act + a] = (uint8_t)k;
        }
        __syncthreads();
        if (tid < n_act)
            for (int c = 0; c < n_chunks; ++c) { total = total + part[c * n_act + tid]; visits += (int32_t)cnt[c * n_act + tid]; }
        __syncthreads();                                     // the next tile overwrites r_lds / part
    }
    if (tid < n_act) {
        const double q = visits > 0 ? total / (double)visits : 0.0;
        out.q[root * out.stride + tid] = q;
        out.visits[root * out.stride + tid] = visits;
        q_lds[tid] = q;
        n_lds[tid] = visits;
    }
    __syncthreads();
    if (tid == 0) {                                          // n_act <= 255 values: the first strict maximum among the visited actions
        int b = -1;
        double bq = 0.0;
        for (int a = 0; a < n_act; ++a)
            if (n_lds[a] > 0 && (b < 0 || q_lds[a] > bq)) { b = a; bq = q_lds[a]; }
        out.best[root] = b;
        if (out.value) out.value[root] = b >= 0 ? bq : 0.0;
    }
}

template <class Env>
static int launch_legal(const typename Env::Params &p, const uint32_t *state, int32_t *list, int32_t *len, int64_t n,
                        int stride, void *stream)
{
    if (!state || !list || !len || n < 0 || stride < 1) return POMDP_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(legal_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, list, len,
                       n, stride);
    return (int)hipGetLastError();
}
template <class Env>
static int launch_prob(const typename Env::Params &p, const uint32_t *state, const int32_t *action, const int32_t *ob,
                       double *out, int64_t n, void *stream)
{
    if (!state || !action || !ob || !out || n < 0) return POMDP_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(prob_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, action, ob,
                       out, n);
    return (int)hipGetLastError();
}
template <class Env>
static int launch_rollout(const typename Env::Params &p, const uint32_t *state, int64_t n_roots, int64_t sims,
                          int depth, double discount, int flags, uint64_t seed, uint32_t lane0, uint64_t t0, double *ret,
                          int32_t *n_steps, int32_t *first_action, int32_t *last_ob, uint8_t *terminated, void *stream)
{
    if (!state || !ret || !first_action || n_roots < 0 || sims < 1 || depth < 0 ||
        bad_range(n_roots * sims, lane0) || (lane0 & 3u))                  // quad-shared blocks travel within the hardware quad
        return POMDP_E_BADARG;
    const int64_t n = n_roots * sims;
    if (n == 0) return 0;
    hipLaunchKernelGGL(rollout_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, n_roots,
                       sims, depth, discount, (flags & POMDP_ROLLOUT_ALL_ACTIONS) ? 1 : 0, make_key(seed, t0), lane0, ret,
                       n_steps, first_action, last_ob, terminated);
    return (int)hipGetLastError();
}
template <class Env>
static int launch_belief_update(const typename Env::Params &p, const uint32_t *state, const int32_t *action, const int32_t *ob,
                                const uint8_t *done, const pomdp_rock_belief *b, int64_t n, int flags, void *stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(belief_update_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, action,
                       ob, done, *b, n, (flags & POMDP_AUTO_RESET) ? 1 : 0);
    return (int)hipGetLastError();
}
template <class Env>
static int launch_select_target(const typename Env::Params &p, const uint32_t *state, const pomdp_rock_belief *b,
                                int32_t *target, int64_t n, void *stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(select_target_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state, *b,
                       target, n);
    return (int)hipGetLastError();
}
template <class Env>
static int launch_preferred(const typename Env::Params &p, const uint32_t *state, const pomdp_rock_belief *b,
                            const pomdp_history *h, int32_t *list, int32_t *len, int64_t n, int stride, void *stream)
{
    if (n == 0) return 0;
    hipLaunchKernelGGL(preferred_kernel<Env>, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p, state,
                       b ? *b : NO_BELIEF, *h, list, len, n, stride);
    return (int)hipGetLastError();
}

} // namespace pomdp

extern "C" {

int pomdp_legal_actions(int env, const void *params, const uint32_t *state, int32_t *list, int32_t *len, int64_t n,
                        int stride, void *stream)
{
    if (!params) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_legal<E>(p, state, list, len, n, stride, stream);
    });
}

int pomdp_compute_prob(int env, const void *params, const uint32_t *state, const int32_t *action, const int32_t *ob,
                       double *out, int64_t n, void *stream)
{
    if (!params) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_prob<E>(p, state, action, ob, out, n, stream);
    });
}

int pomdp_rollout(int env, const void *params, const uint32_t *root_state, int64_t n_roots, int64_t sims_per_root,
                  int depth, double discount, int flags, uint64_t seed, uint32_t lane0, uint64_t t0, double *ret,
                  int32_t *n_steps, int32_t *first_action, int32_t *last_ob, uint8_t *terminated, void *stream)
{
    if (!params) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_rollout<E>(p, root_state, n_roots, sims_per_root, depth, discount, flags, seed, lane0, t0, ret, n_steps,
                                 first_action, last_ob, terminated, stream);
    });
}

int pomdp_plan_reduce(const double *ret, const int32_t *first_action, int64_t n_roots, int64_t sims_per_root, int n_actions,
                      const pomdp_plan_out *out, void *stream)
{
    if (!ret || !first_action || n_roots < 0 || n_roots > 0x7FFFFFFF || sims_per_root < 1 || !plan_out_ok(out, n_actions))
        return POMDP_E_BADARG;
    if (n_roots == 0) return 0;
    hipLaunchKernelGGL(plan_reduce_kernel, dim3((unsigned)n_roots), dim3(BLOCK), plan_lds_bytes(n_actions), (hipStream_t)stream, ret,
                       first_action, sims_per_root, n_actions, *out);
    return (int)hipGetLastError();
}

int pomdp_plan(int env, const void *params, const uint32_t *root_state, int64_t n_roots, int64_t sims_per_root, int depth,
               double discount, int flags, uint64_t seed, uint32_t lane0, uint64_t t0, double *sim_ret,
               int32_t *sim_first_action, const pomdp_plan_out *out, void *stream)
{
    return plan_with(env, params, n_roots, sims_per_root, sim_ret, sim_first_action, out, stream, [&]() {
        return pomdp_rollout(env, params, root_state, n_roots, sims_per_root, depth, discount, flags, seed, lane0, t0, sim_ret,
                             nullptr, sim_first_action, nullptr, nullptr, stream);
    });
}

int pomdp_rock_belief_reset(const pomdp_rock_params *p, const pomdp_rock_belief *b, const uint8_t *where, int64_t n,
                            void *stream)
{
    if (!p || !belief_ok(b) || n < 0) return POMDP_E_BADARG;
    if (!rock_ok(p)) return POMDP_E_BADPARAMS;
    if (n == 0) return 0;
    hipLaunchKernelGGL(belief_reset_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, *b, p->num_rocks, where, n);
    return (int)hipGetLastError();
}

int pomdp_rock_belief_refresh(const pomdp_rock_params *p, const pomdp_rock_belief *b, int64_t n, void *stream)
{
    if (!p || !belief_ok(b) || n < 0) return POMDP_E_BADARG;
    if (!rock_ok(p)) return POMDP_E_BADPARAMS;
    if (n == 0) return 0;
    hipLaunchKernelGGL(belief_refresh_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, *b, p->num_rocks, n);
    return (int)hipGetLastError();
}

int pomdp_rock_belief_update(const pomdp_rock_params *p, const uint32_t *state, const int32_t *action, const int32_t *ob,
                             const uint8_t *done, const pomdp_rock_belief *b, int64_t n, int flags, void *stream)
{
    if (!p || !state || !action || !ob || !done || !belief_ok(b) || n < 0) return POMDP_E_BADARG;
    if (!rock_ok(p)) return POMDP_E_BADPARAMS;
    if (p->num_rocks <= 12) return launch_belief_update<RockEnv<1>>(*p, state, action, ob, done, b, n, flags, stream);
    return launch_belief_update<RockEnv<2>>(*p, state, action, ob, done, b, n, flags, stream);
}

int pomdp_rock_select_target(const pomdp_rock_params *p, const uint32_t *state, const pomdp_rock_belief *b, int32_t *target,
                             int64_t n, void *stream)
{
    if (!p || !state || !target || !belief_ok(b) || n < 0) return POMDP_E_BADARG;
    if (!rock_ok(p)) return POMDP_E_BADPARAMS;
    if (p->num_rocks <= 12) return launch_select_target<RockEnv<1>>(*p, state, b, target, n, stream);
    return launch_select_target<RockEnv<2>>(*p, state, b, target, n, stream);
}

int pomdp_history_clear(int env, const void *params, const pomdp_history *h, const uint8_t *where, int64_t n, void *stream)
{
    const int K = history_rocks(env, params);
    if (K < 0 || !history_ok(h, K > 0) || n < 0) return POMDP_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(history_clear_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, *h, K, where, n);
    return (int)hipGetLastError();
}

int pomdp_history_append(int env, const void *params, const pomdp_history *h, const int32_t *observation,
                         const int32_t *action, const int32_t *next_observation, const uint8_t *done, int64_t n, int flags,
                         void *stream)
{
    const int K = history_rocks(env, params);
    if (K < 0 || !history_ok(h, K > 0) || !observation || !action || !next_observation || !done || n < 0)
        return POMDP_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(history_append_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, *h, K, observation,
                       action, next_observation, done, n, (flags & POMDP_AUTO_RESET) ? 1 : 0);
    return (int)hipGetLastError();
}

int pomdp_preferred_actions(int env, const void *params, const uint32_t *state, const pomdp_rock_belief *b,
                            const pomdp_history *h, int32_t *list, int32_t *len, int64_t n, int stride, void *stream)
{
    if (!params || !state || !list || !len || n < 0 || stride < 1) return POMDP_E_BADARG;
    if (!history_ok(h, env == POMDP_ENV_ROCK) || (env == POMDP_ENV_ROCK && !belief_ok(b))) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_preferred<E>(p, state, b, h, list, len, n, stride, stream);
    });
}

int pomdp_pick_actions(const int32_t *list, const int32_t *len, int stride, int32_t *action, int64_t n, uint64_t seed,
                       uint32_t lane0, uint64_t t, void *stream)
{
    if (!list || !len || !action || stride < 1 || bad_range(n, lane0)) return POMDP_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(pick_actions_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, list, len, stride,
                       action, n, make_key(seed, t), lane0);
    return (int)hipGetLastError();
}

int pomdp_heuristic_steps(int env, const void *params, uint32_t *state, const pomdp_rock_belief *b, const pomdp_history *h,
                          int32_t *prev_ob, int32_t *action, int32_t *ob, void *reward, uint8_t *done,
                          const pomdp_returns *returns, int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0,
                          int64_t k_steps, int flags, void *stream)
{
    const int K = history_rocks(env, params);
    if (!heuristic_args_ok(K, params, state, b, h, prev_ob, action, ob, reward, done, returns, n, lane0, k_steps)) return POMDP_E_BADARG;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_heuristic_steps<E>(p, state, b, h, K, prev_ob, action, ob, reward, done, returns, n, seed, lane0, t0,
                                         k_steps, flags, stream);
    });
}

} // extern "C"
