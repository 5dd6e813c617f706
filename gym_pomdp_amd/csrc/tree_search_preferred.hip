// tree_search_preferred.hip — POMCP's search with the env's preferred-action policy (include/pomdp_hip.h:
// pomdp_tree_search_preferred): tree_search_kernel's trees, lanes, words and backup, with rollouts that pick from
// _generate_preferred(history) and new nodes that start their preferred actions with a count and a value.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
// A translation unit of its own: tree_search.hip compiles exactly as it did without this file.
#include "kernels_common.hip.h"
#include "planner_common.hip.h"
#include "tree_pool.hip.h"

namespace pomdp {

int tree_check_args(const pomdp_tree_args *a, int *n_act_out);                 // tree_search.hip
int launch_tree_merge(const pomdp_tree_args *a, int n_act, void *stream);

// tree_search_kernel (one lane per tree, wave-uniform (s, k), __any exit) joined with rollout_preferred_kernel's private policy
// inputs.  At the start of every simulation the lane takes root r's words — size, last action / observation and, for
// RockSample, check_ok / move_ok / prev_ob — into registers and clears `touched`; after every executed step, in the tree and in
// the rollout alike, it updates them as a simulation of pomdp_rollout_preferred does.  The per-rock entries a CHECK changes live
// in the policy workspace, one slot per (rock, tree), copy on first touch: bit j of `touched` says that THIS simulation owns
// slot (j, tree); while it is clear a CHECK of rock j reads root r's entry, whatever an earlier simulation left in the slot.
// A lane reads only what it wrote itself, in program order: plain loads and stores, no fence.
// Env::preferred_mask runs once per step.  In rollout mode it is the list to pick from (the legal list where it is empty); at
// the step after a node's creation — and at step 0 of simulation 0 for node 0 — the same mask gives the node its priors
// before the pick.  Tree-mode selection scans the legal list, as tree_search_kernel's.
template <class Env>
__global__ __launch_bounds__(BLOCK) void tree_preferred_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                               int64_t n_cols, int n_particles, int64_t n_trees, int trees_per_root,
                                                               int64_t n_roots, int64_t sims, int depth, double discount, double ucb_c,
                                                               const double *__restrict__ logn, int32_t nh_max,
                                                               void *__restrict__ workspace, pomdp_rock_belief b, pomdp_history h,
                                                               const int32_t *__restrict__ prev_ob, int4 *ws_stat, double *ws_lkv,
                                                               double *ws_lkw, int32_t prior_n, double prior_v, RngKey key0,
                                                               uint32_t lane0, int32_t *__restrict__ tree_visits,
                                                               double *__restrict__ tree_q, int32_t *__restrict__ n_nodes_out,
                                                               int stride, double *__restrict__ sim_ret,
                                                               int32_t *__restrict__ sim_steps, int32_t *__restrict__ sim_tree_steps)
{
#pragma clang fp contract(off)
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    stage_policy_tables<Env>(sh, p);
    __syncthreads();
    const int K = rock_count(p);
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in_range = i < n_trees;
    const int64_t ic = in_range ? i : n_trees - 1;
    const uint32_t lane = lane0 + (uint32_t)i;
    const int64_t root = ic / trees_per_root;
    const int n_act = Env::n_actions(p);
    const TreeView tree = tree_view(workspace, ic, n_act, sims, depth);
    int32_t n_nodes = 1;
    if (in_range) tree_fresh_node(tree, 0, 0, 0);            // every search starts from an empty tree
    const uint64_t t0 = ((uint64_t)key0.t_hi << 32) | key0.t_lo;
#pragma unroll 1
    for (int64_t s = 0; s < sims; ++s) {
        const uint64_t ts = t0 + (uint64_t)s * (uint64_t)depth;
        int64_t col = root;
        if (n_particles > 0) {
            const uint32_t x = stream_block(key_at(key0, ts), lane, POMDP_STREAM_TREE, 0u).x;
            col = root * n_particles + (int64_t)__umulhi(x, (uint32_t)n_particles);
        }
        typename Env::State st;
        Env::load(st, state, n_cols, (uint32_t)col);
        // root r's policy inputs, private from here on; the touched set starts empty
        int hsize = h.size[root], la = h.last_action[root], lo = h.last_ob[root], pob = 0;
        uint32_t ck = 0, mv = 0, touched = 0;
        if constexpr (Env::HAS_ROCKS) { ck = b.check_ok[root]; mv = h.move_ok[root]; pob = prev_ob[root]; }
        double acc = 0.0, disc = 1.0;
        int32_t hn = 0, plen = 0;
        int k = 0, d = 0, k0 = -1;                           // k0 < 0: still in the tree
        uint4 pw = make_uint4(0, 0, 0, 0);
        bool active = in_range;
        bool unprimed = prior_n > 0 && s == 0;               // node hn has no priors yet: node 0 now, later the node created last
#pragma unroll 1
        for (int step = 0; step < depth; ++step) {
            // _generate_preferred(history) on the private inputs; the legal list for the tree's scan and for the fallback
            const uint32_t m = Env::preferred_mask(sh, p, st, h, n_roots, (uint32_t)root, ck, mv, hsize, la, lo);
            const bool rolling = k0 >= 0;
            const auto L = LegalOf<Env>::make(sh, p, st, rolling && m != 0u);
            const int count = (rolling && m) ? __popc(m) : L.count;
            active = active && !d && count > 0;
            if (!__any(active)) break;                       // wave-uniform exit
            int a = 0;
            if (active) {
                if (unprimed) {                              // P(h): the list this step's rollout pick would come from
                    uint32_t pm = m;
                    if (!pm) for (int j = 0; j < count; ++j) pm |= 1u << (LegalOf<Env>::pick(sh, p, st, L, j) & 31);
                    tree_node_priors(tree, hn, [&](int32_t act) { return act < 32 && ((pm >> act) & 1u) != 0u; }, prior_n, prior_v);
                    unprimed = false;
                }
                if (!rolling) {
                    a = tree_select_clamped(tree, hn, count, [&](int idx) { return LegalOf<Env>::pick(sh, p, st, L, idx); }, ucb_c,
                                            logn, nh_max);
                } else {
                    const int j = step - k0;
                    if ((j & 3) == 0) pw = stream_block(key_at(key0, ts + (uint64_t)k0), lane, POMDP_STREAM_ROLLOUT, (uint32_t)(j >> 2));
                    const uint32_t w = (j & 3) == 0 ? pw.x : (j & 3) == 1 ? pw.y : (j & 3) == 2 ? pw.z : pw.w;
                    const int idx = (int)__umulhi(w, (uint32_t)count);
                    a = m ? nth_set_bit(m, idx) : LegalOf<Env>::pick(sh, p, st, L, idx);
                }
            }
            const RngKey key = key_at(key0, ts + (uint64_t)step);
            typename Env::State nx = st;
            int o2, d2;
            typename Env::Reward rw;                         // the reward as pomdp_<env>_step writes it, then (double)
            Env::step(sh, p, nx, a, key, lane, o2, rw, d2);
            const double r = (double)rw;
            if (active) {
                st = nx; d = d2;
                k = step + 1;
                if (k0 < 0) {
                    tree_push(tree, plen, hn, a, r);
                    if (!d) {
                        bool created;
                        hn = tree_child(tree, hn, a, o2, n_nodes, created);
                        if (created) { k0 = k; unprimed = prior_n > 0; }
                    }
                } else {
                    const double term = disc * r;
                    acc = acc + term;
                    disc = disc * discount;
                }
                // history.append(Transition(prev_ob, a, r, o2, d2)) and the side statistics, on the lane's own copies
                la = a; lo = o2;
                hsize += (int)(hsize != 0x7FFFFFFF);
                if constexpr (Env::HAS_ROCKS) {
                    if (a >= 5 && a < 5 + K) {                           // an executed CHECK of rock j
                        const int j = a - 5;
                        const uint32_t bit = 1u << j;
                        const int64_t kr = (int64_t)j * n_roots + root, ks = (int64_t)j * n_trees + ic;
                        int cnt, meas, tsum, tmov;
                        double lkv, lkw;
                        if (touched & bit) {
                            const int4 v = ws_stat[ks];
                            cnt = v.x; meas = v.y; tsum = v.z; tmov = v.w;
                            lkv = ws_lkv[ks]; lkw = ws_lkw[ks];
                        } else {
                            cnt = b.count[kr]; meas = b.measured[kr]; tsum = h.total_sample[kr]; tmov = h.total_move[kr];
                            lkv = b.lkv[kr]; lkw = b.lkw[kr];
                        }
                        // the history's two sums and Env::belief_update, on the private entry
                        const int ds = check_ds(o2), dm = check_dm(o2, pob == 1);
                        if (ds) { tsum += ds; mv = with_bit(mv, bit << 16, tsum > 0); }
                        if (dm) { tmov += dm; mv = with_bit(mv, bit, tmov >= 0); }
                        if (o2 != 0 && !d2) {                            // CHECK does not move: st is where the reading was taken
                            const auto u = Env::check_update(Env::sensor_eff(sh, p, st, j & 15), o2, lkv, cnt, lkw);
                            meas += 1; cnt = u.count; lkv = u.lkv; lkw = u.lkw;
                            ck = with_bit(ck, bit, Env::check_ok(meas, cnt, u.pv));
                        }
                        ws_stat[ks] = make_int4(cnt, meas, tsum, tmov);
                        ws_lkv[ks] = lkv; ws_lkw[ks] = lkw;
                        touched |= bit;
                    }
                    pob = o2;
                }
            }
        }
        if (in_range) {
            const double rt = tree_backup(tree, plen, acc, discount);
            if (sim_ret) sim_ret[s * n_trees + i] = rt;      // kernel arguments: wave-uniform
            if (sim_steps) sim_steps[s * n_trees + i] = k;
            if (sim_tree_steps) sim_tree_steps[s * n_trees + i] = plen;
        }
    }
    if (in_range) {
        for (int a = 0; a < n_act; ++a) {
            const TreeEdge e = tree.edge[a];
            tree_visits[i * stride + a] = e.n;
            tree_q[i * stride + a] = e.v;
        }
        n_nodes_out[i] = n_nodes;
    }
}

} // namespace pomdp

extern "C" {

size_t pomdp_tree_search_preferred_workspace(int env, const void *params, int64_t n_trees)
{
    if (env != POMDP_ENV_ROCK || !params || n_trees < 0 || n_trees > (1ll << 32)) return 0;
    return (size_t)(32ull * (uint64_t)((const pomdp_rock_params *)params)->num_rocks * (uint64_t)n_trees);
}

int pomdp_tree_search_preferred(const pomdp_tree_args *a, const pomdp_tree_policy *pol, uint64_t t0, void *stream)
{
    int n_act = 0;
    const int rc = tree_check_args(a, &n_act);
    if (rc) return rc;
    if (!pol || pol->prior_n < 0 || pol->prior_n > 65535) return POMDP_E_BADARG;
    if (!(pol->prior_v >= -1.7976931348623157e308 && pol->prior_v <= 1.7976931348623157e308)) return POMDP_E_BADARG;   // NaN, +-inf
    const int64_t R = a->n_roots, W = a->trees_per_root, S = a->sims_per_tree;
    const int64_t nh_max = S + (int64_t)n_act * pol->prior_n;                   // logn has nh_max + 1 entries
    if (W * nh_max > 0x7FFFFFFFll) return POMDP_E_BADARG;                      // merged visit counts are int32
    const bool policy = dispatch_env(a->env, a->params, [](auto tag, const auto &) {
        return (int)has_policy<typename decltype(tag)::Env>::value;
    }) != 0;
    if (!policy) {                                                             // the preferred list is the legal list
        if (pol->prior_n > 0) return POMDP_E_BADARG;                           // a uniform prior over it steers nothing
        return pomdp_tree_search(a, t0, stream);
    }
    const bool rock = a->env == POMDP_ENV_ROCK;
    if (!history_ok(pol->history, rock) || pol->history->max_size != -1) return POMDP_E_BADARG;
    const uint64_t need = pomdp_tree_search_preferred_workspace(a->env, a->params, R * W);
    if (rock && (!belief_ok(pol->belief) || !pol->prev_ob)) return POMDP_E_BADARG;
    if (rock && R > 0 && (!pol->workspace || ((uintptr_t)pol->workspace & 15u) || pol->workspace_bytes < need)) return POMDP_E_BADARG;
    if (R == 0) return 0;
    const int r2 = dispatch_env(a->env, a->params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        if constexpr (has_policy<E>::value) {
            const int P = a->particles ? a->n_particles : 0;
            const int64_t cells = E::HAS_ROCKS ? R * W * rock_count(p) : 0;    // policy workspace: int4 [K][n], then lkv, lkw double [K][n]
            int4 *const ws_stat = (int4 *)pol->workspace;
            double *const ws_lkv = (double *)(ws_stat + cells);
            hipLaunchKernelGGL(tree_preferred_kernel<E>, dim3(blocks_for(R * W)), dim3(BLOCK), 0, (hipStream_t)stream, p,
                               a->particles ? a->particles : a->root_state, P ? R * P : R, P, R * W, (int)W, R, S, a->depth,
                               a->discount, a->ucb_c, a->logn, (int32_t)nh_max, a->workspace,
                               (E::HAS_ROCKS && pol->belief) ? *pol->belief : NO_BELIEF, *pol->history, pol->prev_ob, ws_stat, ws_lkv,
                               ws_lkv + cells, pol->prior_n, pol->prior_v, make_key(a->seed, t0), a->lane0, a->tree_visits, a->tree_q,
                               a->n_nodes, (int)a->out.stride, a->sim_ret, a->sim_steps, a->sim_tree_steps);
            return (int)hipGetLastError();
        } else {
            return POMDP_E_BADARG;
        }
    });
    if (r2) return r2;
    return launch_tree_merge(a, n_act, stream);
}

} // extern "C"
