// tree_keep_preferred.hip — the preferred-policy search resumed from kept trees (include/pomdp_hip.h:
// pomdp_tree_search_preferred_resume): tree_preferred_kernel's loop, private policy inputs and node priors on the pools of C
// nodes that tree_keep.hip resumes and pomdp_tree_advance copies.  A node receives its priors while its stored Nh is 0
// (tree_keep.hip.h: tree_node_priors_once), so a kept node is primed at most once, whichever search first stands on it.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
// A translation unit of its own: tree_search.hip, tree_search_preferred.hip and tree_keep.hip compile exactly as they did without it.
#include "kernels_common.hip.h"
#include "planner_common.hip.h"
#include "tree_keep.hip.h"

namespace pomdp {

int launch_tree_merge(const pomdp_tree_args *a, int n_act, void *stream);       // tree_search.hip

// tree_preferred_kernel (one lane per tree, wave-uniform (s, k), __any exit, the same STEP / ROLLOUT / TREE words, the private
// policy block copied as it stands there: planner_common.hip.h says why it is not factored) with tree_resume_kernel's three
// differences — the lane starts from the kept_nodes[i] nodes its pool holds, the pool has C nodes and a missing child in a full
// pool ends tree mode without a node, Nh is clamped to logn_len - 1 — and one rule of its own: node hn receives priors from
// this step's P(hn) when the lane is about to choose at it and its stored Nh is 0.  In tree mode the one read of the node word
// serves the test and the selection (tree_node_priors_once, tree_select_nh); at the step after a creation the lane knows the
// node is its own fresh one (`fresh`) and reads nothing.  A full pool creates nothing, so nothing is primed there.
template <class Env>
__global__ __launch_bounds__(BLOCK) void tree_resume_preferred_kernel(
    const typename Env::Params p, const uint32_t *__restrict__ state, int64_t n_cols, int n_particles, int64_t n_trees,
    int trees_per_root, int64_t n_roots, int64_t sims, int depth, double discount, double ucb_c, const double *__restrict__ logn,
    int32_t nh_max, void *__restrict__ workspace, int64_t capacity, int32_t *__restrict__ kept_nodes, pomdp_rock_belief b,
    pomdp_history h, const int32_t *__restrict__ prev_ob, int4 *ws_stat, double *ws_lkv, double *ws_lkw, int32_t prior_n,
    double prior_v, RngKey key0, uint32_t lane0, int32_t *__restrict__ tree_visits, double *__restrict__ tree_q,
    int32_t *__restrict__ n_nodes_out, int stride, double *__restrict__ sim_ret, int32_t *__restrict__ sim_steps,
    int32_t *__restrict__ sim_tree_steps)
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
    const TreeView tree = tree_keep_view(workspace, ic, n_act, capacity, depth);
    int32_t n_nodes = tree_keep_clamp_count(tree, kept_nodes[ic]);
    if (in_range && n_nodes < 1) {                           // an empty tree
        tree_fresh_node(tree, 0, 0, 0);
        n_nodes = 1;
    }
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
        bool fresh = false;                                  // node hn was created by the step before and has no priors yet
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
                // P(hn): the list this step's rollout pick would come from; the fallback's mask is built only where a node is primed
                uint32_t pm = m;
                const auto in_p = [&](int32_t act) {
                    if (!pm) for (int j = 0; j < count; ++j) pm |= 1u << (LegalOf<Env>::pick(sh, p, st, L, j) & 31);
                    return act < 32 && ((pm >> act) & 1u) != 0u;
                };
                if (!rolling) {
                    const int32_t nh = tree_node_priors_once(tree, hn, n_nodes, in_p, prior_n, prior_v);
                    a = tree_select_nh(tree, hn, nh, count, [&](int idx) { return LegalOf<Env>::pick(sh, p, st, L, idx); }, ucb_c, logn,
                                       nh_max);
                } else {
                    if (fresh) {
                        tree_node_priors(tree, hn, in_p, prior_n, prior_v);
                        fresh = false;
                    }
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
                        bool created, full;
                        hn = tree_child_or_full(tree, hn, a, o2, n_nodes, created, full);
                        if (created || full) k0 = k;         // full: the rollout starts here all the same, without a node
                        fresh = created && prior_n > 0;
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
        kept_nodes[i] = n_nodes;
    }
}

// tree_keep.hip's checks of a kept-tree descriptor, restated: that file is not edited and keeps them to itself
constexpr uint64_t TREE_KEEP_WORKSPACE_MAX = 1ull << 46;
static uint64_t keep_workspace_bytes(int n_act, int64_t n_trees, int64_t capacity, int depth)
{
    if (n_act < 1 || n_act > 255 || n_trees < 0 || n_trees > (1ll << 32) || capacity < 1 || depth < 0) return 0;
    if (capacity > 0x7FFFFFFFll || capacity * (int64_t)n_act > 0x7FFFFFFFll) return 0;    // edge indices are int32
    const unsigned __int128 total = (unsigned __int128)tree_keep_bytes(n_act, capacity, depth) * (unsigned __int128)n_trees;
    return total > TREE_KEEP_WORKSPACE_MAX ? 0 : (uint64_t)total;
}
static int keep_check(const pomdp_tree_keep *k, int n_act, int64_t n_trees, int depth)
{
    if (!k || !k->n_nodes || k->node_capacity < 1) return POMDP_E_BADARG;
    const uint64_t need = keep_workspace_bytes(n_act, n_trees, k->node_capacity, depth);
    if (n_trees > 0 && (need == 0 || !k->workspace || ((uintptr_t)k->workspace & 15u) || k->workspace_bytes < need)) return POMDP_E_BADARG;
    return 0;
}

} // namespace pomdp

extern "C" {

int pomdp_tree_search_preferred_resume(const pomdp_tree_args *a, const pomdp_tree_policy *pol, const pomdp_tree_keep *k, uint64_t t0,
                                       void *stream)
{
    if (!a || !a->params || !k || !pol) return POMDP_E_BADARG;
    if (pol->prior_n < 0 || pol->prior_n > 65535) return POMDP_E_BADARG;
    if (!(pol->prior_v >= -1.7976931348623157e308 && pol->prior_v <= 1.7976931348623157e308)) return POMDP_E_BADARG;   // NaN, +-inf
    const int policy = dispatch_env(a->env, a->params, [](auto tag, const auto &) {
        return (int)has_policy<typename decltype(tag)::Env>::value;
    });
    if (policy < 0) return policy;                                             // POMDP_E_BADPARAMS / unknown env
    if (!policy) {                                                             // the preferred list is the legal list
        if (pol->prior_n > 0) return POMDP_E_BADARG;                           // a uniform prior over it steers nothing
        return pomdp_tree_search_resume(a, k, t0, stream);
    }
    // pomdp_tree_search_resume's checks
    const int n_act = (int)env_action_count(a->env, a->params);
    const int64_t R = a->n_roots, W = a->trees_per_root, S = a->sims_per_tree;
    if (R < 0 || R > 0x7FFFFFFF || W < 1 || S < 1 || S > 0x7FFFFFFF || a->depth < 0 || (a->lane0 & 3u) || bad_range(R * W, a->lane0) ||
        W * S > 0x7FFFFFFFll)
        return POMDP_E_BADARG;
    if (!plan_out_ok(&a->out, n_act)) return POMDP_E_BADARG;                  // NULL q / visits / best, A > 255, stride < A
    if (!a->tree_visits || !a->tree_q || !a->n_nodes || !a->logn) return POMDP_E_BADARG;
    if (!(a->ucb_c >= 0.0) || a->ucb_c > 1.7976931348623157e308) return POMDP_E_BADARG;   // negative, NaN or infinite
    if (a->particles) {
        const int P = a->n_particles;
        if (P < 4 || P > 4096 || (P & 3) || R * (int64_t)P > (1ll << 32)) return POMDP_E_BADARG;
    } else if (a->n_particles != 0 || !a->root_state) return POMDP_E_BADARG;
    if (k->logn_len < 2 || k->logn_len - 1 > 0x7FFFFFFFll || W * (k->logn_len - 1) > 0x7FFFFFFFll) return POMDP_E_BADARG;   // merged visits are int32
    if (k->logn_len - 1 < (int64_t)n_act * pol->prior_n + 1) return POMDP_E_BADARG;       // a primed node's Nh must index the table
    const int rk = keep_check(k, n_act, R * W, a->depth);
    if (rk) return rk;
    // pomdp_tree_search_preferred's checks of pol
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
            hipLaunchKernelGGL(tree_resume_preferred_kernel<E>, dim3(blocks_for(R * W)), dim3(BLOCK), 0, (hipStream_t)stream, p,
                               a->particles ? a->particles : a->root_state, P ? R * P : R, P, R * W, (int)W, R, S, a->depth,
                               a->discount, a->ucb_c, a->logn, (int32_t)(k->logn_len - 1), k->workspace, k->node_capacity, k->n_nodes,
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
