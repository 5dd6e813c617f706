// tree_keep.hip — trees kept between searches (include/pomdp_hip.h: pomdp_tree_search_resume, pomdp_tree_advance): the search of
// tree_search.hip resumed from the nodes a caller's workspace holds, in pools of C nodes that do fill up, and the copy of the
// subtree under the real step's (action, observation) into a second workspace.  One lane per tree in both kernels; the pool
// code is tree_pool.hip.h's and tree_keep.hip.h's.  tree_search.hip and tree_search_preferred.hip are not touched by it.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "kernels_common.hip.h"
#include "planner_common.hip.h"
#include "tree_keep.hip.h"

namespace pomdp {

int launch_tree_merge(const pomdp_tree_args *a, int n_act, void *stream);       // tree_search.hip

// tree_search_kernel's loop — the same lanes, the same wave-uniform (s, k), the same STEP / ROLLOUT / TREE words — with three
// differences: the lane starts from the n_nodes[i] nodes its pool holds (an empty tree clears node 0), the pool has C nodes and
// a missing child in a full pool ends tree mode without a node, and Nh is clamped to the caller's logn_len - 1.
template <class Env>
__global__ __launch_bounds__(BLOCK) void tree_resume_kernel(const typename Env::Params p, const uint32_t *__restrict__ state,
                                                            int64_t n_cols, int n_particles, int64_t n_trees, int trees_per_root,
                                                            int64_t sims, int depth, double discount, double ucb_c,
                                                            const double *__restrict__ logn, int32_t nh_max,
                                                            void *__restrict__ workspace, int64_t capacity,
                                                            int32_t *__restrict__ kept_nodes, RngKey key0, uint32_t lane0,
                                                            int32_t *__restrict__ tree_visits, double *__restrict__ tree_q,
                                                            int32_t *__restrict__ n_nodes_out, int stride,
                                                            double *__restrict__ sim_ret, int32_t *__restrict__ sim_steps,
                                                            int32_t *__restrict__ sim_tree_steps)
{
#pragma clang fp contract(off)
    __shared__ typename Env::Shared sh;
    Env::stage(sh, p, (int)threadIdx.x);
    __syncthreads();
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
        double acc = 0.0, disc = 1.0;
        int32_t h = 0, plen = 0;
        int k = 0, d = 0, k0 = -1;                           // k0 < 0: still in the tree
        uint4 pw = make_uint4(0, 0, 0, 0);
        bool active = in_range;
#pragma unroll 1
        for (int step = 0; step < depth; ++step) {
            const auto L = LegalOf<Env>::make(sh, p, st, false);
            const int count = L.count;
            active = active && !d && count > 0;
            if (!__any(active)) break;                       // wave-uniform exit
            int a = 0;
            if (active) {
                if (k0 < 0) {
                    a = tree_select_clamped(tree, h, count, [&](int idx) { return LegalOf<Env>::pick(sh, p, st, L, idx); }, ucb_c, logn,
                                            nh_max);
                } else {
                    const int j = step - k0;
                    if ((j & 3) == 0) pw = stream_block(key_at(key0, ts + (uint64_t)k0), lane, POMDP_STREAM_ROLLOUT, (uint32_t)(j >> 2));
                    const uint32_t w = (j & 3) == 0 ? pw.x : (j & 3) == 1 ? pw.y : (j & 3) == 2 ? pw.z : pw.w;
                    a = LegalOf<Env>::pick(sh, p, st, L, (int)__umulhi(w, (uint32_t)count));
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
                    tree_push(tree, plen, h, a, r);
                    if (!d) {
                        bool created, full;
                        h = tree_child_or_full(tree, h, a, o2, n_nodes, created, full);
                        if (created || full) k0 = k;         // full: the rollout starts here all the same, without a node
                    }
                } else {
                    const double term = disc * r;
                    acc = acc + term;
                    disc = disc * discount;
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

// Lane i copies what tree i keeps after the real step of its root (tree_keep_copy) from src to dst: one lane per tree, each
// writing only its own pool and its own count; no atomics.
__global__ __launch_bounds__(BLOCK) void tree_advance_kernel(int n_act, int64_t capacity, int depth, int64_t n_trees, int trees_per_root,
                                                             void *__restrict__ src_ws, const int32_t *__restrict__ src_nodes,
                                                             void *__restrict__ dst_ws, int32_t *__restrict__ dst_nodes,
                                                             const int32_t *__restrict__ action, const int32_t *__restrict__ ob,
                                                             const uint8_t *__restrict__ drop)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_trees) return;
    const int64_t r = i / trees_per_root;
    int32_t kept = 0;
    if (!(drop && drop[r])) {
        const TreeView src = tree_keep_view(src_ws, i, n_act, capacity, depth);
        const TreeView dst = tree_keep_view(dst_ws, i, n_act, capacity, depth);
        kept = tree_keep_copy(src, src_nodes[i], dst, action[r], ob[r]);
    }
    dst_nodes[i] = kept;
}

constexpr uint64_t TREE_KEEP_WORKSPACE_MAX = 1ull << 46;     // refuse sizes no device holds instead of overflowing

// bytes of workspace, 0 where the shape is refused; n_act: the env's action count
static uint64_t tree_keep_workspace_bytes(int n_act, int64_t n_trees, int64_t capacity, int depth)
{
    if (n_act < 1 || n_act > 255 || n_trees < 0 || n_trees > (1ll << 32) || capacity < 1 || depth < 0) return 0;
    if (capacity > 0x7FFFFFFFll || capacity * (int64_t)n_act > 0x7FFFFFFFll) return 0;    // edge indices are int32
    const unsigned __int128 total = (unsigned __int128)tree_keep_bytes(n_act, capacity, depth) * (unsigned __int128)n_trees;
    return total > TREE_KEEP_WORKSPACE_MAX ? 0 : (uint64_t)total;
}

// a kept-tree descriptor against the shape it is used with: -> 0 or POMDP_E_BADARG
static int tree_keep_check(const pomdp_tree_keep *k, int n_act, int64_t n_trees, int depth)
{
    if (!k || !k->n_nodes || k->node_capacity < 1) return POMDP_E_BADARG;
    const uint64_t need = tree_keep_workspace_bytes(n_act, n_trees, k->node_capacity, depth);
    if (n_trees > 0 && (need == 0 || !k->workspace || ((uintptr_t)k->workspace & 15u) || k->workspace_bytes < need)) return POMDP_E_BADARG;
    return 0;
}

static bool ranges_overlap(const void *a, uint64_t na, const void *b, uint64_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

} // namespace pomdp

extern "C" {

size_t pomdp_tree_keep_workspace(int env, const void *params, int64_t n_trees, int64_t node_capacity, int depth)
{
    if (!params || dispatch_env(env, params, [](auto, const auto &) { return 0; })) return 0;
    return (size_t)tree_keep_workspace_bytes((int)env_action_count(env, params), n_trees, node_capacity, depth);
}

int pomdp_tree_search_resume(const pomdp_tree_args *a, const pomdp_tree_keep *k, uint64_t t0, void *stream)
{
    // pomdp_tree_search's checks, without its workspace's (a->workspace is ignored) and its pool's (S + 1) * A bound
    if (!a || !a->params || !k) return POMDP_E_BADARG;
    const int rc = dispatch_env(a->env, a->params, [](auto, const auto &) { return 0; });   // POMDP_E_BADPARAMS / unknown env
    if (rc) return rc;
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
    const int rk = tree_keep_check(k, n_act, R * W, a->depth);
    if (rk) return rk;
    if (R == 0) return 0;
    const int r2 = dispatch_env(a->env, a->params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        const int P = a->particles ? a->n_particles : 0;
        hipLaunchKernelGGL(tree_resume_kernel<E>, dim3(blocks_for(R * W)), dim3(BLOCK), 0, (hipStream_t)stream, p,
                           a->particles ? a->particles : a->root_state, P ? R * P : R, P, R * W, (int)W, S, a->depth, a->discount,
                           a->ucb_c, a->logn, (int32_t)(k->logn_len - 1), k->workspace, k->node_capacity, k->n_nodes,
                           make_key(a->seed, t0), a->lane0, a->tree_visits, a->tree_q, a->n_nodes, (int)a->out.stride, a->sim_ret,
                           a->sim_steps, a->sim_tree_steps);
        return (int)hipGetLastError();
    });
    if (r2) return r2;
    return launch_tree_merge(a, n_act, stream);
}

int pomdp_tree_advance(int env, const void *params, int64_t n_roots, int trees_per_root, int depth, const pomdp_tree_keep *src,
                       const pomdp_tree_keep *dst, const int32_t *action, const int32_t *ob, const uint8_t *drop, void *stream)
{
    if (!params || !src || !dst || !action || !ob) return POMDP_E_BADARG;
    const int rc = dispatch_env(env, params, [](auto, const auto &) { return 0; });
    if (rc) return rc;
    const int n_act = (int)env_action_count(env, params);
    const int64_t R = n_roots, W = trees_per_root;
    if (n_act < 1 || n_act > 255 || R < 0 || R > 0x7FFFFFFF || W < 1 || depth < 0 || R * W > (1ll << 32)) return POMDP_E_BADARG;
    const int64_t n = R * W;
    if (tree_keep_check(src, n_act, n, depth) || tree_keep_check(dst, n_act, n, depth)) return POMDP_E_BADARG;
    if (src == dst || src->node_capacity != dst->node_capacity) return POMDP_E_BADARG;
    const uint64_t need = tree_keep_workspace_bytes(n_act, n, src->node_capacity, depth);
    if (n > 0 && (ranges_overlap(src->workspace, need, dst->workspace, need) ||
                  ranges_overlap(src->n_nodes, 4ull * (uint64_t)n, dst->n_nodes, 4ull * (uint64_t)n)))
        return POMDP_E_BADARG;
    if (R == 0) return 0;
    hipLaunchKernelGGL(tree_advance_kernel, dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, n_act, src->node_capacity, depth, n,
                       (int)W, src->workspace, (const int32_t *)src->n_nodes, dst->workspace, dst->n_nodes, action, ob, drop);
    return (int)hipGetLastError();
}

} // extern "C"
