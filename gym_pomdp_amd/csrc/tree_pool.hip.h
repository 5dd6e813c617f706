// tree_pool.hip.h — the node pool of one search tree (include/pomdp_hip.h: pomdp_tree_search): UCB1 selection, child lookup /
// insert, the path stack and the backup.  __host__ __device__ and free of device builtins, so that the same text runs inside
// the search kernels (tree_search.hip, tree_search_preferred.hip) and in a stand-alone host program (which is how its bounds
// were checked before it first ran on a GPU).
//
// Layout: a tree owns three consecutive arrays of the caller's workspace,
//   edge [S + 1][A]   16 B   {V(h,a) double, N(h,a) int32, first child of (h,a) int32}: what selection reads per legal action is ONE
//                            16-byte load, and a node's A entries share A / 8 cache lines;
//   node [S + 1]      16 B   {observation, next sibling — the next child of the same (h,a) —, visits Nh = sum_a N(h,a), unused};
//   path [min(D, S)]  16 B   {reward double, node, action}: the in-tree steps of the running simulation.
// Node 0 is the root and is never a child, so 0 ends a sibling chain.  A node's edges are cleared when the node is created, by
// the lane that owns the tree: the workspace needs no initialisation, and a search starts from an empty tree by resetting node 0.
// Bounds, by construction and enforced again at every index: a simulation creates at most one node, so n_nodes <= s + 1 <= S
// before the insert of simulation s < S and every node index is <= S; the in-tree steps of simulation s walk a chain of
// existing nodes (at most s of them below the root) and are steps of the simulation (fewer than D), so the path holds fewer than
// min(D, S) entries before a push.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define POMDP_TREE_HD __host__ __device__ __forceinline__
#else
#define POMDP_TREE_HD inline
#endif

namespace pomdp {

struct alignas(16) TreeEdge { double v; int32_t n; int32_t child; };
struct alignas(16) TreeNode { int32_t ob; int32_t next; int32_t visits; int32_t unused; };
struct alignas(16) TreePath { double r; int32_t h; int32_t a; };

struct TreeDims {
    int32_t A, S, Dp;                                        // actions; simulations (node capacity S + 1); path capacity min(D, S)
};
static POMDP_TREE_HD int32_t tree_path_cap(int64_t S, int depth) { return (int32_t)(S < (int64_t)depth ? S : (int64_t)depth); }
// bytes of one tree; the caller has checked (S + 1) * A < 2^31
static POMDP_TREE_HD uint64_t tree_bytes(int32_t A, int64_t S, int depth)
{
    return 16ull * ((uint64_t)(S + 1) * (uint64_t)A + (uint64_t)(S + 1) + (uint64_t)tree_path_cap(S, depth));
}

struct TreeView {                                            // one tree's slices of the workspace
    TreeEdge *edge;
    TreeNode *node;
    TreePath *path;
    TreeDims d;
};
static POMDP_TREE_HD TreeView tree_view(void *workspace, int64_t tree, int32_t A, int64_t S, int depth)
{
    TreeView t;
    char *base = (char *)workspace + (uint64_t)tree * tree_bytes(A, S, depth);
    t.edge = (TreeEdge *)base;
    t.node = (TreeNode *)(t.edge + (uint64_t)(S + 1) * (uint64_t)A);
    t.path = (TreePath *)(t.node + (S + 1));
    t.d.A = A; t.d.S = (int32_t)S; t.d.Dp = tree_path_cap(S, depth);
    return t;
}

static POMDP_TREE_HD int32_t tree_clamp_node(const TreeView &t, int32_t h) { return h < 0 ? 0 : (h > t.d.S ? t.d.S : h); }
static POMDP_TREE_HD int64_t tree_edge_index(const TreeView &t, int32_t h, int32_t a)
{
    const int32_t ac = a < 0 ? 0 : (a >= t.d.A ? t.d.A - 1 : a);
    return (int64_t)tree_clamp_node(t, h) * t.d.A + ac;
}

// a new node: N = V = 0 and no child for every action
static POMDP_TREE_HD void tree_fresh_node(const TreeView &t, int32_t h, int32_t ob, int32_t next)
{
    const int32_t hc = tree_clamp_node(t, h);
    TreeNode nd; nd.ob = ob; nd.next = next; nd.visits = 0; nd.unused = 0;
    t.node[hc] = nd;
    TreeEdge e; e.v = 0.0; e.n = 0; e.child = 0;
    for (int32_t a = 0; a < t.d.A; ++a) t.edge[(int64_t)hc * t.d.A + a] = e;
}

// Selection at node h over the legal list (count entries, pick(i) its i-th): the first entry with N == 0, else the first
// maximum of V + c * sqrt(logn[Nh] / N) — one division, one square root, one multiply, one add, none fused.  logn has
// nh_max + 1 entries: S + 1 for a search without priors, S + 1 + A * prior_n with them (tree_node_priors).
template <class Pick>
static POMDP_TREE_HD int32_t tree_select_clamped(const TreeView &t, int32_t h, int count, Pick pick, double ucb_c, const double *logn,
                                                 int32_t nh_max)
{
#pragma clang fp contract(off)
    const int32_t hc = tree_clamp_node(t, h);
    int32_t nh = t.node[hc].visits;
    nh = nh < 0 ? 0 : (nh > nh_max ? nh_max : nh);
    const double ln = logn[nh];
    int32_t fresh = -1, best = -1;
    double bu = 0.0;
    for (int i = 0; i < count; ++i) {
        const int32_t a = pick(i);
        const TreeEdge e = t.edge[tree_edge_index(t, hc, a)];
        if (e.n == 0) {
            if (fresh < 0) fresh = a;
        } else {
            const double ratio = ln / (double)e.n;
            const double root = __builtin_sqrt(ratio);
            const double bonus = ucb_c * root;
            const double u = e.v + bonus;
            if (best < 0 || u > bu) { best = a; bu = u; }
        }
    }
    return fresh >= 0 ? fresh : best;
}
template <class Pick>
static POMDP_TREE_HD int32_t tree_select(const TreeView &t, int32_t h, int count, Pick pick, double ucb_c, const double *logn)
{
    return tree_select_clamped(t, h, count, pick, ucb_c, logn, t.d.S);   // logn has S + 1 entries
}

// Node priors (pomdp_tree_search_preferred), the second half of a node's creation where the search sets them: the edges of
// node h start at N = prior_n, V = prior_v for the actions a with
// in(a) and at N = V = 0 for the others, no child anywhere, and the node's visits at prior_n * |{a : in(a)}| (prior_n <=
// 65535 and A <= 255: below 2^24).  For a node that has no child yet: the node created last, or node 0 of an empty tree.
// Stores only — the node's observation and sibling link stay as its creation wrote them.
template <class In>
static POMDP_TREE_HD void tree_node_priors(const TreeView &t, int32_t h, In in, int32_t prior_n, double prior_v)
{
    const int32_t hc = tree_clamp_node(t, h);
    const int32_t pn = prior_n < 0 ? 0 : (prior_n > 65535 ? 65535 : prior_n);
    int32_t listed = 0;
    for (int32_t a = 0; a < t.d.A; ++a) {
        const bool on = in(a);
        TreeEdge e; e.v = on ? prior_v : 0.0; e.n = on ? pn : 0; e.child = 0;
        t.edge[(int64_t)hc * t.d.A + a] = e;
        listed += (int32_t)on;
    }
    t.node[hc].visits = pn * listed;
}
// the child of (h, a) under observation ob; created — as node n_nodes, whatever depth remains — when there is none.
// -> its index; `created` tells which.  A full pool (impossible: one insert per simulation) hands back the root.
static POMDP_TREE_HD int32_t tree_child(const TreeView &t, int32_t h, int32_t a, int32_t ob, int32_t &n_nodes, bool &created)
{
    const int64_t ei = tree_edge_index(t, h, a);
    const int32_t first = t.edge[ei].child;
    int32_t c = first;
    created = false;
    for (int32_t guard = 0; c > 0 && c <= t.d.S && guard <= t.d.S; ++guard) {
        const TreeNode nd = t.node[c];
        if (nd.ob == ob) return c;
        c = nd.next;
    }
    if (n_nodes < 1 || n_nodes > t.d.S) return 0;
    const int32_t fresh = n_nodes++;
    tree_fresh_node(t, fresh, ob, first);
    t.edge[ei].child = fresh;
    created = true;
    return fresh;
}

static POMDP_TREE_HD void tree_push(const TreeView &t, int32_t &plen, int32_t h, int32_t a, double r)
{
    if (plen < 0 || plen >= t.d.Dp) return;
    TreePath e; e.r = r; e.h = h; e.a = a;
    t.path[plen++] = e;
}

// the backup of one simulation, deepest entry first: Rt = r + discount * Rt; N += 1; V += (Rt - V) / N.  -> the final Rt
static POMDP_TREE_HD double tree_backup(const TreeView &t, int32_t plen, double acc, double discount)
{
#pragma clang fp contract(off)
    double rt = acc;
    if (plen > t.d.Dp) plen = t.d.Dp;
    for (int32_t j = plen - 1; j >= 0; --j) {
        const TreePath pe = t.path[j];
        const double tail = discount * rt;
        rt = pe.r + tail;
        const int64_t ei = tree_edge_index(t, pe.h, pe.a);
        TreeEdge e = t.edge[ei];
        e.n += 1;
        const double diff = rt - e.v;
        const double inc = diff / (double)e.n;
        e.v = e.v + inc;
        t.edge[ei] = e;
        t.node[tree_clamp_node(t, pe.h)].visits += 1;
    }
    return rt;
}

} // namespace pomdp
