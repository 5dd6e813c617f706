// tree_keep.hip.h — what a tree kept between searches adds to the node pool of tree_pool.hip.h (include/pomdp_hip.h:
// pomdp_tree_search_resume, pomdp_tree_advance): the layout of a pool of C nodes, a child lookup / insert that reports a full
// pool, and the copy of the subtree under one child of the root into another pool.  __host__ __device__ and free of device
// builtins like tree_pool.hip.h, so that the same text runs in the kernels (tree_keep.hip, tree_keep_preferred.hip) and in
// stand-alone host programs (tools/tree_keep_hostcheck.cpp, tools/tree_keep_preferred_hostcheck.cpp, built with the host
// sanitizers).  At its end: what the preferred-policy search needs on such a pool, priors for a node that may have them.
//
// Layout: tree_pool.hip.h's three arrays with a node capacity C that no longer follows from the simulation count,
//   edge [C][A], node [C], path [min(D, C)].
// A TreeView of it carries d.S = C - 1 (the largest node index) and d.Dp = min(D, C), so that every clamp of tree_pool.hip.h
// holds unchanged.
// Bounds, by construction and enforced again at every index: a resumed search creates a node only while n_nodes < C, so every
// node index is <= C - 1; the in-tree steps of a simulation are pushed at existing nodes, each the child of the one before
// (at most C of them, the root included), and are steps of the simulation (at most D), so the path holds fewer than
// min(D, C) entries before a push — a full pool ends tree mode at the step that finds it, after that step's push.
// The copy reads a source pool whose contents it does not trust: every index read from memory is clamped to the source's
// n_nodes before use, a sibling chain is followed only while the destination has room, and every followed link creates one
// destination node — at most C of them — so the copy ends after at most C * A edge copies and C node copies whatever the source holds.
#pragma once
#include "tree_pool.hip.h"

namespace pomdp {

static POMDP_TREE_HD int32_t tree_keep_path_cap(int64_t C, int depth) { return (int32_t)(C < (int64_t)depth ? C : (int64_t)depth); }
// bytes of one kept tree; the caller has checked C >= 1 and C * A < 2^31
static POMDP_TREE_HD uint64_t tree_keep_bytes(int32_t A, int64_t C, int depth)
{
    return 16ull * ((uint64_t)C * (uint64_t)A + (uint64_t)C + (uint64_t)tree_keep_path_cap(C, depth));
}
static POMDP_TREE_HD TreeView tree_keep_view(void *workspace, int64_t tree, int32_t A, int64_t C, int depth)
{
    TreeView t;
    char *base = (char *)workspace + (uint64_t)tree * tree_keep_bytes(A, C, depth);
    t.edge = (TreeEdge *)base;
    t.node = (TreeNode *)(t.edge + (uint64_t)C * (uint64_t)A);
    t.path = (TreePath *)(t.node + C);
    t.d.A = A; t.d.S = (int32_t)(C - 1); t.d.Dp = tree_keep_path_cap(C, depth);
    return t;
}

// the node count a lane starts from: < 1 is an empty tree (the caller clears node 0), values above C are read as C
static POMDP_TREE_HD int32_t tree_keep_clamp_count(const TreeView &t, int32_t n) { return n < 1 ? 0 : (n > t.d.S + 1 ? t.d.S + 1 : n); }

// tree_child for a pool that does fill up: the child of (h, a) under observation ob, created as node n_nodes when there is
// none and the pool has room.  With no child and no room nothing is written, `full` is set and h comes back: the simulation
// leaves the tree without a node.
static POMDP_TREE_HD int32_t tree_child_or_full(const TreeView &t, int32_t h, int32_t a, int32_t ob, int32_t &n_nodes, bool &created,
                                                bool &full)
{
    const int64_t ei = tree_edge_index(t, h, a);
    const int32_t first = t.edge[ei].child;
    int32_t c = first;
    created = false;
    full = false;
    for (int32_t guard = 0; c > 0 && c <= t.d.S && guard <= t.d.S; ++guard) {
        const TreeNode nd = t.node[c];
        if (nd.ob == ob) return c;
        c = nd.next;
    }
    if (n_nodes < 1 || n_nodes > t.d.S) { full = true; return tree_clamp_node(t, h); }
    const int32_t fresh = n_nodes++;
    tree_fresh_node(t, fresh, ob, first);
    t.edge[ei].child = fresh;
    created = true;
    return fresh;
}

// The subtree of src under the root's child (action, ob), copied into dst breadth-first (a Cheney copy: dst's nodes are the
// queue, a pending node's source index waits in its spare fourth word and is cleared when the node is scanned).  The kept
// child becomes node 0 with observation 0 and no sibling; a node's actions are scanned in ascending order and the children
// of one (h, a) keep their chain order; N, V and Nh are copied as they are.  -> the node count of dst, 0 where there is
// nothing to keep (an empty source, an action outside [0, A), no such child) — dst is then left as it was.
// src and dst have the same A and C and do not overlap; src is only read.
static POMDP_TREE_HD int32_t tree_keep_copy(const TreeView &src, int32_t n_src, const TreeView &dst, int32_t action, int32_t ob)
{
    const int32_t A = dst.d.A, C = dst.d.S + 1;
    const int32_t n = tree_keep_clamp_count(src, n_src);
    if (n < 1 || action < 0 || action >= A) return 0;
    int32_t c = src.edge[action].child;                      // node 0's edge row
    bool found = false;
    for (int32_t guard = 0; c > 0 && c < n && guard < C; ++guard) {
        const TreeNode nd = src.node[c];
        if (nd.ob == ob) { found = true; break; }
        c = nd.next;
    }
    if (!found) return 0;
    TreeNode root; root.ob = 0; root.next = 0; root.visits = src.node[c].visits; root.unused = c;
    dst.node[0] = root;
    int32_t count = 1;
    for (int32_t q = 0; q < count && q < C; ++q) {
        int32_t s = dst.node[q].unused;
        s = s < 0 ? 0 : (s >= n ? n - 1 : s);
        dst.node[q].unused = 0;
        for (int32_t a = 0; a < A; ++a) {
            const TreeEdge e = src.edge[(int64_t)s * A + a];
            int32_t head = 0, tail = 0;
            int32_t cc = e.child;
            while (cc > 0 && cc < n && count < C) {          // every turn fills one node of dst: at most C - 1 turns in all
                const TreeNode nd = src.node[cc];
                const int32_t idx = count++;
                TreeNode cp; cp.ob = nd.ob; cp.next = 0; cp.visits = nd.visits; cp.unused = cc;
                dst.node[idx] = cp;
                if (head == 0) head = idx; else dst.node[tail].next = idx;
                tail = idx;
                cc = nd.next;
            }
            TreeEdge o; o.v = e.v; o.n = e.n; o.child = head;
            dst.edge[(int64_t)q * A + a] = o;
        }
    }
    return count;
}

// What a kept tree adds where the search sets node priors (pomdp_tree_search_preferred_resume).  A kept node may or may not
// have received its priors: the one a simulation's last step created has none, and after the advance a later search stands
// on it.  Stored Nh == 0 says "neither primed nor visited" — priming sets Nh = prior_n * |P(h)| >= 1 and every backup adds
// one — so no flag word is needed and the spare word stays the copy's.
// tree_node_priors for a node h of a pool that holds n_nodes nodes, applied only while the node's stored Nh is 0: the ONE
// read of the node word decides, and its Nh comes back for the selection that follows (-> the node's Nh afterwards).  With
// Nh != 0, with prior_n < 1 or with h outside [0, n_nodes) nothing is written; otherwise the stores are tree_node_priors's:
// the node's A edges and its visit count, nothing else.
template <class In>
static POMDP_TREE_HD int32_t tree_node_priors_once(const TreeView &t, int32_t h, int32_t n_nodes, In in, int32_t prior_n, double prior_v)
{
    if (h < 0 || h > t.d.S || h >= n_nodes) return 0;
    const int32_t nh = t.node[h].visits;
    const int32_t pn = prior_n < 0 ? 0 : (prior_n > 65535 ? 65535 : prior_n);
    if (nh != 0 || pn == 0) return nh;
    int32_t listed = 0;
    for (int32_t a = 0; a < t.d.A; ++a) {
        const bool on = in(a);
        TreeEdge e; e.v = on ? prior_v : 0.0; e.n = on ? pn : 0; e.child = 0;
        t.edge[(int64_t)h * t.d.A + a] = e;
        listed += (int32_t)on;
    }
    t.node[h].visits = pn * listed;
    return pn * listed;
}

// tree_select_clamped with the node's Nh handed in (what tree_node_priors_once returned) instead of read again: the same
// scan, the same four float64 operations per visited action, none fused.
template <class Pick>
static POMDP_TREE_HD int32_t tree_select_nh(const TreeView &t, int32_t h, int32_t nh, int count, Pick pick, double ucb_c, const double *logn,
                                            int32_t nh_max)
{
#pragma clang fp contract(off)
    const int32_t hc = tree_clamp_node(t, h);
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

} // namespace pomdp
