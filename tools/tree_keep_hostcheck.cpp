// tree_keep_hostcheck.cpp — the pool code of kept search trees (gym_pomdp_amd/csrc/tree_keep.hip.h on top of tree_pool.hip.h) run on
// the host under the sanitizers:   g++ -std=c++17 -fsanitize=address,undefined -o hostcheck tools/tree_keep_hostcheck.cpp
// Every pool is one aligned_alloc of exactly the advertised bytes, so an index past a tree's slice is a heap overflow.  A toy
// env (A actions, a few observations, episodes that end) drives the search loop of tree_keep.hip — select, push, the child
// lookup / insert that reports a full pool, backup — through several searches with the copy to a second pool between them;
// each copy of a well-formed source is compared, node for node, with a pointer-based reference built from the source pool.
// Then the copy and the search loop run over garbage: random bytes and random small indices in the source pool, with a node
// count anywhere in int32.  Exit status 0 = every check held; tests/test_tree_keep_host.py builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../gym_pomdp_amd/csrc/tree_keep.hip.h"

using namespace pomdp;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static int rnd_below(int n) { return (int)(rnd() % (uint32_t)n); }

#define CHECK(c)                                                                                                              \
    do {                                                                                                                      \
        if (!(c)) {                                                                                                           \
            std::fprintf(stderr, "tree_keep_hostcheck: %s failed at line %d\n", #c, __LINE__);                                \
            std::exit(1);                                                                                                     \
        }                                                                                                                     \
    } while (0)

struct Pool {                                                // one tree in exactly tree_keep_bytes bytes
    void *mem;
    uint64_t bytes;
    TreeView view;
    Pool(int A, int C, int D) : bytes(tree_keep_bytes(A, C, D))
    {
        mem = std::aligned_alloc(16, bytes);
        CHECK(mem != nullptr && bytes % 16 == 0);
        std::memset(mem, 0xA5, bytes);
        view = tree_keep_view(mem, 0, A, C, D);
        CHECK((char *)(view.path + view.d.Dp) == (char *)mem + bytes);      // the three slices fill the pool exactly
    }
    ~Pool() { std::free(mem); }
    Pool(const Pool &) = delete;
    Pool &operator=(const Pool &) = delete;
};

// the pointer-based reference: a node owns its children
struct RNode {
    std::vector<int32_t> N;
    std::vector<double> V;
    int32_t Nh = 0;
    std::vector<std::vector<std::pair<int32_t, std::unique_ptr<RNode>>>> kids;   // per action, in chain order: (ob, child)
};

// a well-formed pool as reference nodes; also counts the nodes reached
static std::unique_ptr<RNode> decode(const TreeView &t, int32_t n_nodes, int32_t h, int &reached)
{
    CHECK(h >= 0 && h < n_nodes);
    CHECK(++reached <= n_nodes);
    auto r = std::make_unique<RNode>();
    r->Nh = t.node[h].visits;
    r->kids.resize(t.d.A);
    for (int a = 0; a < t.d.A; ++a) {
        const TreeEdge e = t.edge[(int64_t)h * t.d.A + a];
        r->N.push_back(e.n);
        r->V.push_back(e.v);
        for (int32_t c = e.child; c != 0; c = t.node[c].next) {
            CHECK(c > 0 && c < n_nodes);
            r->kids[a].emplace_back(t.node[c].ob, decode(t, n_nodes, c, reached));
        }
    }
    return r;
}

static int count_nodes(const RNode &r)
{
    int n = 1;
    for (const auto &ks : r.kids)
        for (const auto &k : ks) n += count_nodes(*k.second);
    return n;
}

static void same_tree(const RNode &x, const RNode &y)
{
    CHECK(x.Nh == y.Nh && x.N == y.N && x.kids.size() == y.kids.size());
    CHECK(std::memcmp(x.V.data(), y.V.data(), x.V.size() * sizeof(double)) == 0);
    for (size_t a = 0; a < x.kids.size(); ++a) {
        CHECK(x.kids[a].size() == y.kids[a].size());
        for (size_t j = 0; j < x.kids[a].size(); ++j) {      // chain order is kept
            CHECK(x.kids[a][j].first == y.kids[a][j].first);
            same_tree(*x.kids[a][j].second, *y.kids[a][j].second);
        }
    }
}

// the copy's numbering: breadth-first, actions ascending, chain order
static void check_breadth_first(const TreeView &t, int32_t n_nodes)
{
    int32_t next = 1;
    CHECK(t.node[0].ob == 0 && t.node[0].next == 0);
    for (int32_t q = 0; q < n_nodes; ++q) {
        CHECK(t.node[q].unused == 0);
        for (int a = 0; a < t.d.A; ++a)
            for (int32_t c = t.edge[(int64_t)q * t.d.A + a].child; c != 0; c = t.node[c].next) CHECK(c == next++);
    }
    CHECK(next == n_nodes);
}

// the toy env: the state is a small integer, an episode ends now and then
struct Toy {
    int A, n_obs;
    void step(int &s, int a, int &ob, double &r, int &done) const
    {
        const uint32_t x = rnd();
        s = (int)((uint32_t)(s * 31 + a * 7 + 1) % 97u);
        ob = (int)(x % (uint32_t)n_obs) - 1;                 // -1 is an observation like any other
        r = (double)((s % 7) - 3);
        done = (x >> 8) % 11 == 0;
    }
};

// tree_keep.hip's simulation loop for one lane.  well_formed: also check what only holds for pools a search made.
static void search(const Toy &env, const TreeView &t, int32_t &n_nodes, int S, int D, const std::vector<double> &logn, bool well_formed,
                   int &full_events)
{
    const int C = t.d.S + 1;
    n_nodes = tree_keep_clamp_count(t, n_nodes);
    if (n_nodes < 1) {
        tree_fresh_node(t, 0, 0, 0);
        n_nodes = 1;
    }
    for (int s = 0; s < S; ++s) {
        int st = s % 5, d = 0, k0 = -1;
        int32_t h = 0, plen = 0;
        double acc = 0.0, disc = 1.0;
        for (int step = 0; step < D && !d; ++step) {
            int a;
            if (k0 < 0)
                a = tree_select_clamped(t, h, env.A, [](int idx) { return idx; }, 1.5, logn.data(), (int32_t)logn.size() - 1);
            else
                a = rnd_below(env.A);
            CHECK(a >= 0 && a < env.A);
            int ob;
            double r;
            env.step(st, a, ob, r, d);
            if (k0 < 0) {
                const int32_t before = plen;
                tree_push(t, plen, h, a, r);
                if (well_formed) CHECK(plen == before + 1);  // the path bound min(D, C) is never the one that binds
                if (!d) {
                    bool created, full;
                    const int32_t n_before = n_nodes;
                    std::vector<char> snap;
                    if (n_nodes >= C) snap.assign((char *)t.edge, (char *)t.path);     // edges and nodes
                    const int32_t hn = tree_child_or_full(t, h, a, ob, n_nodes, created, full);
                    CHECK(!(created && full) && hn >= 0 && hn < C && n_nodes <= C);
                    if (created) CHECK(n_before < C && hn == n_before && n_nodes == n_before + 1);
                    if (full) {
                        CHECK(n_before == C && n_nodes == C);
                        CHECK(std::memcmp(snap.data(), t.edge, snap.size()) == 0);     // nothing in the tree is written
                        ++full_events;
                    }
                    if (well_formed && !created && !full) CHECK(hn > 0 && t.node[hn].ob == ob);
                    h = hn;
                    if (created || full) k0 = step + 1;
                }
            } else {
                acc += disc * r;
                disc *= 0.95;
            }
        }
        CHECK(plen <= t.d.Dp);
        const double rt = tree_backup(t, plen, acc, 0.95);
        if (well_formed) CHECK(std::isfinite(rt));
    }
}

static std::vector<double> log_table(int n)
{
    std::vector<double> t(n < 2 ? 2 : n);
    t[0] = -INFINITY;
    for (size_t k = 1; k < t.size(); ++k) t[k] = std::log((double)k);
    return t;
}

// several searches with the copy between them, every copy against the reference
static void well_formed_case(int A, int C, int S, int D, int searches, int &full_events, int &kept_max)
{
    const Toy env{A, 3};
    Pool p0(A, C, D), p1(A, C, D);
    Pool *cur = &p0, *other = &p1;
    int32_t n_nodes = rnd_below(2) ? 0 : -rnd_below(1000);   // empty, both spellings
    const std::vector<double> logn = log_table(searches * S + 1);
    for (int round = 0; round < searches; ++round) {
        search(env, cur->view, n_nodes, S, D, logn, true, full_events);
        CHECK(n_nodes >= 1 && n_nodes <= C && n_nodes <= 1 + (round + 1) * S);
        int reached = 0;
        std::unique_ptr<RNode> ref = decode(cur->view, n_nodes, 0, reached);
        CHECK(reached == n_nodes);                           // every node hangs in the tree
        CHECK(ref->Nh <= (round + 1) * S);
        std::vector<char> src_before((char *)cur->mem, (char *)cur->mem + cur->bytes);
        // a child that exists (when there is one), else whatever; now and then an action out of range
        int action = rnd_below(A), ob = rnd_below(3) - 1;
        for (int a = 0; a < A; ++a)
            if (!ref->kids[a].empty() && rnd_below(4) != 0) {
                action = a;
                ob = ref->kids[a][rnd_below((int)ref->kids[a].size())].first;
                break;
            }
        if (rnd_below(9) == 0) action = rnd_below(2) ? -1 - rnd_below(3) : A + rnd_below(3);
        const RNode *want = nullptr;
        if (action >= 0 && action < A)
            for (const auto &k : ref->kids[action])
                if (k.first == ob) want = k.second.get();
        const int32_t kept = tree_keep_copy(cur->view, n_nodes, other->view, action, ob);
        CHECK(std::memcmp(src_before.data(), cur->mem, cur->bytes) == 0);     // src is not written
        if (!want) {
            CHECK(kept == 0);
        } else {
            CHECK(kept == count_nodes(*want) && kept < n_nodes);
            int r2 = 0;
            std::unique_ptr<RNode> got = decode(other->view, kept, 0, r2);
            CHECK(r2 == kept);
            same_tree(*got, *want);
            check_breadth_first(other->view, kept);
            if (kept > kept_max) kept_max = kept;
        }
        n_nodes = kept;
        std::swap(cur, other);
    }
}

// garbage in the source pool and a node count anywhere in int32: the copy and the search stay inside the pools and end
static void garbage_case(int A, int C, int D, bool small_indices)
{
    Pool src(A, C, D), dst(A, C, D);
    unsigned char *b = (unsigned char *)src.mem;
    for (uint64_t j = 0; j < src.bytes; ++j) b[j] = (unsigned char)rnd();
    if (small_indices) {                                     // links that mostly stay in range: cycles, shared children, self loops
        for (int64_t j = 0; j < (int64_t)C * A; ++j) {
            src.view.edge[j].child = rnd_below(C + 4) - 2;
            src.view.edge[j].n = rnd_below(5) - 1;
            src.view.edge[j].v = (double)rnd_below(9);
        }
        for (int j = 0; j < C; ++j) {
            src.view.node[j].ob = rnd_below(3) - 1;
            src.view.node[j].next = rnd_below(C + 4) - 2;
            src.view.node[j].visits = rnd_below(2) ? (int32_t)rnd() : rnd_below(50);
        }
    }
    static const int32_t counts[] = {INT32_MIN, -1, 0, 1, 2, INT32_MAX};
    int32_t n = rnd_below(3) == 0 ? counts[rnd_below(6)] : (rnd_below(2) ? (int32_t)((rnd() << 1) ^ rnd()) : rnd_below(C + 3) - 1);
    const int action = rnd_below(A + 2) - 1, ob = rnd_below(3) - 1;
    const int32_t kept = tree_keep_copy(src.view, n, dst.view, action, ob);
    CHECK(kept >= 0 && kept <= C);
    if (n < 1 || action < 0 || action >= A) CHECK(kept == 0);
    if (kept > 0)                                            // what the copy wrote is itself in range
        for (int32_t q = 0; q < kept; ++q)
            for (int a = 0; a < A; ++a) {
                const int32_t c = dst.view.edge[(int64_t)q * A + a].child;
                CHECK(c >= 0 && c < kept);
            }
    int full_events = 0;
    const Toy env{A, 3};
    search(env, src.view, n, 6, D, log_table(8), false, full_events);     // a short table: Nh is clamped
    CHECK(n >= 1 && n <= C);
}

int main()
{
    int full_events = 0, kept_max = 0;
    const int As[] = {1, 2, 3, 5, 13, 64, 255};
    for (int A : As)
        for (int S : {1, 9, 40})
            for (int C : {1, 2, S + 1, S / 2 + 2, 2 * S + 1})
                for (int D : {0, 1, 6, C + 3}) well_formed_case(A, C, S, D, 5, full_events, kept_max);
    for (int j = 0; j < 200; ++j) {
        const int A = 1 + rnd_below(255), S = 1 + rnd_below(30);
        well_formed_case(A, 1 + rnd_below(2 * S + 2), S, rnd_below(12), 4, full_events, kept_max);
    }
    CHECK(full_events > 0 && kept_max >= 8);                 // the branches were reached
    for (int j = 0; j < 3000; ++j) {
        const int A = j % 7 == 0 ? 255 : 1 + rnd_below(j % 3 == 0 ? 255 : 6);
        const int C = 1 + rnd_below(j % 5 == 0 ? 40 : 6);
        garbage_case(A, C, rnd_below(2) ? rnd_below(C + 4) : 0, j % 2 == 0);
    }
    std::printf("tree_keep_hostcheck: ok (%d full-pool events, largest kept subtree %d nodes)\n", full_events, kept_max);
    return 0;
}
