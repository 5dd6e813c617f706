// tree_keep_preferred_hostcheck.cpp — what the preferred-policy search adds to the pool code of kept trees
// (gym_pomdp_amd/csrc/tree_keep.hip.h: tree_node_priors_once, tree_select_nh) run on the host under the sanitizers:
//   g++ -std=c++17 -fsanitize=address,undefined -o hostcheck tools/tree_keep_preferred_hostcheck.cpp
// Every pool is one aligned_alloc of exactly tree_keep_bytes, so an index past the tree's slice is a heap overflow.  For every
// A in 1..255, prior_n in {0, 1, 65535}, pools of C = 1 and more, part-filled and full, and random masks (empty and full
// included) it primes nodes whose Nh is 0, nodes whose Nh is > 0 and nodes the pool does not hold, and compares the whole pool
// byte for byte with a snapshot: a primed or absent node changes nothing at all, an unprimed one changes its own A edges and its
// own visit word and nothing else.  tree_select_nh with the Nh that comes back must pick what tree_select_clamped picks from the
// stored one, at every clamp of the log table.  Exit status 0 = every check held; tests/test_tree_keep_preferred_host.py
// builds and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gym_pomdp_amd/csrc/tree_keep.hip.h"

using namespace pomdp;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static int rnd_below(int n) { return (int)(rnd() % (uint32_t)n); }

#define CHECK(c)                                                                                                              \
    do {                                                                                                                      \
        if (!(c)) {                                                                                                           \
            std::fprintf(stderr, "tree_keep_preferred_hostcheck: %s failed at line %d\n", #c, __LINE__);                      \
            std::exit(1);                                                                                                     \
        }                                                                                                                     \
    } while (0)

struct Pool {                                                // one tree in exactly tree_keep_bytes bytes
    unsigned char *mem;
    uint64_t bytes;
    TreeView view;
    Pool(int A, int C, int D) : bytes(tree_keep_bytes(A, C, D))
    {
        mem = (unsigned char *)std::aligned_alloc(16, bytes);
        CHECK(mem != nullptr && bytes % 16 == 0);
        std::memset(mem, 0xA5, bytes);
        view = tree_keep_view(mem, 0, A, C, D);
        CHECK((unsigned char *)(view.path + view.d.Dp) == mem + bytes);     // the three slices fill the pool exactly
    }
    ~Pool() { std::free(mem); }
    Pool(const Pool &) = delete;
    Pool &operator=(const Pool &) = delete;
};

static long n_primed = 0, n_kept = 0, n_absent = 0, n_selects = 0;

// the nodes [0, n_nodes) of a pool: some unprimed (Nh == 0, cleared edges), the others visited (Nh > 0, arbitrary edges)
static void fill(const TreeView &t, int n_nodes)
{
    for (int h = 0; h < n_nodes; ++h) {
        tree_fresh_node(t, h, rnd_below(7), h + 1 < n_nodes && rnd_below(2) ? h + 1 : 0);
        t.node[h].unused = (int32_t)rnd();                  // the copy's spare word: whatever it holds must stay
        if (rnd_below(2)) continue;
        int32_t nh = 0;
        for (int a = 0; a < t.d.A; ++a) {
            TreeEdge e; e.n = rnd_below(3) ? rnd_below(50) : 0; e.v = (double)rnd_below(2001) / 8.0 - 125.0; e.child = 0;
            t.edge[(int64_t)h * t.d.A + a] = e;
            nh += e.n;
        }
        t.node[h].visits = nh > 0 ? nh : 1 + rnd_below(9);  // Nh > 0 even where the edges sum to 0: the word alone decides
    }
}

static std::vector<bool> random_mask(int A, int kind)
{
    std::vector<bool> m(A);
    for (int a = 0; a < A; ++a) m[a] = kind == 0 ? false : kind == 1 ? true : rnd_below(kind) == 0;
    return m;
}

// selection from the Nh handed in == selection from the stored Nh
static std::vector<double> logn;                             // logn[n] = log(n) up to the largest Nh a primed node can start with
static void check_select(const TreeView &t, int32_t h, int32_t nh, int32_t nh_max)
{
    CHECK(nh_max >= 1 && (size_t)nh_max < logn.size());
    std::vector<int32_t> legal;
    for (int a = 0; a < t.d.A; ++a)
        if (rnd_below(3)) legal.push_back(a);
    if (legal.empty()) legal.push_back(rnd_below(t.d.A));
    const auto pick = [&](int i) { return legal[(size_t)i]; };
    const double c = (double)rnd_below(40);
    const int32_t x = tree_select_nh(t, h, nh, (int)legal.size(), pick, c, logn.data(), nh_max);
    const int32_t y = tree_select_clamped(t, h, (int)legal.size(), pick, c, logn.data(), nh_max);
    CHECK(x == y && x >= 0 && x < t.d.A);
    ++n_selects;
}

static void one_pool(int A, int C, int D, int n_nodes, int32_t prior_n, double prior_v)
{
    Pool pool(A, C, D);
    const TreeView &t = pool.view;
    fill(t, n_nodes);
    std::vector<unsigned char> snap(pool.bytes);
    for (int round = 0; round < 6; ++round) {
        // a node the pool holds, the slot after the last one, and indices no pool has
        int32_t h = rnd_below(n_nodes);
        if (round == 3) h = n_nodes;                         // absent: inside the pool's memory when n_nodes < C, past it when full
        if (round == 4) h = rnd_below(2) ? -1 - rnd_below(1000) : C + rnd_below(1000);
        if (round == 5) h = (int32_t)(rnd() | 0x40000000u);
        const std::vector<bool> mask = random_mask(A, round % 3 == 0 ? rnd_below(2) : 2 + rnd_below(4));
        int32_t listed = 0;
        for (int a = 0; a < A; ++a) listed += mask[a];
        long calls = 0;
        const auto in = [&](int32_t a) { ++calls; CHECK(a >= 0 && a < A); return (bool)mask[(size_t)a]; };
        std::memcpy(snap.data(), pool.mem, pool.bytes);
        const bool present = h >= 0 && h < n_nodes;
        const int32_t stored = present ? t.node[h].visits : 0;
        const int32_t got = tree_node_priors_once(t, h, n_nodes, in, prior_n, prior_v);
        if (!present || stored != 0 || prior_n < 1) {        // absent, primed or visited, or a search without priors: nothing at all
            CHECK(std::memcmp(snap.data(), pool.mem, pool.bytes) == 0);
            CHECK(got == stored && calls == 0);
            if (present) ++n_kept; else ++n_absent;
        } else {
            CHECK(got == prior_n * listed && calls == A);
            CHECK(t.node[h].visits == got);
            for (int a = 0; a < A; ++a) {
                const TreeEdge e = t.edge[(int64_t)h * A + a];
                CHECK(e.child == 0 && e.n == (mask[a] ? prior_n : 0));
                const double want = mask[a] ? prior_v : 0.0;
                CHECK(std::memcmp(&e.v, &want, sizeof(double)) == 0);
            }
            // nothing outside the node's edge row and its visit word: put the old bytes back there and compare everything
            std::vector<unsigned char> now(pool.mem, pool.mem + pool.bytes);
            const size_t row = (size_t)h * (size_t)A * sizeof(TreeEdge);
            std::memcpy(now.data() + row, snap.data() + row, (size_t)A * sizeof(TreeEdge));
            const size_t word = (size_t)((unsigned char *)&t.node[h].visits - pool.mem);
            std::memcpy(now.data() + word, snap.data() + word, sizeof(int32_t));
            CHECK(std::memcmp(now.data(), snap.data(), pool.bytes) == 0);
            ++n_primed;
            if (got > 0) {                                   // primed now: a second call writes nothing
                std::memcpy(snap.data(), pool.mem, pool.bytes);
                calls = 0;
                CHECK(tree_node_priors_once(t, h, n_nodes, in, prior_n, prior_v) == got && calls == 0);
                CHECK(std::memcmp(snap.data(), pool.mem, pool.bytes) == 0);
            }
        }
        if (present) {
            // a table that holds Nh, one that is one entry short of it, and the shortest one
            for (int32_t nh_max : {got + 3, got - 1 > 1 ? got - 1 : 1, 1}) check_select(t, h, got, nh_max);
        }
    }
}

int main()
{
    const int32_t priors[3] = {0, 1, 65535};
    logn.resize((size_t)65535 * 255 + 8);
    logn[0] = -INFINITY;
    for (size_t k = 1; k < logn.size(); ++k) logn[k] = std::log((double)k);
    for (int A = 1; A <= 255; ++A)
        for (int pi = 0; pi < 3; ++pi)
            for (int shape = 0; shape < 4; ++shape) {
                const int C = shape == 0 ? 1 : 2 + rnd_below(shape == 1 ? 3 : 40);
                const int D = rnd_below(12);
                const int n_nodes = shape == 2 ? C : 1 + rnd_below(C);         // shape 2 (and C = 1): a full pool
                one_pool(A, C, D, n_nodes, priors[pi], pi == 1 ? -20.0 : 5.0);
            }
    CHECK(n_primed > 1000 && n_kept > 1000 && n_absent > 1000 && n_selects > 10000);
    std::printf("tree_keep_preferred_hostcheck: ok (%ld primed, %ld left as they were, %ld absent, %ld selections)\n", n_primed, n_kept,
                n_absent, n_selects);
    return 0;
}
