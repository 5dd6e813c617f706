// particles.hip — particle beliefs (pomdp_particle_init / pomdp_particle_update / pomdp_plan_particles): the batched filter
// a POMCP-style planner keeps per real episode.  Each root holds P particles (state columns r * P .. r * P + P - 1); after a
// real step every particle is stepped under the real action, the ones that reproduce the real observation survive, and the
// others are redrawn from the survivors — all in one launch per call, so a planning step never leaves the device.
// Part of libpomdp_hip.so; built by gym_pomdp_amd/_native.py (hipcc --offload-arch=gfx950 -O3 -std=c++17 -c, one object per file).
#include "kernels_common.hip.h"

namespace pomdp {

constexpr int PARTICLE_MAX = 4096;
constexpr int PARTICLE_WORDS = PARTICLE_MAX / 64;             // match-bitmap words of one workgroup: a wave ballot each

// ---- the fused filter ---------------------------------------------------------------------------------------------------
// Geometry: P >= 256: one workgroup per root, thread v holds slots v, v + 256, ... (ceil(P / 256) chunks); P < 256: 256 / P
// roots per workgroup, thread v holds slot v % P of root v / P (threads past the last whole root idle).  A slot's global lane
// g = lane0 + r * P + j keeps g & 3 == v & 3 (lane0 and P are multiples of 4), so a global quad sits in a hardware quad.
// Phase 1: every slot's proposal — Env::step of its column under action[r] at (seed, g, t) (INIT: Env::reset) — is written
// to its own column of `out`, and its match bit goes into the workgroup's bitmap (one 64-bit ballot per wave and chunk, in
// slot order).  Phase 2: an exclusive scan of the bitmap's popcounts (one wave) gives every matching slot its rank among its
// root's survivors, which it writes into the survivor list in LDS.  Phase 3: a non-matching slot of a root with m >= 1
// survivors copies the column of survivor (w * m) >> 32, w = word 0 of stream PARTICLE at (seed, g, t).  Survivors' columns
// are only read and other columns only written in phase 3, so the copy has no hazard.
// Visibility of phase 1's columns to phase 3's readers in other waves of the workgroup (the hand-off of
// cdna_hip_programming.md §6 Guideline 16, R1, inside one workgroup): the proposals are stored write-through
// (Env::store: st_stream, `global_store ... sc1`); every storing wave then waits for its own stores to complete
// (`s_waitcnt vmcnt(0)`, R1's drain — a barrier alone drains no vector-memory operation, MI355X_MICROARCH.md) before the
// workgroup barrier, so when any wave passes that barrier every proposal has left the CU.  Phase 3 reads the columns with
// nontemporal loads, which bypass the CU's vector L1 and are served by the XCD's L2 or memory (MI355X_MICROARCH.md,
// visibility table: "sc1 / sc0 sc1 / nt loads bypass L1 only") — no stale L1 line can be read.  All waves of a workgroup
// run on one CU, hence one XCD: no agent-scope fence is involved.
// Every lane of a wave runs the lane step (BattleShip's step, Tag's and Tiger's quad words are lane-local,
// but the step kernels run it convergently too); results of padding threads and unfiltered roots are discarded.
template <class Env, bool INIT>
__global__ __launch_bounds__(BLOCK) void particle_kernel(const typename Env::Params p, const uint32_t *__restrict__ in,
                                                         uint32_t *__restrict__ out, const int32_t *__restrict__ action,
                                                         const int32_t *__restrict__ ob, const uint32_t *__restrict__ reward,
                                                         const uint8_t *__restrict__ done, const uint8_t *__restrict__ where,
                                                         int32_t *__restrict__ n_match, int64_t n_roots, int P, int match_reward,
                                                         RngKey key, uint32_t lane0)
{
    constexpr int W = Env::WORDS;
    __shared__ typename Env::Shared sh;
    __shared__ uint16_t surv[PARTICLE_MAX];
    __shared__ uint64_t bits[PARTICLE_WORDS + 1];
    __shared__ uint32_t pre[PARTICLE_WORDS + 1];
    Env::stage(sh, p, (int)threadIdx.x);
    const int v = (int)threadIdx.x, wave = v >> 6;
    const bool wide = P >= BLOCK;
    const int T = wide ? BLOCK : P;                             // threads per root
    const int C = wide ? (P + BLOCK - 1) / BLOCK : 1;           // chunks
    const int G = BLOCK / T;                                    // roots per workgroup
    const int gr = wide ? 0 : v / P;
    const int64_t root = (int64_t)blockIdx.x * G + gr;
    const bool root_ok = gr < G && root < n_roots;
    const int64_t rc = root_ok ? root : n_roots - 1;            // padding threads read the last root
    const int64_t N = n_roots * (int64_t)P;
    const int fs = wide ? 0 : gr * P;                           // the root's first bit of the workgroup's bitmap
    const uint32_t n_act = (uint32_t)Env::n_actions(p);
    int32_t a = 0;
    bool filt = root_ok;                                        // the root is filtered (INIT: reset) in this call
    if constexpr (INIT) {
        if (where) filt = filt && where[rc] != 0;
    } else {
        a = action[rc];
        filt = filt && (uint32_t)a < n_act;
    }
    const int32_t want_ob = ob ? ob[rc] : 0;
    const uint32_t want_r = (!INIT && match_reward) ? reward[rc] : 0u;
    const uint8_t want_d = (!INIT && done) ? (uint8_t)(done[rc] != 0) : 0;
    __syncthreads();

    uint32_t mine = 0;                                          // bit c: this thread's slot of chunk c matched
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const int jr = wide ? c * BLOCK + v : v - fs;           // slot within the root
        const bool slot_ok = root_ok && jr < P;
        const int jc = slot_ok ? jr : 0;
        const uint32_t col = (uint32_t)(rc * P + jc);
        const uint32_t g = lane0 + col;
        typename Env::State st;
        bool m = false;
        if constexpr (INIT) {
            const int o = Env::reset(sh, p, st, key, g);
            if (slot_ok && filt) {
                Env::store(st, out, N, col, true);
                m = !ob || o == want_ob;
            }
        } else {
            Env::load(st, in, N, col);
            if constexpr (has_next<Env>::value) Env::load_next(st, in, N, col);
            int o, d;
            typename Env::Reward r;
            Env::step(sh, p, st, filt ? (int)a : 0, key, g, o, r, d);
            if (slot_ok) {
                if (filt) {
                    Env::store(st, out, N, col, true);
                    static_assert(sizeof(typename Env::Reward) == 4, "rewards are compared as their 32-bit patterns");
                    uint32_t rb;
                    __builtin_memcpy(&rb, &r, 4);
                    m = o == want_ob && (!done || (uint8_t)(d != 0) == want_d) && (!match_reward || rb == want_r);
                } else {                                        // an action out of range: the column as it was
#pragma unroll
                    for (int w = 0; w < W; ++w) out[(int64_t)w * N + col] = ld_stream(in + (int64_t)w * N + col);
                }
            }
        }
        const uint64_t b = __ballot(m);
        if ((v & 63) == 0) bits[c * (BLOCK / 64) + wave] = b;
        mine |= (uint32_t)m << c;
    }
    const int nw = C * (BLOCK / 64);
    if (v == 0) bits[nw] = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the proposals' stores complete before the barrier (above)
    __syncthreads();
    if (wave == 0) {                                            // exclusive scan of the words' popcounts: pre[k] = bits before word k
        const uint32_t x = v < nw ? (uint32_t)__popcll(bits[v]) : 0u;
        uint32_t s = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(s, d);
            s += (v & 63) >= d ? y : 0u;
        }
        pre[v] = s - x;
        if (v == 63) pre[64] = s;
    }
    __syncthreads();
    auto below = [&](int f) -> uint32_t {                       // matching slots of the workgroup before flat position f
        const uint64_t lo = (f & 63) ? (bits[f >> 6] & ((1ull << (f & 63)) - 1ull)) : 0ull;
        return pre[f >> 6] + (uint32_t)__popcll(lo);
    };
    const uint32_t base = below(fs);
    const uint32_t m_root = below(fs + P) - base;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const int f = wide ? c * BLOCK + v : v;
        if ((mine >> c) & 1u) surv[fs + (int)(below(f) - base)] = (uint16_t)(f - fs);
    }
    __syncthreads();
    if (root_ok && filt && m_root > 0) {
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            const int jr = wide ? c * BLOCK + v : v - fs;
            if (jr >= P || ((mine >> c) & 1u)) continue;
            const uint32_t col = (uint32_t)(root * P + jr);
            const uint32_t w = stream_block(key, lane0 + col, POMDP_STREAM_PARTICLE, 0u).x;
            const uint32_t src = (uint32_t)(root * P) + surv[fs + (int)__umulhi(w, m_root)];
#pragma unroll
            for (int k = 0; k < W; ++k) out[(int64_t)k * N + col] = __builtin_nontemporal_load(out + (int64_t)k * N + src);
        }
    }
    if (root_ok && (wide ? v == 0 : v == fs)) n_match[root] = filt ? (int32_t)m_root : -1;
}

template <class Env, bool INIT>
static int launch_particles(const typename Env::Params &p, const uint32_t *in, uint32_t *out, const int32_t *action,
                            const int32_t *ob, const void *reward, const uint8_t *done, const uint8_t *where, int32_t *n_match,
                            int64_t n_roots, int P, int flags, uint64_t seed, uint32_t lane0, uint64_t t, void *stream)
{
    const int64_t G = P >= BLOCK ? 1 : BLOCK / P;
    const unsigned grid = (unsigned)((n_roots + G - 1) / G);
    hipLaunchKernelGGL((particle_kernel<Env, INIT>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, p, in, out, action, ob,
                       reinterpret_cast<const uint32_t *>(reward), done, where, n_match, n_roots, P,
                       (flags & POMDP_PARTICLE_MATCH_REWARD) ? 1 : 0, make_key(seed, t), lane0);
    return (int)hipGetLastError();
}

// the shape checks every entry point shares: P % 4 == 0, 4 <= P <= 4096, lane0 % 4 == 0, lane0 + R * P <= 2^32
static bool particle_shape_ok(int64_t n_roots, int P, uint32_t lane0)
{
    if (n_roots < 0 || P < 4 || P > PARTICLE_MAX || (P & 3) || (lane0 & 3u) || n_roots > (1ll << 32)) return false;
    return !bad_range(n_roots * (int64_t)P, lane0);
}

static int env_words(int env, const void *params)
{
    return dispatch_env(env, params, [](auto tag, const auto &) { return (int)decltype(tag)::Env::WORDS; });
}

} // namespace pomdp

extern "C" {

int pomdp_particle_init(int env, const void *params, uint32_t *particles, const int32_t *ob, const uint8_t *where,
                        int32_t *n_match, int64_t n_roots, int n_particles, uint64_t seed, uint32_t lane0, uint64_t t,
                        void *stream)
{
    using namespace pomdp;
    if (!params || !particles || !n_match || !particle_shape_ok(n_roots, n_particles, lane0)) return POMDP_E_BADARG;
    const int rc = dispatch_env(env, params, [](auto, const auto &) { return 0; });
    if (rc) return rc;
    if (n_roots == 0) return 0;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_particles<E, true>(p, nullptr, particles, nullptr, ob, nullptr, nullptr, where, n_match, n_roots, n_particles, 0,
                                         seed, lane0, t, stream);
    });
}

int pomdp_particle_update(int env, const void *params, const uint32_t *particles_in, uint32_t *particles_out,
                          const int32_t *action, const int32_t *ob, const void *reward, const uint8_t *done,
                          int32_t *n_match, int64_t n_roots, int n_particles, int flags, uint64_t seed, uint32_t lane0,
                          uint64_t t, void *stream)
{
    using namespace pomdp;
    if (!params || !particles_in || !particles_out || !action || !ob || !n_match || (flags & ~POMDP_PARTICLE_MATCH_REWARD) ||
        ((flags & POMDP_PARTICLE_MATCH_REWARD) && !reward) || !particle_shape_ok(n_roots, n_particles, lane0))
        return POMDP_E_BADARG;
    const int words = env_words(env, params);
    if (words < 0) return words;                                // POMDP_E_BADPARAMS / unknown env
    const uintptr_t bytes = (uintptr_t)words * (uintptr_t)n_roots * (uintptr_t)n_particles * 4u;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(particles_in), b0 = reinterpret_cast<uintptr_t>(particles_out);
    if (a0 < b0 + bytes && b0 < a0 + bytes && (bytes > 0 || a0 == b0)) return POMDP_E_BADARG;   // in and out overlap
    if (n_roots == 0) return 0;
    return dispatch_env(env, params, [&](auto tag, const auto &p) {
        using E = typename decltype(tag)::Env;
        return launch_particles<E, false>(p, particles_in, particles_out, action, ob, reward, done, nullptr, n_match, n_roots,
                                          n_particles, flags, seed, lane0, t, stream);
    });
}

int pomdp_plan_particles(int env, const void *params, const uint32_t *particles, int64_t n_roots, int n_particles,
                         int64_t sims_per_root, int depth, double discount, int flags, uint64_t seed, uint32_t lane0,
                         uint64_t t0, double *sim_ret, int32_t *sim_first_action, const pomdp_plan_out *out, void *stream)
{
    using namespace pomdp;
    if (!params || !particles || !out || n_particles < 4 || n_particles > PARTICLE_MAX || (n_particles & 3) || n_roots < 0 ||
        n_roots > 0x7FFFFFFF || sims_per_root < n_particles || sims_per_root % n_particles)
        return POMDP_E_BADARG;
    const int rc = dispatch_env(env, params, [](auto, const auto &) { return 0; });
    if (rc) return rc;
    const int n_act = (int)env_action_count(env, params);
    if (!out->q || !out->visits || !out->best || n_act < 1 || n_act > 255 || out->stride < n_act) return POMDP_E_BADARG;
    // every argument pomdp_rollout / pomdp_plan_reduce check is checked before anything is enqueued
    if (!sim_ret || !sim_first_action || depth < 0 || bad_range(n_roots * sims_per_root, lane0) || (lane0 & 3u)) return POMDP_E_BADARG;
    const int r = pomdp_rollout(env, params, particles, n_roots * n_particles, sims_per_root / n_particles, depth, discount, flags,
                                seed, lane0, t0, sim_ret, nullptr, sim_first_action, nullptr, nullptr, stream);
    if (r) return r;
    return pomdp_plan_reduce(sim_ret, sim_first_action, n_roots, sims_per_root, n_act, out, stream);
}

} // extern "C"
