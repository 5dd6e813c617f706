// heuristic_impl.hip.h — the heuristic-policy loop: History's append on a lane's words, the sinks for
// the loop's rows, the kernel and its launcher (the side statistics' update is RockEnv::belief_update, a fresh episode's
// arrays and the sums' contributions are planner_common.hip.h's).  Shared by planner.hip, which instantiates
// the loop that keeps nothing per step (pomdp_heuristic_steps), and heuristic_collect.hip, which instantiates it with the
// record sinks (pomdp_heuristic_collect) — translation units of their own, so that the second family's register allocation
// cannot disturb the first's (RockSample's sits on the 80-register edge).
#pragma once
#include "kernels_common.hip.h"
#include "planner_common.hip.h"

namespace pomdp {

// check_sums applied to the history's own arrays, in place; mv: the caller's copy of h.move_ok[i]
static __device__ __forceinline__ void history_check_sums(const pomdp_history &h, int j, int next_ob, bool prev_bad, int64_t n,
                                                          uint32_t i, uint32_t &mv, int sign = 1)
{
    const int64_t k = (int64_t)j * n + i;
    const int ds = check_ds(next_ob, sign), dm = check_dm(next_ob, prev_bad, sign);
    if (ds) {
        const int ts = h.total_sample[k] + ds;
        h.total_sample[k] = ts;
        mv = with_bit(mv, 0x10000u << j, ts > 0);
    }
    if (dm) {
        const int tm = h.total_move[k] + dm;
        h.total_move[k] = tm;
        mv = with_bit(mv, 1u << j, tm >= 0);
    }
}

// history.append(transition) of rock.py:541-544 on the lane's words: `size` (the list length), the window of a bounded
// history (max_size >= 0: one byte per kept transition — action | next_ob << 5 | (observation == BAD) << 7 — in a ring of
// max_size + 1 rows, `head` = the row the next transition goes to, which holds the OLDEST one once the ring is full:
// the reference pops element 0 when size > max_size and then appends, so the list settles at max_size + 1 records) and,
// for RockSample (K > 0), the two per-rock sums kept current as transitions enter and leave the window.
// A record leaves the sums with exactly what it entered them with ONLY for what the byte holds — an action in [0, 31] and a
// next observation in [0, 3]: the caller hands in nothing else (the heuristic loop's come from the env; history_append_kernel
// canonicalises the caller's int32s first).
// RING = false: the caller knows there is no window to keep (an unbounded history, or an env without rocks) — the
// heuristic loop is instantiated both ways so that the unbounded history does not carry the window's registers and branches.
template <bool RING = true>
static __device__ __forceinline__ void history_push(const pomdp_history &h, int K, int a, int next_ob, int prev_ob, int64_t n,
                                                    uint32_t i, int &hsize, int &head, uint32_t &mv)
{
    const int W = h.max_size + 1;                                              // 0: unbounded
    if (RING && W > 0 && K > 0) {
        uint8_t *slot = h.ring + (int64_t)head * n + i;
        if (hsize == W) {                                                      // self._history.pop(0)
            const uint32_t old = *slot;
            const int oa = (int)(old & 31u);
            if (oa >= 5 && oa < 5 + K) history_check_sums(h, oa - 5, (int)((old >> 5) & 3u), (old >> 7) != 0u, n, i, mv, -1);
        }
        *slot = (uint8_t)((uint32_t)a | ((uint32_t)next_ob << 5) | ((prev_ob == 1) ? 128u : 0u));
        head = head + 1 == W ? 0 : head + 1;
    }
    hsize = (W > 0 && hsize == W) ? W : hsize + 1;
    if (a >= 5 && a < 5 + K) history_check_sums(h, a - 5, next_ob, prev_ob == 1, n, i, mv);
}

// ---- what the heuristic loop keeps of every step --------------------------------------------------------------------------
// One thread = one lane here (the fused step loops' sinks, traj_out.hip.h, belong to threads that own two or four lanes).  Arg:
// a record sink's kernel argument (advance(c): on to the next launch of a call that is split at pomdp_fuse_max()); the object
// itself is built per thread from the thread's index in the shard.  put(record) once per step, by EVERY thread of the workgroup — the
// narrow sink moves words round the hardware quad, whose padding threads take part.  The row's base is wave-uniform and moves
// on by scalar adds; a thread adds its 32-bit offset at the store (PackedRowOut, traj_out.hip.h).
struct HeurNoRows {
    static constexpr bool ROWS = false;
    __device__ __forceinline__ HeurNoRows(uint32_t, int64_t) {}
    __device__ __forceinline__ void put(uint32_t) {}
};
// POMDP_LAYOUT_PACKED: uint32 [k_steps][pitch] — one dword per thread, 256 contiguous bytes per wave
struct HeurPackedRows {
    static constexpr bool ROWS = true;
    struct Arg {
        uint8_t *traj;
        int64_t pitch;                                       // records per row
        void advance(int64_t steps) { traj += steps * 4 * pitch; }
    };
    uint8_t *row;                                            // the workgroup's first record of the row
    uint32_t off;
    int64_t row_bytes;
    bool on;
    __device__ __forceinline__ HeurPackedRows(uint32_t idx, int64_t n, const Arg &a)
        : row(a.traj + 4ull * BLOCK * blockIdx.x), off(4u * threadIdx.x), row_bytes(4 * a.pitch), on((uint64_t)idx < (uint64_t)n) {}
    __device__ __forceinline__ void put(uint32_t record)
    {
        off = row_offset(off);
        if (on) st_stream(reinterpret_cast<uint32_t *>(row + off), record);
        row += row_bytes;
    }
};
// POMDP_LAYOUT_NARROW: uint8 [k_steps][4][pitch].  A hardware quad holds four consecutive lanes' records; its thread e gathers
// byte e of the four (four DPP quad broadcasts, three v_perm_b32) and stores them as ONE dword of plane e: four dword stores per
// quad-step where a thread storing its own four bytes would make sixteen byte stores.  The padding threads of a ragged last
// quad hand in a record of 0 and store their plane's word like the others (pitch is a multiple of 4: the bytes lie inside the
// row); the quads past it store nothing.  A thread's offset within the row, 3 * pitch + 252 at most, has to fit 32 bits: the
// entry point refuses a wider pitch.
constexpr int64_t HEUR_NARROW_MAX_PITCH = (0xFFFFFFFFll - 252) / 3 / 4 * 4;
struct HeurNarrowRows {
    static constexpr bool ROWS = true;
    struct Arg {
        uint8_t *traj;
        int64_t pitch;                                       // bytes per plane
        void advance(int64_t steps) { traj += steps * 4 * pitch; }
    };
    uint8_t *row;                                            // the workgroup's first byte of the row's action plane
    uint32_t off, sel;
    int64_t row_bytes;
    bool on;
    __device__ __forceinline__ HeurNarrowRows(uint32_t idx, int64_t n, const Arg &a)
        : row(a.traj + (uint64_t)BLOCK * blockIdx.x), off((threadIdx.x & ~3u) + (threadIdx.x & 3u) * (uint32_t)a.pitch),
          sel(0x0C0C0400u + (threadIdx.x & 3u) * 0x0101u),   // v_perm_b32: byte e of the second operand, byte e of the first, 0, 0
          row_bytes(4 * a.pitch), on((uint64_t)(idx & ~3u) < (uint64_t)n) {}
    __device__ __forceinline__ void put(uint32_t record)
    {
        const uint32_t r0 = quad_bcast<0>(record), r1 = quad_bcast<1>(record), r2 = quad_bcast<2>(record), r3 = quad_bcast<3>(record);
        const uint32_t lo = __builtin_amdgcn_perm(r1, r0, sel), hi = __builtin_amdgcn_perm(r3, r2, sel);
        off = row_offset(off);
        if (on) st_stream(reinterpret_cast<uint32_t *>(row + off), __builtin_amdgcn_perm(hi, lo, 0x05040100u));
        row += row_bytes;
    }
};

// k heuristic-policy steps in one launch: per step choice(_generate_preferred(history)) -> step -> side statistics ->
// history.append, i.e. preferred_kernel + pick_actions_kernel + step_kernel + belief_update_kernel +
// history_append_kernel on the same call counter, with the lists never leaving registers.  Across the k steps a lane's
// state, its history words (size, last action / observation, prev_ob), the two derived words and the running return stay
// in registers and are written back once; the per-rock arrays are read and written in place when a CHECK touches them;
// every step's action / ob / reward / done (and state) is written as the single-step launches write them.
// Six waves per SIMD (at most 80 registers) where the compiler's own choice was five (81-86): the loop's CHECK / fresh-episode
// branches stall on memory, and the sixth wave fills those slots — RockSample(7,8) 4.64 -> 4.52, (15,15) 5.98 -> 5.85, Tag
// 4.35 -> 4.15 us per step at 2^20 lanes; four waves: 4.95 / 6.42 / 4.69, eight (spilling): 5.17 / 6.58 / 4.22.  BattleShip
// (three state words and more) keeps the compiler's own choice — waves_per_eu(1) constrains nothing: 81-105 registers, five
// or four waves; six would spill 100+ bytes per lane.  Every launch runs at least one step (the launcher's k >= 1): the
// outputs written after the loop are those of the launch's last step.
// Rows: what the loop keeps of every step (HeurNoRows: nothing — pomdp_heuristic_steps; HeurPackedRows / HeurNarrowRows: one
// 4-byte record per lane-step — pomdp_heuristic_collect, heuristic_collect.hip).  A record sink stores at the END of the step,
// behind the CHECK / fresh-episode branch: loads and stores share one counter and return in order, so a store issued before
// that branch would be one more thing every load in it waits for in the same step; issued after it, the store has the next
// step's policy and lane step (no loads) to drain behind.  The record sinks ask for five waves per SIMD (up to 96 registers)
// where the envs of one or two state words otherwise run six: at six RockSample's loops spill more than without rows (scratch
// per lane, (7,8): 20 -> 28 bytes packed, 36 narrow), at five they take 93-96 registers and spill nothing ((15,15) with a
// window: 12 bytes, 60 without rows); Tag, Tiger and BattleShip 5 x 5 stay under 80 registers and keep their six or seven
// waves.  What a row per step costs: DESIGN.md §9.
template <class Env, class Rows = HeurNoRows> struct heur_waves { static constexpr int value = Env::WORDS <= 2 ? (Rows::ROWS ? 5 : 6) : 1; };
// RING: a bounded RockSample history (history_push keeps its window).  RowsArg: Rows::Arg for a record sink, nothing for
// HeurNoRows — whose kernels keep the argument list they always had.
template <class Env, bool RING, class Rows = HeurNoRows, class... RowsArg>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(heur_waves<Env, Rows>::value)))
void heuristic_steps_kernel(const typename Env::Params p, uint32_t *__restrict__ state,
                                                                pomdp_rock_belief b, pomdp_history h, int K, pomdp_returns R,
                                                                int32_t *__restrict__ prev_ob, int32_t *__restrict__ action,
                                                                int32_t *__restrict__ ob, typename Env::Reward *__restrict__ reward,
                                                                uint8_t *__restrict__ done, int64_t n, RngKey key0, uint32_t lane0,
                                                                int flags, int k_steps, RowsArg... rows_arg)
{
#pragma clang fp contract(off)
    // the number of rocks is 0 at compile time for the envs without rocks: their loop carries none of the per-rock code
    // (Tag 4.03 -> 3.69 us per step, BattleShip 10 x 10 81 -> 72 registers; RockSample's own code is untouched — its
    // allocation sits on the 80-register edge and any rewording of these lines has cost it 8 %)
    K = Env::HAS_ROCKS ? K : 0;
    __shared__ typename Env::Shared sh;
    const bool auto_reset = flags & POMDP_AUTO_RESET;
    const uint32_t idx = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    const bool in_range = (uint64_t)idx < (uint64_t)n;
    const uint32_t i = in_range ? idx : (uint32_t)(n - 1);     // memory index only: threads past n read lane n - 1's words
    // the lane id — and with it the quad element e that picks which step's quad-shared block this thread computes — comes
    // from the UNCLAMPED index, as in rollout_kernel / steps_kernel: the padding threads of a ragged last quad (n % 4 != 0)
    // still supply the blocks of steps base + 1 .. 3 to the quad's in-range lanes through quad_transpose4
    const uint32_t lane = lane0 + idx;
    // every per-lane word first (one memory latency), then the tables
    typename Env::State st;
    Env::load(st, state, n, i);
    if constexpr (has_next<Env>::value) Env::load_next(st, state, n, i);
    int hsize = ld_stream(h.size + i), pob = ld_stream(prev_ob + i), head = RING ? ld_stream(h.head + i) : 0;
    int la = ld_stream(h.last_action + i), lo = ld_stream(h.last_ob + i);
    uint32_t ck = K ? ld_stream(b.check_ok + i) : 0u, mv = K ? ld_stream(h.move_ok + i) : 0u;
    bool was_done = auto_reset ? false : (ld_stream(done + i) != 0);
    double ret = R.ret ? R.ret[i] : 0.0, disc = R.ret ? R.disc[i] : 1.0;
    Env::stage(sh, p, (int)threadIdx.x);
    stage_policy_tables<Env>(sh, p);
    __syncthreads();
    bool ever_fresh = false;
    Rows rows(idx, n, rows_arg...);
    // what the launch's LAST step returns: every step overwrites the same n-element outputs, so only the last one's values
    // are ever visible — they are written once, after the loop (round 4).  Inside the loop they were four stores per step
    // that every CHECK's read-modify-write of the side statistics then waited behind (loads and stores share one counter).
    int out_a = -1, out_o = 0, out_d = 0;
    typename Env::Reward out_r = 0;
    const int hcap = h.max_size >= 0 ? h.max_size + 1 : 0x7FFFFFFF;            // len(history) stops there (rock.py:541-544)
    const uint64_t t0 = ((uint64_t)key0.t_hi << 32) | key0.t_lo;
    const uint32_t e = lane & 3u;
    // Random words four steps at a time, as in the rollout kernel: the policy's ACTION block is shared by the four lanes
    // of a quad (and so is RockSample's STEP block), so lane e of a quad computes the block(s) of step base + e and the
    // words travel by DPP quad-broadcast — one block per lane per four steps instead of four.
    // (no priority ladder here — LoopPrio, kernels_common.hip.h: this loop's launches run several rounds of workgroups and
    // its CHECK steps load; measured 2.17 -> 2.02e11 steps/s on RockSample(7,8) with it, no change on Tag)
    for (int base = 0; base < k_steps; base += 4) {
        const uint64_t te = t0 + (uint64_t)base + (uint64_t)e;
        RngKey ke = key0;
        ke.t_lo = (uint32_t)te; ke.t_hi = (uint32_t)(te >> 32);
        const uint4 aq = quad_transpose4(stream_block(ke, lane >> 2, POMDP_STREAM_ACTION, 0u), e);   // .J: this lane's word of step base + J
        uint4 sq = make_uint4(0, 0, 0, 0);
        if constexpr (Env::QUAD_SENSOR) sq = quad_transpose4(Env::quad_block(ke, lane, 0u), e);
        auto one_step = [&](auto jc) {
            constexpr int J = decltype(jc)::value;
            const int s = base + J;
            if (s >= k_steps) return;                                          // wave-uniform
            RngKey key = key0;
            key.t_lo = (uint32_t)(t0 + (uint64_t)s); key.t_hi = (uint32_t)((t0 + (uint64_t)s) >> 32);
            // the policy: a = list[(w * len(list)) >> 32] over the preferred list (ascending mask order) or the legal list
            const uint32_t word = comp<J>(aq);
            const uint32_t m = Env::preferred_mask(sh, p, st, h, n, i, ck, mv, hsize, la, lo);
            int a;
            if (m) a = nth_set_bit(m, (int)__umulhi(word, (uint32_t)__popc(m)));
            else {
                const auto L = LegalOf<Env>::make(sh, p, st, false);
                a = LegalOf<Env>::pick(sh, p, st, L, (int)__umulhi(word, (uint32_t)L.count));
            }
            const bool live = in_range && !was_done;
            const typename Env::State before = st;
            int o, d;
            typename Env::Reward r;
            if constexpr (Env::QUAD_SENSOR) {
                Env::step_with_H(sh, p, st, a, key, lane, comp<J>(sq), o, r, d);
            } else {
                Env::step(sh, p, st, a, key, lane, o, r, d);
            }
            if (!live) { o = 0; r = 0; d = was_done; st = before; }
            const bool fresh = live && d && auto_reset;
            if constexpr (Env::QUAD_SENSOR) {
                // RockSample: the fresh episode starts from the word the step's sensor draw would have read (auto-reset
                // contract, rock.hip.h) — this lane's word of the quad's block is already here; reset_where would compute
                // that block again, per lane, in every wave-step in which some lane's episode ends
                st.s = fresh ? Env::fresh_state(p, comp<J>(sq), key, lane) : st.s;
            } else {
                Env::reset_where(sh, p, st, fresh, key, lane);                 // wave-cooperative: every lane calls it
            }
            ever_fresh |= fresh;
            if (live) {
                if (R.ret) {                                                   // r += rw * discount; discount *= _discount
                    const double term = disc * (double)r;
                    const double acc = ret + term;
                    if (d) R.ret_done[i] = acc;
                    ret = fresh ? 0.0 : acc;
                    disc = fresh ? 1.0 : disc * R.discount;
                }
                if (fresh) {                                                   // new episode: fresh Rock objects, empty History
                    for (int j = 0; j < K; ++j) {
                        const int64_t k = (int64_t)j * n + i;
                        belief_fresh_rock(b, k);
                        history_fresh_rock(h, k);
                    }
                    ck = mv = K ? (1u << K) - 1u : 0u;
                    hsize = 0; la = -1; lo = -1; head = 0;
                    pob = Env::reset_ob(p, st);
                } else {
                    la = a; lo = o;                                            // a terminal transition is recorded too
                    if constexpr (RING) {
                        history_push<true>(h, K, a, o, pob, n, i, hsize, head, mv);
                        if constexpr (Env::HAS_ROCKS)                          // the side statistics (the other envs have none)
                            if (a >= 5 && a < 5 + K && o != 0 && !d) Env::belief_update(sh, p, st, a, o, b, n, i, ck);
                    } else {                                                   // no window: history_push<false>, one CHECK branch
                        hsize += (int)(hsize != hcap);
                        if (a >= 5 && a < 5 + K) {                             // K > 0: RockSample CHECK
                            history_check_sums(h, a - 5, o, pob == 1, n, i, mv);
                            if constexpr (Env::HAS_ROCKS)                      // the side statistics (the other envs have none)
                                if (o != 0 && !d) Env::belief_update(sh, p, st, a, o, b, n, i, ck);
                        }
                    }
                    pob = o;
                }
            }
            if constexpr (Rows::ROWS)                                          // a frozen lane: 0x010000FF; a padding thread: 0
                rows.put(in_range ? pack_record(live ? (uint32_t)a : 0xFFu, (uint32_t)o, Env::reward_code(r), (uint32_t)(d != 0)) : 0u);
            out_a = live ? a : -1; out_o = o; out_r = r; out_d = d;
            if (live) was_done = auto_reset ? false : (d != 0);
        };
        one_step(std::integral_constant<int, 0>{});
        one_step(std::integral_constant<int, 1>{});
        one_step(std::integral_constant<int, 2>{});
        one_step(std::integral_constant<int, 3>{});
    }
    if (!in_range) return;
    st_stream(action + i, (int32_t)out_a);
    st_stream(ob + i, (int32_t)out_o);
    st_stream(reward + i, out_r);
    st_stream(done + i, (uint8_t)out_d);
    Env::store(st, state, n, i, ever_fresh);                                   // the loop's carry, written once
    st_stream(h.size + i, (int32_t)hsize); st_stream(h.last_action + i, (int32_t)la); st_stream(h.last_ob + i, (int32_t)lo);
    st_stream(prev_ob + i, (int32_t)pob);
    if (K) { st_stream(b.check_ok + i, ck); st_stream(h.move_ok + i, mv); }
    if (RING) st_stream(h.head + i, (int32_t)head);                            // without a window `head` never moves
    if (R.ret) { R.ret[i] = ret; R.disc[i] = disc; }
}

template <class Env, class Rows = HeurNoRows, class... RowsArg>
static int launch_heuristic_steps(const typename Env::Params &p, uint32_t *state, const pomdp_rock_belief *b,
                                  const pomdp_history *h, int K, int32_t *prev_ob, int32_t *action, int32_t *ob, void *reward,
                                  uint8_t *done, const pomdp_returns *returns, int64_t n, uint64_t seed, uint32_t lane0,
                                  uint64_t t0, int64_t k_steps, int flags, void *stream, RowsArg... rows)
{
    if (n == 0) return 0;
    static const pomdp_returns NO_RETURNS = {0.0, nullptr, nullptr, nullptr};
    const int64_t FUSE_MAX = fuse_max();                  // steps per launch
    for (int64_t s = 0; s < k_steps; s += FUSE_MAX) {
        const int c = (int)(k_steps - s < FUSE_MAX ? k_steps - s : FUSE_MAX);
        bool ring = false;
        if constexpr (Env::HAS_ROCKS) ring = h->max_size >= 0 && K > 0 && h->ring && h->head;
        if constexpr (Env::HAS_ROCKS) {
            if (ring)
                hipLaunchKernelGGL((heuristic_steps_kernel<Env, true, Rows, RowsArg...>), dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p,
                                   state, b ? *b : NO_BELIEF, *h, K, returns ? *returns : NO_RETURNS, prev_ob, action, ob,
                                   (typename Env::Reward *)reward, done, n, make_key(seed, t0 + (uint64_t)s), lane0, flags, c, rows...);
        }
        if (!ring)
            hipLaunchKernelGGL((heuristic_steps_kernel<Env, false, Rows, RowsArg...>), dim3(blocks_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, p,
                               state, b ? *b : NO_BELIEF, *h, K, returns ? *returns : NO_RETURNS, prev_ob, action, ob,
                               (typename Env::Reward *)reward, done, n, make_key(seed, t0 + (uint64_t)s), lane0, flags, c, rows...);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
        (rows.advance(c), ...);
    }
    return 0;
}

// the number of rocks the history keeps sums for; -1: not an env (or not valid RockSample params)
static int history_rocks(int env, const void *params)
{
    if (env != POMDP_ENV_ROCK) return (env >= POMDP_ENV_TAG && env <= POMDP_ENV_NETWORK) ? 0 : -1;
    const pomdp_rock_params *p = (const pomdp_rock_params *)params;
    return (p && rock_ok(p)) ? rock_count(*p) : -1;
}

// what pomdp_heuristic_steps and pomdp_heuristic_collect refuse alike; K = history_rocks(env, params)
static inline bool heuristic_args_ok(int K, const void *params, const uint32_t *state, const pomdp_rock_belief *b, const pomdp_history *h,
                                     const int32_t *prev_ob, const int32_t *action, const int32_t *ob, const void *reward,
                                     const uint8_t *done, const pomdp_returns *returns, int64_t n, uint32_t lane0, int64_t k_steps)
{
    // (the policy's block — and RockSample's STEP / RESET blocks — are shared by global lanes 4 q .. 4 q + 3 and travel
    // within the hardware quad: a shard has to start on such a boundary)
    if (K < 0 || !params || !state || !prev_ob || !action || !ob || !reward || !done || k_steps < 0 || bad_range(n, lane0) || (lane0 & 3u))
        return false;
    if (!history_ok(h, K > 0) || (K > 0 && !belief_ok(b))) return false;
    return !returns || (returns->ret && returns->disc && returns->ret_done);
}

} // namespace pomdp
