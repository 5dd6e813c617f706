/*
 * pomdp_hip.h — C ABI of libpomdp_hip.so, the MI355X (gfx950) batched step()/reset()
 * path for gym_pomdp's discrete envs.
 *
 * The reference (d3sm0/gym_pomdp) is pure Python and has no FFI; the boundary it
 * exposes for this path is the gym.Env duck type of each env class:
 *     reset() -> ob                     step(a) -> (ob, reward, done, info)
 * Each entry point below replaces the *arithmetic* of one of those methods for a
 * whole batch of independent env instances ("lanes"); the reference method it
 * stands in for is cited per function (paths relative to gym_pomdp/envs/).
 * The modules under gym_pomdp_amd/envs/ are the host-side mirror that calls these through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every pointer marked "device" is HBM the caller owns (e.g. a torch tensor's
 *     data_ptr()); the library never allocates or frees device memory, and never synchronises (pomdp_step_sync / pomdp_reset_sync / pomdp_stream_sync,
 *     which exist to do so, aside; those two keep ONE 64-byte block of pinned, portable host memory per calling thread — the flag
 *     a one-lane kernel publishes its outputs through — allocated at the thread's first such call and freed when the thread ends);
 *   - `state` is struct-of-arrays: uint32 [words][n], word-major, lane i at state[w*n + i];
 *   - params structs are read on the host at call time and passed to the kernel
 *     by value (kernarg) — they may live on the caller's stack;
 *   - `stream` is a hipStream_t (NULL = the null stream); launches are asynchronous; the calling thread's
 *     current HIP device must be the one that owns `stream` and the buffers (the library never calls
 *     hipSetDevice);
 *   - lanes are globally numbered: lane = lane0 + i.  Random draws depend only on
 *     (seed, lane, t, stream-id), never on n, the grid or the GPU count, so a batch
 *     sharded over several GPUs reproduces the single-GPU result exactly;
 *   - return value: 0 = ok, > 0 = hipError_t of the launch, < 0 = POMDP_E_*.
 *
 * Random-word contract: Philox4x32-10, key = (seed lo, seed hi),
 * ctr = (lane, t lo, t hi, stream_id << 24 | block); numpy legacy constructions on
 * top (res53 doubles, masked-rejection randint).  RockSample / StochasticRock lay their doubles out
 * "split": the high word of a double in one block, its low word in the following block, generated only when the
 * high word leaves a comparison undecided.  Both RockSample streams are shared by the four lanes of a quad: counter
 * word 0 = lane / 4, lane L reads element L % 4 of every block.  step: block 2j for the step's double j (RockEnv: j = 0
 * the sensor; StochasticRock: j = 0 the action gate, j = 1 the sensor).  reset: rock j reads the lane's element of block 0
 * of stream RESET rotated right by 2j + 2 bits (reset() only uses the top bit of the double: one word serves the lane's
 * sixteen rocks), its low word the element of block 1 under the same rotation.  The reset that follows a done step inside
 * that step's call (POMDP_AUTO_RESET) reads the same rotated pair from the step's own SENSOR blocks — stream STEP, blocks
 * b and b + 1, b = 0 (RockEnv) / 2 (StochasticRock) — instead: a step never makes both draws (a CHECK does not end the
 * episode), so each word is consumed once either way and a quad's step costs one Philox block (ABI 10).
 * Network's step (ABI 12): one double per up machine, then one for the action (network.py:94-109).  16 bits decide a
 * comparison with a threshold unless they equal the threshold's top 16 bits, so the TOP 16 bits of double j are a half —
 * upper for even j, lower for odd j — of element lane % 4 of block j / 2 of the QUAD's stream STEP (counter word 0 =
 * lane / 4): one block serves two draws of each of four lanes.  The 37 bits below them come from the lane's own stream
 * STEP_LO (block j / 2, elements 2 (j % 2) and 2 (j % 2) + 1) and are generated on such a tie (2^-16 per draw) only.
 * Tiger (ABI 13): a call with counter t makes at most one draw that matters — LISTEN's uniform() (tiger.py:140-149), the door
 * a wrong guess resamples (tiger.py:117-119), the door of the episode that reset() or the auto-reset after a right guess
 * starts (tiger.py:60-66) — and reads it from the QUAD's stream STEP (counter word 0 = lane / 4, lane L element L % 4): the
 * double's high word, or the door (bit 0), from block 0; the double's low word (a tie of the top 27 bits only) from block
 * 1.  One block serves four lanes.  (Streams STEP_SPACE / RESET_SPACE — the gym-space RNG's own — are no longer read.)
 * Consequence for callers: pomdp_tiger_reset and pomdp_tiger_step of the same lanes must not be given the same (seed, t) —
 * the step's wrong-door resample would redraw the door reset() just dealt.  A call counter that advances with every call
 * (what the host mirror keeps: reset() is call t, the first step call t + 1) never does; re-seeding with the SAME seed
 * rewinds it, so follow such a seed() by reset(), as the reference's callers do (network.py:176-177 in the other order is
 * harmless there: its reset() ran under the previous seed).
 * Tag with ONE opponent (ABI 13): a step draws only when a TAG fails (the opponent's flight: binomial(1, move_prob), then
 * np.random.choice over 2 or 4 moves, tag.py:201-207) or succeeds (the reset that follows inside the call: randint(29) per
 * cell, tag.py:181-193) — never both — and reads the lane's word W of the QUAD's STEP block 0 for either: the flight's double
 * is (W, the same element of block 1 — a tie of the top 27 bits only), its choice word is W again (bits 0-1; the double uses
 * bits 5-31); the auto-reset's attempt i < 6 reads bits 5 i .. 5 i + 4 of W, later attempts (4 x 10^-5 of the resets) the
 * lane's own stream RESET from its first word on.  pomdp_tag_reset itself and games with more opponents keep the
 * sequential per-lane streams.
 */
#ifndef POMDP_HIP_H
#define POMDP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POMDP_ABI_VERSION 15

enum {
    POMDP_E_BADARG = -1,     /* NULL pointer, n < 0, n + lane0 > 2^32 */
    POMDP_E_BADPARAMS = -2,  /* params outside what the packed layout supports */
};

/* flags for *_step */
enum {
    POMDP_AUTO_RESET = 1,    /* done lanes get a fresh episode in the same call (stream RESET of the same t; RockSample:
                                the step's own sensor blocks, BattleShip: the cached board — see the contracts above and
                                below); without it `done` is in/out and done lanes freeze: (ob, reward, done) = (0, 0, 1) */
    POMDP_FUSE_STEPS = 2,    /* pomdp_rollout_synthetic only: consecutive steps may share a launch (see there) */
};

/* id of the word streams of one (seed, lane, t) */
enum { POMDP_STREAM_STEP = 0, POMDP_STREAM_RESET = 1, POMDP_STREAM_STEP_SPACE = 2,
       POMDP_STREAM_RESET_SPACE = 3, POMDP_STREAM_ACTION = 4, POMDP_STREAM_ROLLOUT = 5, POMDP_STREAM_NEXT = 6,
       POMDP_STREAM_STEP_LO = 7, POMDP_STREAM_PARTICLE = 8, POMDP_STREAM_TREE = 9,
       POMDP_STREAM_CONTROLLER = 10 };

/* env kinds for the generic entry points */
enum { POMDP_ENV_ROCK = 0, POMDP_ENV_TAG = 1, POMDP_ENV_BATTLESHIP = 2, POMDP_ENV_TIGER = 3, POMDP_ENV_NETWORK = 4 };

/* ---- RockSample  (rock.py:96-407) ---------------------------------------- */
/* state words: 1 if num_rocks <= 12 else 2.  64-bit view s = w0 | w1 << 32:
 * bits 0-3 x, 4-7 y, bits 8+2j..9+2j = Rock j status + 1 (0 bad, 1 collected, 2 good). */
typedef struct pomdp_rock_params {
    int32_t  size;          /* board is size x size                       rock.py:108 */
    int32_t  num_rocks;     /* K <= 16; actions = 5 + K                   rock.py:113 */
    int32_t  start_x, start_y;                                         /* rock.py:107 */
    int8_t   rock_x[16], rock_y[16];                                   /* rock.py:106 */
    int8_t   grid[256];     /* grid[x * 16 + y] = rock id stamped at (x, y) or -1    rock.py:110-111 */
    uint64_t thr[32];       /* thr[d]: sensor correct iff k53 <= thr[d], d = L1 distance  rock.py:383-407 */
    double   eff[32];       /* eff(d) itself, returned by pomdp_compute_prob            rock.py:383-387 */
    int32_t  stochastic;    /* 1 = StochasticRockEnv (rock.py:428-504): the action is applied only when a
                               binomial(1, p_move) draw succeeds, penalties are 0 and do not terminate */
    int32_t  act_gt;        /* stochastic, 1: act iff k53 > act_thr instead — numpy's binomial(1, p_move) for p_move <= .5 (ABI 14) */
    uint64_t act_thr;       /* stochastic: act iff k53 <= act_thr (first double of stream STEP)  rock.py:443 */
} pomdp_rock_params;

/* replaces RockEnv.reset (rock.py:236-241, 266-271, 78-86).  ob (device, may be NULL) <- 0. */
int pomdp_rock_reset(const pomdp_rock_params *p, uint32_t *state, int32_t *ob, int64_t n,
                     uint64_t seed, uint32_t lane0, uint64_t t, void *stream);
/* replaces RockEnv.step (rock.py:123-194).  reward in {-100,-10,0,10}; err (device uint32, may be
 * NULL) counts lanes whose action was outside [0, 5+K): they are left untouched, (ob,reward,done)=(0,0,0). */
int pomdp_rock_step(const pomdp_rock_params *p, uint32_t *state, const int32_t *action, int32_t *ob,
                    int32_t *reward, uint8_t *done, uint32_t *err, int64_t n,
                    uint64_t seed, uint32_t lane0, uint64_t t, int flags, void *stream);

/* ---- Tag  (tag.py:36-291) -------------------------------------------------- */
/* state: 1 word: bits 0-4 agent cell, bits 5+5j.. opponent j cell (j < 4), bits 25-31 num_opp
 * (7-bit two's complement, saturating at -64). */
typedef struct pomdp_tag_params {
    int32_t  num_opponents; /* 1..4                                       tag.py:87 */
    int32_t  obs_cells;     /* "opponent seen" observation value          tag.py:94 */
    uint64_t move_thr;      /* opponent moves iff k53 <= move_thr         tag.py:204 */
    int32_t  move_gt;       /* 1: ... iff k53 > move_thr instead — numpy's binomial(1, p) for p <= .5 (ABI 12) */
    int32_t  reserved;
} pomdp_tag_params;

/* replaces TagEnv.reset (tag.py:97-102, 181-193) */
int pomdp_tag_reset(const pomdp_tag_params *p, uint32_t *state, int32_t *ob, int64_t n,
                    uint64_t seed, uint32_t lane0, uint64_t t, void *stream);
/* replaces TagEnv.step (tag.py:108-143); reward is float {-1, -10, +10} */
int pomdp_tag_step(const pomdp_tag_params *p, uint32_t *state, const int32_t *action, int32_t *ob,
                   float *reward, uint8_t *done, uint32_t *err, int64_t n,
                   uint64_t seed, uint32_t lane0, uint64_t t, int flags, void *stream);

/* ---- BattleShip  (battleship.py:12-211) ------------------------------------ */
/* state: 3*MW words, MW = ceil((x_size*y_size + 6) / 32) <= 4: occupied mask words 0..MW-1, then the
 * visited mask words (cell a = y * x_size + x is bit a; total_remaining in bits 26-31 of the last
 * visited word), then the occupied mask of the lane's NEXT episode.  Board contract: whenever a board
 * is dealt at call counter t — reset() draws it from stream RESET of (lane, t); the auto-reset of a
 * step at t moves the cached next board in — the board after it is drawn from stream NEXT of (lane, t).
 * A lane's boards are therefore known one episode ahead, and a fused launch builds the boards its
 * lanes used up side by side when it ends instead of stalling a wave on one lane's rejection loop. */
typedef struct pomdp_battleship_params {
    int32_t x_size, y_size; /* x_size * y_size <= 122                     battleship.py:67 */
    int32_t max_len;        /* ctor max_len (ships max_len .. 2), 2..10   battleship.py:74-75 */
    int32_t reserved;
    /* 128-bit cell masks (4 little-endian words each) the reset's placement test uses, derived from x_size
     * and y_size on the host so that no lane recomputes them: */
    uint32_t col0[4];       /* cells with x == 0 */
    uint32_t vpat[12][4];   /* vpat[k]: k cells in a column, from cell 0 upwards (bits 0, X, 2X, ...) */
} pomdp_battleship_params;

/* replaces BattleShipEnv.reset (battleship.py:131-137, 167-211) */
int pomdp_battleship_reset(const pomdp_battleship_params *p, uint32_t *state, int32_t *ob, int64_t n,
                           uint64_t seed, uint32_t lane0, uint64_t t, void *stream);
/* replaces BattleShipEnv.step (battleship.py:91-122) */
int pomdp_battleship_step(const pomdp_battleship_params *p, uint32_t *state, const int32_t *action,
                          int32_t *ob, int32_t *reward, uint8_t *done, uint32_t *err, int64_t n,
                          uint64_t seed, uint32_t lane0, uint64_t t, int flags, void *stream);

/* ---- Tiger  (tiger.py:47-172) ---------------------------------------------- */
/* state: 1 word, bit 0 = tiger door */
typedef struct pomdp_tiger_params {
    uint64_t listen_thr;    /* listen is wrong iff k53 > listen_thr       tiger.py:141-148 */
} pomdp_tiger_params;

/* replaces TigerEnv.reset (tiger.py:60-66); the hidden state is bit 0 of the lane's word of the quad's STEP block */
int pomdp_tiger_reset(const pomdp_tiger_params *p, uint32_t *state, int32_t *ob, int64_t n,
                      uint64_t seed, uint32_t lane0, uint64_t t, void *stream);
/* replaces TigerEnv.step (tiger.py:72-88) */
int pomdp_tiger_step(const pomdp_tiger_params *p, uint32_t *state, const int32_t *action, int32_t *ob,
                     int32_t *reward, uint8_t *done, uint32_t *err, int64_t n,
                     uint64_t seed, uint32_t lane0, uint64_t t, int flags, void *stream);

/* ---- Network  (network.py:24-168) ------------------------------------------ */
/* state: 1 word, bit i = machine i is up */
typedef struct pomdp_network_params {
    int32_t  n_machines;    /* <= 32                                      network.py:27 */
    uint32_t deg_gt2_mask;  /* machines with more than 2 neighbours       network.py:89 */
    uint32_t nb_mask[32];   /* neighbour set of machine i                 network.py:144-168 */
    uint64_t fail_thr;      /* fails iff k53 >  fail_thr     (p = .1)     network.py:97 */
    uint64_t fail_nb_thr;   /* fails iff k53 >  fail_nb_thr  (q = .33)    network.py:99 */
    uint64_t obs_thr;       /* truthful iff k53 <= obs_thr   (.95)        network.py:106-109 */
} pomdp_network_params;

/* replaces NetworkEnv.reset (network.py:61-69) */
int pomdp_network_reset(const pomdp_network_params *p, uint32_t *state, int32_t *ob, int64_t n,
                        uint64_t seed, uint32_t lane0, uint64_t t, void *stream);
/* replaces NetworkEnv.step (network.py:71-114); reward = float32(float64 reward of the reference) */
int pomdp_network_step(const pomdp_network_params *p, uint32_t *state, const int32_t *action, int32_t *ob,
                       float *reward, uint8_t *done, uint32_t *err, int64_t n,
                       uint64_t seed, uint32_t lane0, uint64_t t, int flags, void *stream);

/* ---- step with bound arguments ------------------------------------------------ */
/* Everything of a pomdp_<env>_step call that does not change from one step of a batched env to the next, gathered once by
 * the caller (host memory the caller owns; the library only reads it during the call).  pomdp_step(args, action, t, stream)
 * is pomdp_<env>_step(args->params, args->state, action, args->ob, args->reward, args->done, args->err, args->n, args->seed,
 * args->lane0, t, args->flags, stream) for the env kind args->env: the same kernels, the same results — what it saves is
 * the marshalling of thirteen arguments per call in the host language's FFI (ctypes: ~1 us of a ~7 us env.step()). */
typedef struct pomdp_step_args {
    int32_t   env;       /* POMDP_ENV_* */
    int32_t   flags;     /* POMDP_AUTO_RESET or 0 */
    const void *params;  /* the env's pomdp_<env>_params (host) */
    uint32_t *state;     /* device, [words][n] */
    int32_t  *ob;        /* device [n] */
    void     *reward;    /* device [n], int32 or float per env */
    uint8_t  *done;      /* device [n] */
    uint32_t *err;       /* device uint32, may be NULL */
    int64_t   n;
    uint64_t  seed;
    uint32_t  lane0;
    uint32_t  reserved;
} pomdp_step_args;
int pomdp_step(const pomdp_step_args *args, const int32_t *action, uint64_t t, void *stream);
/* pomdp_step, then wait until its outputs can be read by the host — with pomdp_reset_sync / pomdp_stream_sync the only
 * entry points of this library that block.  For hosts that step a single env the way the reference is used (python
 * scalars in and out, batch of 1, ob / reward / done pointing at PINNED HOST memory): launch and wait cost one FFI call.
 * With n == 1 the kernel publishes its outputs through a flag in pinned host memory (system-scope release) that the host
 * polls, so the call returns as soon as the outputs are visible; the stream stays ordered and later launches need no
 * further wait.  With n != 1 it is pomdp_step followed by hipStreamSynchronize(stream). */
int pomdp_step_sync(const pomdp_step_args *args, const int32_t *action, uint64_t t, void *stream);
/* pomdp_<env>_reset (env: POMDP_ENV_*, params: its pomdp_<env>_params) followed by the same wait; `ob` in pinned host
 * memory when n == 1 */
int pomdp_reset_sync(int env, const void *params, uint32_t *state, int32_t *ob, int64_t n, uint64_t seed, uint32_t lane0,
                     uint64_t t, void *stream);
/* hipStreamSynchronize(stream) by itself */
int pomdp_stream_sync(void *stream);

/* ---- helpers ---------------------------------------------------------------- */
/* synthetic uniform random policy used by bench.py: lanes 4q..4q+3 share the Philox block
 * ctr = (q, t lo, t hi, STREAM_ACTION << 24); action = (word[lane & 3] * n_actions) >> 32.
 * lane0 must be a multiple of 4 and `action` 16-byte aligned; n is arbitrary. */
int pomdp_synthetic_actions(int32_t *action, int64_t n, uint64_t seed, uint32_t lane0, uint64_t t,
                            uint32_t n_actions, void *stream);
/* raw generator, for known-answer tests: out (device) <- Philox4x32-10 of each of the n_blocks
 * (ctr[4], key[2]) pairs in `ctr_key` (device, uint32 [n_blocks][6]). */
int pomdp_philox_blocks(const uint32_t *ctr_key, uint32_t *out, int64_t n_blocks, void *stream);

/* Random-policy rollout driven from C: for s in [0, k_steps): pomdp_synthetic_actions at t0+s into
 * `action` (device scratch, int32[n]) with key `action_seed`, then pomdp_<env>_step at t0+s.  Exactly
 * the results a host loop over pomdp_synthetic_actions + step would produce, in k_steps + 1 launches:
 * when action_seed == seed (policy and env share the Philox key; their streams differ by stream id) the
 * policy kernel runs once, for t0, and every step launch also leaves the policy's actions for the
 * following call counter in `action` (on RockSample they ride in the cooperative reset pass); with a
 * distinct action_seed each step is a policy launch plus a step launch.  With POMDP_FUSE_STEPS in `flags` (shared key
 * only) up to pomdp_fuse_max() (256) consecutive steps run inside one launch: every step's ob / reward / done / next action is still
 * computed and written, in the same order, and the state when the launch ends, so every buffer holds what the per-step
 * launches leave, but a lane's state and action stay in registers between its steps and the launch ramp is paid once
 * per launch; the first launch derives the actions of t0 itself, so there is no policy launch at all.  Either way
 * `action` holds the actions of t0 + k_steps on return.  The caller's call counter advances by k_steps.  `params` points
 * at the env's pomdp_<env>_params; `reward` is int32 or float per env.  lane0 must be a multiple of 4 (the policy's
 * Philox block is shared by global lanes 4q .. 4q+3); n is arbitrary.  Params and pointers are checked before anything
 * is enqueued. */
int pomdp_rollout_synthetic(int env, const void *params, uint32_t *state, int32_t *action, int32_t *ob,
                            void *reward, uint8_t *done, uint32_t *err, int64_t n, uint64_t seed,
                            uint64_t action_seed, uint32_t lane0, uint64_t t0, int64_t k_steps, int flags,
                            void *stream);

/* Trajectory collection under the same policy (shared key, fused launches, POMDP_AUTO_RESET required): the k_steps
 * steps of pomdp_rollout_synthetic, but step s writes ROW s of ob / reward / done (device, [k_steps][pitch], pitch >= n
 * elements) instead of overwriting one row, and `action` (device, int32 [k_steps + 1][pitch]) receives the actions of
 * call counter t0 + s in row s (row k_steps = the actions the next call would take).  Row s of every output equals what
 * pomdp_synthetic_actions + pomdp_<env>_step at t0 + s leave in their n-element buffers; `state` ends as after the last
 * step.  This is the batched form of the reference callers' episode loops (rock.py:553-575): one launch per 256 steps,
 * each lane's state in registers, 13 bytes per lane-step written, state and first actions read once per launch.  Any
 * alignment and pitch >= n is accepted; columns on 16-byte boundaries (done: 4) with a pitch that is a multiple of 4 take the
 * launches that store 16 bytes per thread. */
int pomdp_collect_synthetic(int env, const void *params, uint32_t *state, int32_t *action, int32_t *ob, void *reward,
                            uint8_t *done, uint32_t *err, int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0,
                            int64_t k_steps, int64_t pitch, int flags, void *stream);

/* pomdp_collect_synthetic with its per-batch arguments bound once (see pomdp_step_args): pomdp_collect(a, t0, k, stream) is
 * pomdp_collect_synthetic(a->env, a->params, a->state, a->action, a->ob, a->reward, a->done, a->err, a->n, a->seed, a->lane0,
 * t0, k, a->pitch, a->flags, stream). */
typedef struct pomdp_collect_args {
    int32_t   env, flags;
    const void *params;
    uint32_t *state;
    int32_t  *action;    /* device [k + 1][pitch] */
    int32_t  *ob;        /* device [k][pitch] */
    void     *reward;
    uint8_t  *done;
    uint32_t *err;
    int64_t   n, pitch;
    uint64_t  seed;
    uint32_t  lane0, reserved;
} pomdp_collect_args;
int pomdp_collect(const pomdp_collect_args *args, uint64_t t0, int64_t k_steps, void *stream);

/* ---- trajectory layouts (ABI 11) ------------------------------------------------ */
/* pomdp_collect_synthetic writes the default layout, COLUMNS: four separate [step][pitch] arrays, the values the reference's
 * `ob, rw, done, info = env.step(action)` returns (rock.py:553-575) as int32 / float / uint8 columns.  A fused step then
 * feeds four write streams that lie whole columns apart, and how fast they drain depends on where the allocation's pages
 * happen to lie.  The two layouts below keep exactly the same information in ONE write stream:
 *
 * POMDP_LAYOUT_BLOCKED — same types, same 13 bytes per lane-step.  traj: uint8 [k_steps][pitch * 13], pitch a multiple of
 *   256 lanes; row s = pitch / 256 blocks of 3328 bytes, block q holding lanes 256 q .. 256 q + 255 of step s as
 *       action int32[256] | ob int32[256] | reward (int32 | float)[256] | done uint8[256]
 *   (action = the action TAKEN at step s; there is no row of "next actions").
 * POMDP_LAYOUT_PACKED — 4 bytes per lane-step.  traj: uint32 [k_steps][pitch]; record of (step s, lane i):
 *       action | ob << 8 | reward_code << 16 | done << 24
 *   Actions and observations of every env fit a byte (Tag's obs_cells <= 255 is checked).  reward_code: the reward itself as
 *   an int8 for RockSample / StochasticRock (-100, -10, 0, 10), Tag (-1, -10, 10), BattleShip (-10 .. cells - 1) and Tiger
 *   (-20, -1, 10: tiger.py:165-172); Network: kind * 68 + base for reward = float32(base - cost), cost = 0 / .1 / 2.5 for kind 0 (no action) /
 *   1 (ping) / 2 (reboot) (network.py:87-92, 103, 110).  pomdp_packed_reward() decodes either to the value COLUMNS holds.
 * POMDP_LAYOUT_NARROW (ABI 12) — the PACKED record's four bytes as four typed planes, 4 bytes per lane-step and nothing to
 *   decode.  traj: uint8 [k_steps][4][pitch], pitch a multiple of 4; plane 0 action uint8, 1 ob uint8, 2 reward_code (int8
 *   reward; Network: the code above, an index for a 204-entry table), 3 done uint8 — each plane of each step a typed array
 *   a consumer reads in place (plane p of step s starts (4 s + p) * pitch bytes into traj).
 * All three: POMDP_AUTO_RESET required, lane0 a multiple of 4; rows on 16-byte boundaries and n a multiple of 1024 take the
 * launches that store 16 bytes per thread, anything else the general ones; `state` ends as after the last step; the next
 * call derives its first actions from (seed, lane, t) again, so nothing else carries over. */
enum { POMDP_LAYOUT_COLUMNS = 0, POMDP_LAYOUT_BLOCKED = 1, POMDP_LAYOUT_PACKED = 2, POMDP_LAYOUT_NARROW = 3 };
int pomdp_collect_layout(int env, const void *params, uint32_t *state, void *traj, uint32_t *err, int64_t n, uint64_t seed,
                         uint32_t lane0, uint64_t t0, int64_t k_steps, int64_t pitch, int layout, int flags, void *stream);
/* the same with the per-batch arguments bound once (see pomdp_step_args) */
typedef struct pomdp_traj_args {
    int32_t   env, flags;
    int32_t   layout, reserved;
    const void *params;
    uint32_t *state;
    void     *traj;
    uint32_t *err;
    int64_t   n, pitch;
    uint64_t  seed;
    uint32_t  lane0, reserved2;
} pomdp_traj_args;
int pomdp_collect_traj(const pomdp_traj_args *args, uint64_t t0, int64_t k_steps, void *stream);
/* host-side: the reward a PACKED record's reward_code byte stands for (exactly the value the COLUMNS layout stores) */
double pomdp_packed_reward(int env, uint32_t reward_code);

/* PACKED records -> the default ABI's four columns, on the device (ABI 12): row s of `records` (uint32 [k_steps][pitch_in])
 * becomes row s of action int32 / ob int32 / reward (int32 | float per env: pomdp_packed_reward of the code) / done uint8,
 * each [k_steps][pitch_out], n lanes per row — the values pomdp_collect_synthetic writes into ob / reward / done and the
 * action TAKEN at each step (its rows 0 .. k_steps - 1).  One pass, 4 bytes read and 13 written per lane-step; rows and
 * columns on 16-byte boundaries (done: 4) with pitches that are multiples of 4 take the 16-byte accesses. */
int pomdp_decode_packed(int env, const uint32_t *records, int64_t n, int64_t k_steps, int64_t pitch_in, int32_t *action,
                        int32_t *ob, void *reward, uint8_t *done, int64_t pitch_out, void *stream);

/* ---- episode returns without a trajectory (ABI 12) ------------------------------- */
/* What the reference's callers do with the stream of `ob, rw, done, info = env.step(action)`: reduce it on the fly,
 *     r += discount * rw; discount *= .95          per step      (network.py:186-187, rock.py:569-570)
 *     eps.append(r) ... sum(eps) / len(eps)        per episode   (network.py:188-189)
 * pomdp_collect_returns runs the k_steps steps of pomdp_collect_synthetic (same policy, same draws, same final state, the
 * same launches) and keeps, per lane, only that reduction — nothing is written per step:
 *     acc  double [4][pitch]   row 0 ret       running return of the lane's current episode   (start at 0)
 *                              row 1 disc      its running discount                             (start at 1)
 *                              row 2 ret_done  return of the lane's last finished episode       (untouched until one ends)
 *                              row 3 ret_sum   sum of the returns of its finished episodes, added in the order they ended
 *     cnt  int32  [2][pitch]   row 0 episodes  number of finished episodes;  row 1 steps  number of steps taken
 * all in/out, so consecutive calls continue the same statistics.  Per step: ret += disc * reward; disc *= discount, in IEEE
 * double with separate multiply and add; a done step banks ret (ret_done = ret; ret_sum += ret; ++episodes) and the fresh
 * episode starts at ret = 0, disc = 1.  `reward` is the reference's own value: the integer rewards of RockSample / Tag /
 * BattleShip / Tiger, and for Network the float64 `base - .1` / `base - 2.5` of network.py:103, 110 (NOT the float32 the
 * reward column rounds it to).  POMDP_AUTO_RESET required; lane0 a multiple of 4; acc and cnt on 16-byte boundaries with a
 * pitch that is a multiple of 4 take the quad-per-thread launches. */
typedef struct pomdp_return_stats {
    double   discount;      /* the env's _discount (rock.py:115, tag.py:91, ...) */
    double  *acc;           /* device double [4][pitch] */
    int32_t *cnt;           /* device int32 [2][pitch] */
    int64_t  pitch;         /* >= n */
} pomdp_return_stats;
int pomdp_collect_returns(int env, const void *params, uint32_t *state, const pomdp_return_stats *stats, uint32_t *err,
                          int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0, int64_t k_steps, int flags, void *stream);

/* ---- fused launches over the CALLER's actions (ABI 14) ----------------------------------------------------------------
 * The reference's callers hand step() whatever they like (rock.py:562-566, tag.py:310-312, network.py:181-187).  With the
 * actions of k_steps steps known up front — a replayed trajectory, a table policy evaluated on the device, another model's
 * output — the fused launches above run on them instead of on the synthetic policy: state in registers between steps, up to
 * pomdp_fuse_max() steps per launch, every sink.
 *     tape.actions  device uint8 [k_steps][tape.stride]: row s = the actions of call counter t0 + s, lane i at byte i
 *                   (tape.stride >= n bytes from one row to the next; the action plane of a POMDP_LAYOUT_NARROW trajectory
 *                   is such a tape with stride = 4 * pitch).  Every env's actions fit a byte.
 * A byte outside the env's action range leaves the lane untouched for that step — (ob, reward, done) = (0, 0, 0), the record
 * keeps the byte as its action, the returns sink books a step with reward 0 — and is counted in *err, as pomdp_<env>_step
 * does.  Everything else is as in the synthetic-policy entry point of the same sink: same draws (the env's streams at (seed,
 * lane, t0 + s) do not depend on where the actions come from), same rows, same final state; POMDP_AUTO_RESET required, lane0
 * a multiple of 4.  Rows on 4-byte boundaries (tape.actions and tape.stride multiples of 4) with n a multiple of 1024 and
 * 16-byte-aligned sinks take the quad-per-thread loops, anything else the general one.
 *   pomdp_collect_tape          the default columns WITHOUT `action` (the caller has it): ob int32, reward int32 | float, done
 *                               uint8, each [k_steps][pitch] — row s what pomdp_<env>_step(action = tape row s) at t0 + s returns
 *   pomdp_collect_tape_layout   POMDP_LAYOUT_BLOCKED / _PACKED / _NARROW, as pomdp_collect_layout
 *   pomdp_collect_tape_returns  the episode statistics of pomdp_collect_returns */
typedef struct pomdp_tape {
    const uint8_t *actions;
    int64_t stride;
} pomdp_tape;
int pomdp_collect_tape(int env, const void *params, uint32_t *state, const pomdp_tape *tape, int32_t *ob, void *reward,
                       uint8_t *done, uint32_t *err, int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0, int64_t k_steps,
                       int64_t pitch, int flags, void *stream);
int pomdp_collect_tape_layout(int env, const void *params, uint32_t *state, const pomdp_tape *tape, void *traj, uint32_t *err,
                              int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0, int64_t k_steps, int64_t pitch, int layout,
                              int flags, void *stream);
int pomdp_collect_tape_returns(int env, const void *params, uint32_t *state, const pomdp_tape *tape,
                               const pomdp_return_stats *stats, uint32_t *err, int64_t n, uint64_t seed, uint32_t lane0,
                               uint64_t t0, int64_t k_steps, int flags, void *stream);

/* ---- episodes played to their end (ABI 15) -------------------------------------------------------------------------------
 * The reference's callers run one episode per env until it ends, then reset that env (rock.py:553-575, tag.py:310-312,
 * battleship.py:220-222).  A batch does the same without auto-reset: a lane whose episode ended is FROZEN — it keeps its state
 * and pomdp_<env>_step(flags = 0) returns (ob, reward, done) = (0, 0, 1) for it — until the caller restarts it.
 *
 * pomdp_reset_where: the masked reset.  A lane with where[i] != 0 starts the episode pomdp_<env>_reset at the same (seed, lane,
 * t) gives it (every state word, BattleShip's cached next board included); its ob[i] gets the fresh observation and done[i]
 * is cleared.  Every other lane keeps its state and done flag and gets ob[i] = -1 (no env observes -1).  ob and done may be
 * NULL; where == NULL means every lane, and then the results equal pomdp_<env>_reset's.  (env: POMDP_ENV_*, params: its
 * pomdp_<env>_params, host.) */
int pomdp_reset_where(int env, const void *params, uint32_t *state, int32_t *ob, uint8_t *done, const uint8_t *where, int64_t n,
                      uint64_t seed, uint32_t lane0, uint64_t t, void *stream);
/* pomdp_finish_episodes: the fused loops in frozen mode.  The results are those of k_steps per-step calls: the actions of
 * pomdp_synthetic_actions at t0 + s (or row s of `tape`, as in pomdp_collect_tape*), then pomdp_<env>_step(flags = 0) at t0 + s.
 *   - a lane that is live at step s writes its real record; its done flag is set when the episode ends;
 *   - a lane that is frozen at step s does not step and its state is untouched; its record is action | 1 << 24 (ob 0, reward 0,
 *     done 1), the action byte being the policy's action at t0 + s (or the tape byte) — what a per-step caller would pass;
 *   - an out-of-range tape byte of a live lane leaves it untouched, record = the byte (ob, reward, done = 0), and is counted
 *     in *err; a frozen lane's byte is not counted.
 * layout POMDP_LAYOUT_PACKED / _NARROW: traj and pitch as in pomdp_collect_layout.  POMDP_LAYOUT_RETURNS: the statistics of
 * pomdp_collect_returns (same float64 order, Network's float64 reward), booked for live steps only: each adds
 * ret += disc * reward; disc *= discount; ++steps, and a done step banks ret (ret_done, ret_sum, ++episodes) and restarts at
 * ret = 0, disc = 1.  With fresh statistics ret_done[i] is lane i's discounted return and steps[i] its length.
 * `done` (device [n]) is in/out: != 0 = the lane's episode has ended.  lane0 a multiple of 4; any n.  RockSample and
 * StochasticRock batches that qualify for steps_quad_kernel (n a multiple of 1024, 16-byte-aligned state and statistics, 4-byte-aligned done
 * and rows, 16 steps per launch or more) take a quad-per-thread loop, everything else one lane per thread; up to
 * pomdp_fuse_max() steps per launch.  The caller's call counter advances by k_steps.  The existing collection entry points
 * keep refusing flags = 0. */
enum { POMDP_LAYOUT_RETURNS = 4 };
typedef struct pomdp_episode_args {
    int32_t  env, layout;                /* POMDP_ENV_*; POMDP_LAYOUT_PACKED, _NARROW or _RETURNS */
    const void *params;                  /* the env's pomdp_<env>_params (host) */
    uint32_t *state;                     /* device [words][n] */
    uint8_t  *done;                      /* device [n], in/out: != 0 = the lane's episode has ended; it does not step */
    const pomdp_tape *tape;              /* NULL = the synthetic policy of pomdp_synthetic_actions at t0 + s */
    void     *traj;                      /* record layouts: device, as pomdp_collect_layout */
    int64_t   pitch;
    const pomdp_return_stats *stats;     /* POMDP_LAYOUT_RETURNS */
    uint32_t *err;                       /* device uint32, may be NULL */
    int64_t   n;
    uint64_t  seed;
    uint32_t  lane0, reserved;
} pomdp_episode_args;
int pomdp_finish_episodes(const pomdp_episode_args *a, uint64_t t0, int64_t k_steps, void *stream);

/* pomdp_controller_episodes: pomdp_finish_episodes under a policy that REACTS to what the lane observes — a finite-state
 * controller: K nodes, an action per node, a successor node per (node, observation).  A memoryless ob -> action table, an
 * open-loop or periodic plan and any finite-memory policy are such controllers; several of them side by side (disjoint node
 * ranges) are one, so a population is evaluated in one call by starting each lane in its own controller's range.  The
 * tables are staged into the workgroup's LDS once per launch (action as a byte, next as a halfword); a lane's node is one
 * register next to its state.  Frozen mode only (flags = 0 semantics, one episode per lane); `a` is read as by
 * pomdp_finish_episodes — layouts POMDP_LAYOUT_PACKED / _NARROW / _RETURNS, `done` in/out — and a->tape must be NULL.  Step s
 * runs at call counter t0 + s on the env's draws of (seed, lane, t0 + s), those of every other path.  Per lane and step:
 *   - a live lane takes action[node]; its record is the real one; then node = next[node][ob] — also on the step that ends the
 *     episode, after which the lane is frozen;
 *   - a frozen lane does not step; state and node are untouched; its record is action[node] | 1 << 24, the action byte being
 *     what a per-step caller would pass; nothing is counted;
 *   - a live lane whose action[node] is outside the env's action range is untouched for that step: record = the action byte,
 *     (ob, reward, done) = (0, 0, 0), the node unchanged, counted in *a->err, and the returns sink books a step with reward 0
 *     (the tape contract);
 *   - a live lane whose next[node][ob] is outside [0, n_nodes): the step stands, the node stays where it was, counted in
 *     *a->err (an observation the table has no column for — Tag with obs_cells < 28 — finds no successor either);
 *   - a lane whose incoming node[i] is outside [0, n_nodes) is treated like an out-of-range action on every step: untouched
 *     and counted while live, node[i] left as it was.
 * The action byte of a record is action[node] where that lies in [0, 255] and 255 otherwise (a value that does not fit a byte,
 * or no node at all) — the rule of a tape byte; 255 is out of range for every env.  No table entry and no node value makes
 * the kernel read outside its tables.
 * Any n; lane0 a multiple of 4; up to pomdp_fuse_max() steps per launch, `node` read when a launch starts and written when
 * it ends, so results never depend on the chunking.  Refused before anything is enqueued (POMDP_E_BADARG / _BADPARAMS):
 * everything pomdp_finish_episodes refuses; NULL c, action, next or node; n_nodes or n_nodes * n_obs past the limits below;
 * n_obs other than the env's observation count (RockSample 3, Tag obs_cells + 1, BattleShip 2, Tiger 3, Network 3); a->tape
 * not NULL; Tag with obs_cells > 255 for the record sinks.  k_steps == 0 or n == 0: 0, nothing launched.  The caller's call
 * counter advances by k_steps. */
typedef struct pomdp_controller {
    const int32_t *action;   /* device [n_nodes]: the action of node q */
    const int32_t *next;     /* device [n_nodes][n_obs]: successor of node q on observation o */
    int32_t  n_nodes, n_obs; /* 1 <= n_nodes <= 4096, n_nodes * n_obs <= 16384; n_obs = the env's observation count */
    int32_t *node;           /* device [n], in/out: lane i's current node */
} pomdp_controller;
int pomdp_controller_episodes(const pomdp_episode_args *a, const pomdp_controller *c,
                              uint64_t t0, int64_t k_steps, void *stream);

/* pomdp_stoch_controller_episodes: pomdp_controller_episodes under a STOCHASTIC finite-state controller — node q draws its
 * action from psi(a | q) and its successor from eta(q' | q, ob), inside the loop, per lane and per step.  The controller comes
 * in candidate form: K nodes, B candidate actions per node, D candidate successors per (node, observation), and uint32
 * thresholds that cut the 32-bit draw into the candidates' shares (the cumulative probabilities, quantised by the caller); the
 * deterministic controller is B = D = 1.  `a` is read as by pomdp_controller_episodes; the env's own draws are untouched (step s
 * runs pomdp_<env>_step(flags = 0) at t0 + s).
 * Draws: at step s lane g = lane0 + i reads block 0 of stream CONTROLLER at (seed, g, t0 + s) — counter (g, t lo, t hi,
 *   POMDP_STREAM_CONTROLLER << 24), as the PARTICLE and TREE words are built; a block per lane, not shared by a quad.  Word 0
 *   (.x) is the action draw u_a, word 1 (.y) the successor draw u_n; words 2 and 3 are not used.
 * Pick, in integers only: the candidate index of a draw u among `cand` candidates with thresholds thr[0 .. cand - 2] is the
 *   NUMBER of j in [0, cand - 1) with u > thr[j] (strict).  A count: defined for any threshold values, monotone or not, always
 *   in [0, cand); a threshold 0xFFFFFFFF is never passed, a threshold 0 is passed by every u but 0.  With thresholds
 *   thr[j] = ceil(2^32 c_j) - 1 of cumulative probabilities c_j, candidate 0 is drawn with probability ceil(2^32 c_0) / 2^32.
 *   The action drawn at t0 + s is action[q][index of u_a under action_thr[q]]; the successor is next[q][ob][index of u_n under
 *   next_thr[q][ob]].
 * Per lane and step, the rules of pomdp_controller_episodes with "action[node]" read as "the action drawn at t0 + s":
 *   - a live lane steps, records, then moves to the drawn successor — also on the step that ends its episode;
 *   - a frozen lane does not step; state and node are untouched; its record is the drawn action byte | 1 << 24 — what a
 *     per-step caller would pass, a function of (seed, lane, t, node) only; nothing is counted;
 *   - a live lane whose drawn action is outside the env's action range is untouched for that step: record = the action byte,
 *     (ob, reward, done) = (0, 0, 0), the node unchanged, counted in *a->err, and the returns sink books a step with reward 0;
 *   - a live lane whose drawn successor is outside [0, n_nodes), or whose observation has no column (Tag with obs_cells < 28):
 *     the step stands, the node stays, counted;
 *   - a lane whose incoming node[i] is outside [0, n_nodes) is treated like an out-of-range action on every step: untouched
 *     and counted while live, node[i] left as it was.
 * The action byte of a record is the drawn action where that lies in [0, 255] and 255 otherwise.  No table entry, threshold or
 * node value makes the kernel read outside its tables.
 * The tables are staged into the workgroup's LDS once per launch, sized by need: actions as bytes, successors as halfwords,
 * thresholds as 32-bit words — K*B + 4*K*(B-1) + 2*K*n_obs*D + 4*K*n_obs*(D-1) bytes, rounded up to 16, at most
 * POMDP_STOCH_CONTROLLER_MAX_BYTES (the deterministic controller's largest footprint).
 * Any n; lane0 a multiple of 4; up to pomdp_fuse_max() steps per launch, `node` read when a launch starts and written when
 * it ends, so results never depend on the chunking (nor on the sharding: every draw is a function of the global lane).
 * Refused before anything is enqueued (POMDP_E_BADARG / _BADPARAMS): everything pomdp_controller_episodes refuses; NULL c,
 * action, next or node; NULL action_thr with n_act_cand > 1, NULL next_thr with n_next_cand > 1; n_nodes outside [1, 4096];
 * n_act_cand or n_next_cand < 1; a footprint past the limit; n_obs other than the env's observation count.  k_steps == 0 or
 * n == 0: 0, nothing launched.  The caller's call counter advances by k_steps. */
#define POMDP_STOCH_CONTROLLER_MAX_BYTES 36864
typedef struct pomdp_stoch_controller {
    const int32_t  *action;      /* device [n_nodes][n_act_cand]: the candidate actions of node q */
    const uint32_t *action_thr;  /* device [n_nodes][n_act_cand - 1]; may be NULL when n_act_cand == 1 */
    const int32_t  *next;        /* device [n_nodes][n_obs][n_next_cand]: the candidate successors of node q on observation o */
    const uint32_t *next_thr;    /* device [n_nodes][n_obs][n_next_cand - 1]; may be NULL when n_next_cand == 1 */
    int32_t  n_nodes, n_obs, n_act_cand, n_next_cand;
    int32_t *node;               /* device [n], in/out: lane i's current node */
} pomdp_stoch_controller;
int pomdp_stoch_controller_episodes(const pomdp_episode_args *a, const pomdp_stoch_controller *c,
                                    uint64_t t0, int64_t k_steps, void *stream);

/* Steps per fused launch of the C-side drivers above (pomdp_rollout_synthetic with POMDP_FUSE_STEPS, pomdp_collect_*,
 * pomdp_heuristic_steps): a launch's fixed cost (kernel start, table build, drain) is paid once per this many steps.
 * pomdp_fuse_max(v) sets it for the calling process (1 <= v <= 256; v <= 0 only reads) and returns the previous value;
 * the default is POMDP_FUSE_MAX_DEFAULT.  Results never depend on it. */
#define POMDP_FUSE_MAX_DEFAULT 256
int pomdp_fuse_max(int v);
/* ... and what a trajectory collection of `env` in `layout` really runs per launch: pomdp_fuse_max(), except that the 13-byte
 * layouts (POMDP_LAYOUT_COLUMNS, _BLOCKED) of RockSample, Tag and Tiger stay at 64 — their launches are bound by the store
 * stream, and in a longer launch the waves drift further apart in the rows they write (RockSample 2.09 -> 2.55 us per step of
 * 2^20 lanes at 256 steps per launch); BattleShip and Network gain from the longer launch in every layout. */
int pomdp_fuse_steps(int env, int layout);

/* ---- planner hooks ------------------------------------- */
/* replaces <Env>._generate_legal (rock.py:273-291, tag.py:228-229, battleship.py:157-165, tiger.py:111-112,
 * network.py:130-131): list (device, int32 [n][stride], stride >= the env's action count) receives each
 * lane's legal actions in the reference's list order, padded with -1; len (device, int32 [n]) their number. */
int pomdp_legal_actions(int env, const void *params, const uint32_t *state, int32_t *list, int32_t *len,
                        int64_t n, int stride, void *stream);

/* replaces <Env>._compute_prob(action, next_state, ob) (rock.py:250-264, tag.py:209-217, battleship.py:80-89,
 * tiger.py:125-138, network.py:43-55): the likelihood of observing ob[i] after action[i] led to state column i
 * (BattleShip reads the grid, i.e. the state after the shot, as the reference does).  out: device double[n]. */
int pomdp_compute_prob(int env, const void *params, const uint32_t *state, const int32_t *action, const int32_t *ob,
                       double *out, int64_t n, void *stream);

/* Random rollouts — the simulations a POMCP-style planner runs through _set_state / _generate_legal /
 * step / _discount.  Lane i (global id lane0 + i, i < n_roots * sims_per_root) starts from
 * root_state column i / sims_per_root (uint32 [words][n_roots], read-only) and for k = 0 .. depth-1, while
 * not done:  list = _generate_legal() (all actions with POMDP_ROLLOUT_ALL_ACTIONS);
 *            a = list[(w * len(list)) >> 32], w = word k of stream ROLLOUT at (seed, lane, t0);
 *            (ob, r, done) = step(a) on stream STEP at (seed, lane, t0 + k);  ret += disc * r;  disc *= discount.
 * The return accumulates in IEEE double (separate multiply and add).  Per-lane outputs (device):
 * ret double[n], n_steps / first_action / last_ob int32[n], terminated uint8[n] (first_action = -1 for a simulation
 * that took no step; n_steps, last_ob and terminated may be NULL since ABI 14).  lane0 must be a multiple of 4
 * (RockSample's STEP blocks are shared by global lanes 4 q .. 4 q + 3 and travel within the hardware quad). */
enum { POMDP_ROLLOUT_ALL_ACTIONS = 1 };
int pomdp_rollout(int env, const void *params, const uint32_t *root_state, int64_t n_roots, int64_t sims_per_root,
                  int depth, double discount, int flags, uint64_t seed, uint32_t lane0, uint64_t t0,
                  double *ret, int32_t *n_steps, int32_t *first_action, int32_t *last_ob, uint8_t *terminated,
                  void *stream);

/* ---- the planning step built on those rollouts (ABI 14; BASELINE.json configs[4]: "a POMCP-style 1024-simulation
 * rollout per real step") ------------------------------------------------------------------------------------------
 * What the reference's hooks exist to be driven for (rock.py:243-245 _set_state, 266-291 _get_init_state /
 * _generate_legal, 115 _discount; readme.md:38-41 credits POMCP): the caller simulates from each root, turns the
 * simulations into action values and takes the best action in the real env.  This planner is FLAT Monte Carlo — independent
 * rollouts, no search tree, no UCB: nothing simulation s learns steers simulation s + 1; POMCP's search itself is
 * pomdp_tree_search (below).  Per root r, over its sims_per_root
 * simulations (simulation s of root r is lane r * sims_per_root + s of pomdp_rollout's outputs):
 *     visits[r][a] = the number of simulations whose first action was a
 *     q[r][a]      = (sum of their returns) / visits[r][a]            0.0 where visits == 0
 *     best[r]      = the action with the largest q among those with visits > 0, the lowest index on ties; -1 if none
 *     value[r]     = q[r][best[r]]                                     0.0 if best == -1
 * The reduction stays on the device — one workgroup per root, the root's returns staged through LDS, no atomics — and is
 * IEEE double with a DEFINED summation order, so that a CPU restatement reproduces it bit for bit: the root's simulations
 * are cut into chunks of POMDP_PLAN_CHUNK = 64 by simulation index; within a chunk the returns whose first action is a are
 * added in simulation-index order, starting from +0.0; the chunk sums are then added in chunk order, starting from +0.0;
 * the mean is one division.  Nothing depends on the launch geometry or on how roots are spread over GPUs: a root's
 * simulations are consecutive lanes, so whole roots never straddle a shard.
 * The real step is then pomdp_<env>_step(root_state, action = best, ...) — an ordinary step of n_roots lanes. */
#define POMDP_PLAN_CHUNK 64
typedef struct pomdp_plan_out {
    double  *q;        /* device double [n_roots][stride] */
    int32_t *visits;   /* device int32  [n_roots][stride] */
    int32_t *best;     /* device int32  [n_roots] */
    double  *value;    /* device double [n_roots]; may be NULL */
    int32_t  stride;   /* >= the env's action count (columns past it are left alone) */
    int32_t  reserved;
} pomdp_plan_out;
/* the reduction alone, over per-simulation returns / first actions the caller already has (n_actions <= 255; a
 * first_action outside [0, n_actions) — pomdp_rollout's -1 — counts for no action).  Non-finite returns go through the same
 * additions (+inf and -inf on one action: q = NaN), and `best` compares with >, which is false for NaN either way: a NaN q is
 * taken only as the first visited action, and then stays. */
int pomdp_plan_reduce(const double *ret, const int32_t *first_action, int64_t n_roots, int64_t sims_per_root,
                      int n_actions, const pomdp_plan_out *out, void *stream);
/* pomdp_rollout (same arguments, same lanes, same draws) followed by pomdp_plan_reduce: two launches.  sim_ret /
 * sim_first_action: device double / int32 [n_roots * sims_per_root], the caller's scratch — on return they hold the
 * simulations' returns and first actions, as pomdp_rollout writes them. */
int pomdp_plan(int env, const void *params, const uint32_t *root_state, int64_t n_roots, int64_t sims_per_root,
               int depth, double discount, int flags, uint64_t seed, uint32_t lane0, uint64_t t0,
               double *sim_ret, int32_t *sim_first_action, const pomdp_plan_out *out, void *stream);

/* ---- particle beliefs: the belief a POMCP planner keeps per real episode ---------------------------------------------
 * pomdp_plan plans from the TRUE state of each root (flat Monte Carlo with the hidden state known).  A planner that does not
 * know the hidden state keeps a set of P particles per root instead: after each real step it keeps the particles that, under
 * the real action, reproduce the real observation, redraws the others from them, and plans from the particles.
 * Layout: `particles` is uint32 [words][R * P], the packing of the env's state; column r * P + j is particle j of root r, and
 * its global lane is g = lane0 + r * P + j (lane0 = lane_offset * P for a shard of roots starting at root lane_offset).
 * pomdp_particle_init and pomdp_particle_update require P % 4 == 0, 4 <= P <= 4096, lane0 % 4 == 0 and lane0 + R * P <= 2^32
 * (POMDP_E_BADARG otherwise); P % 4 keeps RockSample's quad-shared STEP blocks inside one root.  pomdp_plan_particles takes
 * the same P rules but its lane0 is the simulations' (below).  Device buffers are the caller's; launches are
 * asynchronous on `stream`; n_match is device int32 [R].
 *
 * Proposal of slot j of root r:
 *   pomdp_particle_update: the result of pomdp_<env>_step(params, that column, action[r], ..., seed, lane g, t, flags = 0)
 *     with the column's done flag clear — the same arithmetic and words as a call of that entry point on the whole R * P array
 *     with action[r] repeated P times (no auto-reset; the state after a terminal step is the terminal state);
 *   pomdp_particle_init: pomdp_<env>_reset at (seed, g, t), with its reset observation.
 * Match rule: a proposal matches when its ob equals ob[r]; when done != NULL, its done flag equals (done[r] != 0); with
 *   POMDP_PARTICLE_MATCH_REWARD, its reward equals reward[r] bit for bit (int32 or float per env, as step writes it).
 *   In init, ob == NULL means that every proposal matches.
 * Resample per root: let m be the number of matching slots and s_0 < ... < s_{m-1} those slots.
 *   m >= 1: a matching slot keeps its own proposal; a non-matching slot j takes the proposal of s_k, k = (w_j * m) >> 32,
 *           w_j = word 0 of block 0 of stream PARTICLE at (seed, g, t) (counter (g, t lo, t hi, POMDP_STREAM_PARTICLE << 24),
 *           as the ROLLOUT words are built);
 *   m == 0: every slot keeps its own proposal, unfiltered — the root is "depleted"; what to do about it is the caller's call;
 *   n_match[r] = m.
 * Roots that are not filtered: in update, a root whose action[r] lies outside [0, n_actions) (a plan's best == -1 included)
 *   gets its particles copied unchanged and n_match[r] = -1; in init, a root with where[r] == 0 (where != NULL) is left
 *   untouched and n_match[r] = -1.
 * particles_out must not overlap particles_in (POMDP_E_BADARG).  reward is required with POMDP_PARTICLE_MATCH_REWARD; done
 * may be NULL.  One launch per call: one 256-thread workgroup per root for P >= 256, 256 / P roots per workgroup below. */
enum { POMDP_PARTICLE_MATCH_REWARD = 1 };
int pomdp_particle_init(int env, const void *params, uint32_t *particles, const int32_t *ob, const uint8_t *where,
                        int32_t *n_match, int64_t n_roots, int n_particles, uint64_t seed, uint32_t lane0, uint64_t t,
                        void *stream);
int pomdp_particle_update(int env, const void *params, const uint32_t *particles_in, uint32_t *particles_out,
                          const int32_t *action, const int32_t *ob, const void *reward, const uint8_t *done,
                          int32_t *n_match, int64_t n_roots, int n_particles, int flags, uint64_t seed, uint32_t lane0,
                          uint64_t t, void *stream);
/* Planning from particles: pomdp_rollout over the R * P particle columns as roots, sims_per_root / P simulations each
 * (sims_per_root a multiple of P), followed by pomdp_plan_reduce over R roots x sims_per_root simulations.  Simulation s of
 * particle p of root r is therefore simulation p * (sims_per_root / P) + s of root r, and its global lane is
 * lane0 + r * sims_per_root + p * (sims_per_root / P) + s with lane0 = lane_offset * sims_per_root, exactly as in pomdp_plan:
 * q / visits / best do not depend on how the roots are sharded.  Requires sims_per_root % P == 0 (sims_per_root >= P),
 * lane0 % 4 == 0 and lane0 + R * sims_per_root <= 2^32; arguments otherwise as pomdp_plan's. */
int pomdp_plan_particles(int env, const void *params, const uint32_t *particles, int64_t n_roots, int n_particles,
                         int64_t sims_per_root, int depth, double discount, int flags, uint64_t seed, uint32_t lane0,
                         uint64_t t0, double *sim_ret, int32_t *sim_first_action, const pomdp_plan_out *out, void *stream);

/* ---- heuristic-policy support --------------------------- */
/* RockSample's per-rock side statistics — the Rock fields count, measured, lkv, lkw, prob_valuable of rock.py:78-86,
 * which RockEnv.step updates on every CHECK (rock.py:177-191) and `_generate_preferred` / `_select_target` read.
 * Device pointers, struct of arrays [num_rocks][n] (rock j of lane i at [j * n + i]). */
typedef struct pomdp_rock_belief {
    int32_t *count;          /* +1 per GOOD reading, -1 per BAD                     rock.py:183,187 */
    int32_t *measured;       /* number of CHECKs of this rock                       rock.py:178 */
    double  *lkv, *lkw;      /* likelihood of the readings if valuable / worthless  rock.py:184-189 */
    double  *prob_valuable;  /* .5 lkv / (.5 lkv + .5 lkw)                          rock.py:190-191 */
    uint32_t *check_ok;      /* [n] derived: bit j = measured[j] < 5 && |count[j]| < 2 && 0 < prob_valuable[j] < 1, the
                                "worth another CHECK" test of rock.py:371.  Maintained by the entry points below so
                                that the policy reads one word per lane instead of 20 bytes per rock; after writing
                                the arrays directly call pomdp_rock_belief_refresh. */
} pomdp_rock_belief;

/* fresh Rock objects (0, 0, 1., 1., .5) for every lane, or for the lanes with where[i] != 0 (device uint8, may be NULL) */
int pomdp_rock_belief_reset(const pomdp_rock_params *p, const pomdp_rock_belief *b, const uint8_t *where, int64_t n,
                            void *stream);
/* recompute check_ok from count / measured / prob_valuable (after the caller overwrote them, e.g. _set_state) */
int pomdp_rock_belief_refresh(const pomdp_rock_params *p, const pomdp_rock_belief *b, int64_t n, void *stream);
/* The part of RockEnv.step that maintains the statistics (rock.py:177-191), run after pomdp_rock_step on its outputs:
 * a lane whose action was CHECK j and whose ob != 0 updates rock j with eff(d) of the stored agent position (CHECK
 * does not move); with POMDP_AUTO_RESET a done lane gets fresh statistics (its reset() built new Rock objects),
 * without it done lanes are left alone. */
int pomdp_rock_belief_update(const pomdp_rock_params *p, const uint32_t *state, const int32_t *action, const int32_t *ob,
                             const uint8_t *done, const pomdp_rock_belief *b, int64_t n, int flags, void *stream);
/* replaces RockEnv._select_target (rock.py:389-399): the nearest (straight-line; the reference's `manhattan_distance`
 * is sqrt(dx^2+dy^2), coord.py:83-85) uncollected rock with count >= 0, lowest index on ties, -1 if none. */
int pomdp_rock_select_target(const pomdp_rock_params *p, const uint32_t *state, const pomdp_rock_belief *b,
                             int32_t *target, int64_t n, void *stream);

/* What `_generate_preferred(history)` reads from the planner's History of Transition(observation, action, reward,
 * next_observation, done) records (rock.py:525-550; tag.py:233-239 reads history.size, history[-1].action and
 * history[-1].ob), kept per lane as running sums so that no list of records has to be walked (a bounded history keeps
 * one byte per record of its window besides, see `ring`).  Device pointers:
 *   size, last_action, last_ob                                                                   int32 [n]
 *   total_sample[j] = sum over CHECK-j transitions of (+1 if next_ob GOOD, -1 if next_ob BAD)     rock.py:303-310
 *   total_move[j]   = sum over CHECK-j transitions of (+1 if next_ob GOOD, else -1 if the *previous*
 *                     observation was BAD — the reference's elif reads transition.observation)    rock.py:327-334
 * the two sums are int32 [num_rocks][n] for RockSample and unused (may be NULL, like move_ok) for the other envs. */
typedef struct pomdp_history {
    int32_t *size, *last_action, *last_ob;
    int32_t *total_sample, *total_move;
    uint32_t *move_ok;      /* [n] derived, RockSample only: bit j = total_move[j] >= 0 (the test of rock.py:335), bit 16 + j
                               = total_sample[j] > 0 (rock.py:311); maintained by pomdp_history_clear / _append /
                               pomdp_heuristic_steps — _generate_preferred reads this word, not the sums */
    /* History(max_size=k) of rock.py:533-544: append() pops the oldest record once the list holds more than k, so the
     * list settles at k + 1 records and the sums above cover that window only.  max_size = -1: unbounded (the reference's
     * default; ring and head may be NULL).  max_size >= 0: `size` stops at max_size + 1; for RockSample the window
     * itself is kept so that a record's contribution can leave the sums again: ring uint8 [max_size + 1][n], one byte per
     * kept transition (action | next_ob << 5 | (observation == BAD) << 7), head int32 [n] = the row the next transition
     * goes to (the oldest one once the ring is full).  Both may be NULL for the other envs. */
    uint8_t *ring;
    int32_t *head;
    int32_t max_size, reserved;
} pomdp_history;

/* History() — empty history for every lane / the lanes with where[i] != 0 (last_action = last_ob = -1) */
int pomdp_history_clear(int env, const void *params, const pomdp_history *h, const uint8_t *where, int64_t n,
                        void *stream);
/* history.append(Transition(observation, action, reward, next_observation, done)) per lane (rock.py:541-544).  With
 * POMDP_AUTO_RESET a done transition ends the episode and the lane's history starts over, empty.
 * Any int32 is taken: last_action / last_ob keep the caller's values, while a bounded RockSample window keeps a record as
 * what the two sums take from it — an action outside [0, 5 + num_rocks) as a non-CHECK (31), a next observation other than
 * 1 or 2 as 0 — so that a record leaves the sums with exactly what it entered them with. */
int pomdp_history_append(int env, const void *params, const pomdp_history *h, const int32_t *observation,
                         const int32_t *action, const int32_t *next_observation, const uint8_t *done, int64_t n,
                         int flags, void *stream);
/* replaces <Env>._generate_preferred(history) (rock.py:293-374 with use_heuristic=True, tag.py:231-243;
 * tiger.py:114-115, network.py:138-139 and BattleShip, which has none, give the legal list).  Output as
 * pomdp_legal_actions: list int32 [n][stride] in the reference's order padded with -1, len int32 [n].
 * b is read for RockSample only. */
int pomdp_preferred_actions(int env, const void *params, const uint32_t *state, const pomdp_rock_belief *b,
                            const pomdp_history *h, int32_t *list, int32_t *len, int64_t n, int stride, void *stream);
/* the caller's `np.random.choice(list)` over per-lane lists (rock.py:564): action[i] = list[i][(w * len[i]) >> 32]
 * with w the synthetic policy's word of (seed, lane0 + i, t) — the word pomdp_synthetic_actions uses; -1 if len[i] == 0 */
int pomdp_pick_actions(const int32_t *list, const int32_t *len, int stride, int32_t *action, int64_t n, uint64_t seed,
                       uint32_t lane0, uint64_t t, void *stream);

/* k_steps consecutive heuristic-policy steps, one launch each: per lane, at call counter t = t0 + s,
 *     a = choice(_generate_preferred(history))      == pomdp_preferred_actions + pomdp_pick_actions(seed, t)
 *     (ob, reward, done) = step(a)                   == pomdp_<env>_step(seed, t)
 *     side statistics, history.append(Transition(prev_ob, a, reward, ob, done))
 *                                                    == pomdp_rock_belief_update + pomdp_history_append
 *     prev_ob <- ob, or what reset() returned on a lane that auto-reset
 * with exactly the results of that five-launch sequence (the rollout loop of rock.py:557-573 for a batch).
 * prev_ob (device int32[n], in/out) starts as the observation reset() returned; action receives the chosen actions
 * (-1 on frozen lanes).  b is read for RockSample only.  The caller's call counter advances by k_steps.
 * `returns` (may be NULL) adds the loop's discounted return, `r += rw * discount; discount *= env._discount`
 * (rock.py:569-570), in IEEE double with separate multiply and add: ret[i] += disc[i] * reward; disc[i] *= discount.
 * When a lane's episode ends, ret_done[i] receives its return; with POMDP_AUTO_RESET ret[i] / disc[i] then restart at
 * 0 / 1 for the new episode, without it they keep the finished episode's values (the lane is frozen).
 * lane0 must be a multiple of 4 (the policy's block is shared by global lanes 4 q .. 4 q + 3). */
typedef struct pomdp_returns {
    double  discount;       /* the env's _discount (rock.py:115, tag.py:91, ...) */
    double *ret, *disc;     /* device double[n], in/out; start them at 0 and 1 */
    double *ret_done;       /* device double[n], out: return of the last finished episode of the lane */
} pomdp_returns;
int pomdp_heuristic_steps(int env, const void *params, uint32_t *state, const pomdp_rock_belief *b, const pomdp_history *h,
                          int32_t *prev_ob, int32_t *action, int32_t *ob, void *reward, uint8_t *done,
                          const pomdp_returns *returns, int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0,
                          int64_t k_steps, int flags, void *stream);

/* pomdp_heuristic_steps with every step kept (added to ABI 15: a new entry point only, nothing existing changes): the same
 * loop on the same arguments leaves, bit for bit, what pomdp_heuristic_steps leaves — state, prev_ob, the history words,
 * sums and ring, RockSample's side statistics and derived words, the last step's action / ob / reward / done, `returns` —
 * and in addition row s of `traj` holds step t0 + s of every lane, in one of the two 4-byte layouts of pomdp_collect_layout:
 *   POMDP_LAYOUT_PACKED   traj uint32 [k_steps][pitch], pitch >= n;
 *   POMDP_LAYOUT_NARROW   traj uint8 [k_steps][4][pitch], pitch >= n and a multiple of 4 (and at most (2^32 - 256) / 3: a
 *                         thread's offset within a row is a 32-bit word); the bytes of the lanes n .. up to the next
 *                         multiple of 4 are written as 0, nothing beyond them is touched.
 * The record of a live lane-step is  action | ob << 8 | reward_code << 16 | done << 24  with the action the policy chose and
 * the reward code of pomdp_collect_layout (Network: the table index).  With POMDP_AUTO_RESET a done row carries the TERMINAL
 * observation, as in every auto-reset sink; the observation the fresh episode starts with is not recorded (it is what
 * prev_ob holds for the lane if the launch ends there, and what reset() of that (seed, lane, t) returns).  Without
 * POMDP_AUTO_RESET a lane whose `done` was set before step s is frozen and its record is 0x010000FF: action byte 0xFF (the -1
 * pomdp_heuristic_steps reports for it; no env has 255 actions), ob 0, reward 0, done 1.
 * POMDP_E_BADARG before any launch: traj == NULL, pitch < n, a NARROW pitch that is not a multiple of 4, any other layout
 * (COLUMNS and BLOCKED included), lane0 % 4 != 0 and everything pomdp_heuristic_steps refuses.  k_steps == 0 is a no-op;
 * longer calls are split at pomdp_fuse_max() steps per launch, and the rows never depend on the split. */
int pomdp_heuristic_collect(int env, const void *params, uint32_t *state, const pomdp_rock_belief *b, const pomdp_history *h,
                            int32_t *prev_ob, int32_t *action, int32_t *ob, void *reward, uint8_t *done,
                            const pomdp_returns *returns, void *traj, int64_t pitch, int layout,
                            int64_t n, uint64_t seed, uint32_t lane0, uint64_t t0, int64_t k_steps, int flags, void *stream);

/* ---- rollouts under the env's preferred-action policy (added to ABI 15: new entry points only, nothing existing changes) --
 * pomdp_rollout with a different list to pick from: POMCP's rollout policy.  The lanes, the ROLLOUT word k that picks, the
 * STEP words at t0 + k, the float64 return (separate multiply and add) and the outputs ret / n_steps / first_action /
 * last_ob / terminated are pomdp_rollout's.  What is new is read-only and indexed by REAL root r < n_roots — it describes
 * what the agent of root r has seen:
 *   b        RockSample / StochasticRock only (NULL otherwise): the side statistics, arrays [num_rocks][n_roots];
 *   h        the history words, arrays [n_roots] and [num_rocks][n_roots]; max_size must be -1 — a bounded history is refused
 *            with POMDP_E_BADARG: a simulation would have to carry the window;
 *   prev_ob  int32 [n_roots], the observation each root saw last (History.prev_ob); RockSample only (may be NULL otherwise).
 * `state` is uint32 [words][n_roots * n_particles].  n_particles = 1: the roots' TRUE states, column r, as in pomdp_rollout /
 * pomdp_plan.  n_particles = P > 1: particle p = (i % sims_per_root) / (sims_per_root / P) of root r, column r * P + p — the
 * lanes of pomdp_plan_particles; sims_per_root must be a multiple of P.  The policy inputs stay per root r either way.
 * Simulation i of root r = i / sims_per_root (global lane lane0 + i) starts from its state column and from PRIVATE copies of
 * root r's statistics, history words and prev_ob, and for k = 0 .. depth-1, while not done:
 *   1. list = _generate_preferred(history): exactly what pomdp_preferred_actions returns for that state, statistics and
 *      history — ascending action order; an empty list falls back to _generate_legal(); for Tiger, Network and BattleShip
 *      the list is the legal list, as it is there; for RockSample the heuristic always applies (use_heuristic is a switch
 *      of the host mirror: an env built without it runs pomdp_rollout);
 *   2. a = list[(w * len(list)) >> 32], w = word k of stream ROLLOUT at (seed, lane, t0);
 *   3. (ob, r, done) = step(a) on stream STEP at (seed, lane, t0 + k), no auto-reset;  ret += disc * r;  disc *= discount;
 *   4. the private copies are updated as one non-auto-reset step of pomdp_heuristic_steps updates a live lane: history
 *      size / last_action / last_ob and both per-rock sums (the prev_ob == BAD rule included); the side statistics on a
 *      CHECK with ob != 0 that did not end the episode; prev_ob <- ob.
 * Nothing of the roots is written.  Results depend neither on the launch geometry nor on how roots are sharded (lane0 % 4
 * == 0, whole roots per shard, as for pomdp_plan).
 * workspace: device, pomdp_rollout_preferred_workspace(...) = 32 * num_rocks * n_roots * sims_per_root bytes (0 for the
 * envs without rocks: pass NULL), 16-byte aligned, the caller's; it need not be initialised and its contents afterwards are
 * unspecified.  A simulation keeps there the per-rock entries its own CHECKs changed (copy on first touch: the first
 * CHECK of rock j reads root r's entry, later ones the simulation's own).
 * One launch; for the envs whose preferred list is the legal list it is pomdp_rollout's kernel over the state columns. */
int64_t pomdp_rollout_preferred_workspace(int env, const void *params, int64_t n_roots, int64_t sims_per_root);
int pomdp_rollout_preferred(int env, const void *params, const uint32_t *state, int64_t n_roots, int n_particles,
                            int64_t sims_per_root, int depth, double discount, const pomdp_rock_belief *b,
                            const pomdp_history *h, const int32_t *prev_ob, void *workspace, uint64_t seed, uint32_t lane0,
                            uint64_t t0, double *ret, int32_t *n_steps, int32_t *first_action, int32_t *last_ob,
                            uint8_t *terminated, void *stream);
/* pomdp_rollout_preferred followed by pomdp_plan_reduce (unchanged) over n_roots roots x sims_per_root simulations: what
 * pomdp_plan (n_particles = 1) and pomdp_plan_particles (n_particles = P) are to pomdp_rollout. */
int pomdp_plan_preferred(int env, const void *params, const uint32_t *state, int64_t n_roots, int n_particles,
                         int64_t sims_per_root, int depth, double discount, const pomdp_rock_belief *b, const pomdp_history *h,
                         const int32_t *prev_ob, void *workspace, uint64_t seed, uint32_t lane0, uint64_t t0, double *sim_ret,
                         int32_t *sim_first_action, const pomdp_plan_out *out, void *stream);

/* ---- POMCP's tree search (added to ABI 15: new entry points only, nothing existing changes) ------------------------------
 * pomdp_plan is flat Monte Carlo: independent rollouts, the mean return by first action.  This is the search POMCP (Silver &
 * Veness, NIPS 2010) builds from the same hooks: a UCB1 tree over action-observation histories, grown by one node per
 * simulation, with a uniform random rollout from each new leaf; many trees side by side, and several independent trees per
 * root merged at the root (root parallelisation: the simulations of one tree are sequential by nature).
 *
 * Lanes.  A search runs R = n_roots roots x W = trees_per_root trees per root; each tree runs S = sims_per_tree simulations of
 *   at most D = depth steps.  Tree w of root r is global lane g = lane0 + r * W + w; lane0 = lane_offset * W for a shard of
 *   roots starting at root lane_offset, and whole roots never straddle a shard, so results do not depend on sharding.
 *   lane0 % 4 == 0 (RockSample's STEP blocks are shared by global lanes 4 q .. 4 q + 3), lane0 + R * W <= 2^32, W >= 1,
 *   S >= 1, D >= 0; also W * S <= 2^31 - 1 (merged visit counts are int32) and (S + 1) * A <= 2^31 - 1.
 * Call counters.  Simulation s of every tree runs at t_s = t0 + s * D; its step k (k = 0 .. D - 1, counted from the root) draws
 *   the env's randomness from stream STEP at (seed, g, t_s + k): exactly what pomdp_<env>_step at that lane and counter draws,
 *   with no auto-reset.  All trees of a launch are at the same (s, k) at the same time, so the counter is uniform across a
 *   wave.  The env's call counter advances by S * D per search; counters wrap mod 2^64 as everywhere else.
 * Start state.  Without particles (particles == NULL, n_particles == 0): column r of root_state (uint32 [words][R]), the true
 *   state, as in pomdp_plan.  With particles (P = n_particles per root, uint32 [words][R * P], column r * P + j: the layout
 *   and the P rules of pomdp_plan_particles; root_state is ignored): particle j = (x * P) >> 32 of root r, x = word 0 of block 0
 *   of stream TREE at (seed, g, t_s) (counter (g, t_s lo, t_s hi, POMDP_STREAM_TREE << 24), as the PARTICLE words are built).
 * A tree is a pool of at most S + 1 nodes; node 0 is the root history.  Every node keeps N(h,a) (int32) and V(h,a) (double) for
 *   each of the env's A actions, all zero at creation.  Children are found by (action, observation), both full int32.  Node
 *   indices are handed out in creation order.  Every search starts from an empty tree (no reuse after the real step).
 * Simulation s, with h = node 0, k = 0 and mode = tree:
 *   1. If k == D, stop.  L = _generate_legal() of the simulated state, in the env's list order (pomdp_legal_actions).  If L is
 *      empty, stop.
 *   2. Tree mode: if some a in L has N(h,a) == 0, take the first such in list order.  Otherwise let Nh = sum of N(h,a) over all
 *      A actions and take the first maximum, in list order, of u(a) = V(h,a) + c * sqrt(logn[Nh] / (double)N(h,a)), c = ucb_c:
 *      one IEEE division, one square root, one multiply and one add, none fused.  logn is the caller's device table, double
 *      [S + 1], logn[n] = log(n) computed on the host (entry 0 is never read): the device never calls log.
 *   3. Rollout mode: a = L[(x * len(L)) >> 32], x = word j of stream ROLLOUT at (seed, g, t_s + k0), k0 = the step index at
 *      which this simulation left the tree, j = k - k0.  The rollout phase draws word for word what a pomdp_rollout simulation
 *      of depth D - k0 from the leaf at t0' = t_s + k0 draws.
 *   4. (o, r, done) = step(a), then k += 1; r is the reward as pomdp_<env>_step writes it (int32 or float), converted to double.
 *      (Network's pomdp_rollout accumulates its reward before the rounding to float: a search's rollout return can differ from
 *      pomdp_rollout's there in the last bits; every other env's rewards are integers.)  Tree mode: push (h, a, r) on the
 *      path.  Rollout mode: acc += disc * r; disc *= discount — separate multiply and add, from acc = 0, disc = 1 at the leaf.
 *   5. If done, stop.
 *   6. Tree mode: if child (h, a, o) exists it becomes h; otherwise it is created — whatever depth remains — and the mode
 *      becomes rollout (k0 = k).
 * Backup.  Rt = acc (0.0 if there was no rollout); walking the path from its deepest entry to the root, for each entry:
 *   Rt = r + discount * Rt (multiply, then add);  N(h,a) += 1;  V(h,a) = V(h,a) + (Rt - V(h,a)) / (double)N(h,a).
 *   The final Rt is sim_ret[s].
 * Per-tree outputs (device; tree i = r * W + w): tree_visits int32 and tree_q double, both [R * W][out.stride]: node 0's N and
 *   V; n_nodes int32 [R * W].  Diagnostics, each may be NULL: sim_ret double [S][R * W], sim_steps int32 [S][R * W] (steps
 *   taken), sim_tree_steps int32 [S][R * W] (of them in tree mode).
 * Merge per root, into `out`:  visits[r][a] = sum over w of N_w(0,a);  q[r][a] = (sum over w of (double)N_w(0,a) * V_w(0,a))
 *   / visits — the sum from +0.0 in ascending w, separate multiply and add — and 0.0 where visits == 0;  best / value by
 *   pomdp_plan_reduce's rule: the largest q among the visited actions, the lowest index on ties, -1 / 0.0 if none.
 * workspace: device, 16-byte aligned, at least pomdp_tree_search_workspace bytes (0 = the shape is refused) for R * W trees:
 *   the node pools, child links and path stacks.  It need not be initialised; its contents afterwards are unspecified.
 * Everything is checked before anything is enqueued (POMDP_E_BADARG / POMDP_E_BADPARAMS): NULL pointers, A > 255, out.stride <
 *   A, a workspace that is too small, the lane rules, ucb_c negative or not finite, P outside pomdp_plan_particles' rules.
 *   n_roots == 0 returns 0 and launches nothing.  Two launches: the search (one lane per tree) and the merge. */
typedef struct pomdp_tree_args {
    int32_t env;              /* POMDP_ENV_* */
    int32_t depth;            /* D */
    const void *params;       /* the env's params struct */
    const uint32_t *root_state;   /* device; read when particles == NULL */
    const uint32_t *particles;    /* device, or NULL: plan from the true states */
    int64_t n_roots;          /* R */
    int32_t n_particles;      /* P; 0 with particles == NULL */
    int32_t trees_per_root;   /* W */
    int64_t sims_per_tree;    /* S */
    double  discount;
    double  ucb_c;
    const double *logn;       /* device double [S + 1] */
    void    *workspace;       /* device */
    uint64_t workspace_bytes;
    int32_t *tree_visits;     /* device int32  [R * W][out.stride] */
    double  *tree_q;          /* device double [R * W][out.stride] */
    int32_t *n_nodes;         /* device int32  [R * W] */
    double  *sim_ret;         /* device double [S][R * W], or NULL */
    int32_t *sim_steps;       /* device int32  [S][R * W], or NULL */
    int32_t *sim_tree_steps;  /* device int32  [S][R * W], or NULL */
    pomdp_plan_out out;       /* the merged result */
    uint64_t seed;
    uint32_t lane0;
    uint32_t reserved;
} pomdp_tree_args;
size_t pomdp_tree_search_workspace(int env, const void *params, int64_t n_trees, int64_t sims_per_tree, int depth);
int pomdp_tree_search(const pomdp_tree_args *a, uint64_t t0, void *stream);

/* ---- the search under the env's preferred-action policy (added to ABI 15: new entry points only, nothing existing changes) --
 * pomdp_tree_search as POMCP runs it on RockSample and Tag: rollouts pick from _generate_preferred(history) and a new node's
 * preferred actions start with a count and a value ("smart tree").  `a` means what it means for pomdp_tree_search, except that
 * a->logn has S + 1 + A * prior_n entries (logn[n] = log(n), entry 0 never read).  Stated as the differences from that
 * contract's numbered steps; every float64 operation is one of its own (no new one is added: a prior is a stored value).
 * Private policy inputs.  At the start of EVERY simulation the lane takes root r's policy inputs, read-only and indexed by real
 *   root r < R as for pomdp_rollout_preferred: size, last_action, last_ob of pol->history for every env; for RockSample also
 *   check_ok (pol->belief), move_ok, prev_ob (pol->prev_ob, int32 [R]) and per rock count, measured, lkv, lkw (pol->belief),
 *   total_sample, total_move (pol->history).  After every executed step 4, in tree mode and in rollout mode alike, the lane
 *   updates its own copies exactly as a simulation of pomdp_rollout_preferred does after its step (its item 4): the history
 *   append and, for an executed CHECK, the two history sums (the prev_ob == BAD rule included) and, with ob != 0 and not done,
 *   the side statistics in pomdp_rock_belief_update's float64 operations and order — one subtraction 1 - eff; lkv *= eff and
 *   lkw *= (1 - eff) for GOOD, the other way round for BAD; prob_valuable = (.5 * lkv) / ((.5 * lkv) + (.5 * lkw)): two more
 *   multiplies, one add, one division, none fused — which only decides the rock's check_ok bit; then prev_ob <- ob.  The roots' arrays are never
 *   written.  The per-rock entries live in pol->workspace, one slot per (rock, tree), copy on first touch; the touched set starts
 *   empty at every simulation: the first CHECK of rock j in simulation s + 1 reads the ROOT's entry, not what simulation s left.
 * Step 3, rollout mode.  The list is _generate_preferred over the private inputs at the simulated state (what
 *   pomdp_preferred_actions returns: ascending action order); where the heuristic's own list is empty, it is _generate_legal().
 *   a = list[(x * len(list)) >> 32] with the same ROLLOUT word x as pomdp_tree_search, keyed at t_s + k0.
 *   Steps 1, 2, 4, 5, 6 and the backup are unchanged; tree-mode selection (step 2) still scans the LEGAL list.
 * Node priors (prior_n > 0).  Let P(h) be the list the creating simulation's next rollout pick would come from: the preferred
 *   list at the post-step state with the post-append private inputs, the fallback to the legal list included.  Every action a of
 *   P(h) starts with N(h,a) = prior_n and V(h,a) = prior_v, every other action with 0 and 0.0, and Nh = sum_a N(h,a) therefore
 *   starts at prior_n * |P(h)|.  Node 0 gets its priors from simulation 0 at its start — from that simulation's start state (its
 *   particle, with particles) and the root's inputs — when D >= 1; with D == 0 nothing is simulated, no priors are set and the
 *   outputs are pomdp_tree_search's.  A node created by a simulation's last step (k0 == D) is left without priors: no simulation
 *   ever selects there.  The backup's V += (Rt - V) / (double)N runs on top of the priors.  tree_visits, tree_q and the merge
 *   include the priors, each tree's own: merged visits count them W times.  Nh indexes logn up to S + A * prior_n.
 * pol->workspace: device, 16-byte aligned, at least pomdp_tree_search_preferred_workspace(env, params, R * W) = 32 * num_rocks
 *   bytes per tree for RockSample and 0 otherwise (pass NULL); it need not be initialised, its contents afterwards are unspecified.
 * Refused with POMDP_E_BADARG / POMDP_E_BADPARAMS before anything is enqueued: everything pomdp_tree_search refuses; pol or
 *   pol->history NULL (or a history with a NULL array the env reads); history->max_size != -1; RockSample without belief,
 *   without prev_ob, or (R > 0) without a workspace, with a misaligned or a short one; prior_n < 0 or > 65535; prior_v not
 *   finite; W * (S + A * prior_n) > 2^31 - 1.
 * Envs without a policy of their own (Tiger, BattleShip, Network): prior_n == 0 forwards to pomdp_tree_search — the same
 *   result bit for bit, pol's pointers ignored; prior_n > 0 is POMDP_E_BADARG (a uniform prior over the legal list steers
 *   nothing).  For RockSample the heuristic always applies, as for pomdp_rollout_preferred.
 * Two launches: the search (one lane per tree) and pomdp_tree_search's merge. */
typedef struct pomdp_tree_policy {
    const pomdp_rock_belief *belief;   /* RockSample: the roots' side statistics; NULL for Tag */
    const pomdp_history     *history;  /* the roots' history sums; max_size must be -1 */
    const int32_t           *prev_ob;  /* RockSample: device int32 [R] */
    void    *workspace;                /* device, 16-byte aligned, uninitialised */
    uint64_t workspace_bytes;
    int32_t  prior_n;                  /* 0 = no priors */
    int32_t  reserved;
    double   prior_v;
} pomdp_tree_policy;
size_t pomdp_tree_search_preferred_workspace(int env, const void *params, int64_t n_trees);
int    pomdp_tree_search_preferred(const pomdp_tree_args *a, const pomdp_tree_policy *pol, uint64_t t0, void *stream);

/* ---- trees kept between searches (added to ABI 15: new entry points only, nothing existing changes) -----------------------
 * POMCP's other half: after the real step (a, o) the child h.a.o of the root becomes the new root, and its statistics and
 * everything below it carry into the next search.  pomdp_tree_search_resume searches from the trees a workspace holds;
 * pomdp_tree_advance copies, per tree, the subtree under the real step into a second workspace.  pomdp_tree_search_resume is
 * the uniform search; pomdp_tree_search_preferred_resume (further below) is the preferred-policy search on the same pools.
 * A kept tree is a pool of C = node_capacity nodes in k->workspace (device, 16-byte aligned, at least
 *   pomdp_tree_keep_workspace(env, params, R * W, C, D) bytes; 0 = the shape is refused: C < 1, C * A > 2^31 - 1, D < 0, more
 *   than any device holds) and a count k->n_nodes[i] (device int32 [R * W]); tree i = r * W + w as for pomdp_tree_search.  The
 *   workspace needs no initialisation where the count says "empty".  Per node the pool holds pomdp_tree_search's N(h,a),
 *   V(h,a), the child links and Nh = the node's visits (sum_a N(h,a) for every node a search made).
 *
 * pomdp_tree_search_resume is pomdp_tree_search with these differences, stated against that contract's numbered steps; every
 * float64 operation is one of its own (no new one is added: a kept statistic is a stored value).
 * Start.  Tree i starts from the k->n_nodes[i] nodes k->workspace holds.  k->n_nodes[i] < 1 means empty: node 0 is cleared
 *   (N = V = 0, no child, Nh = 0) and the count becomes 1.  A count above C is read as C.  a->workspace and a->workspace_bytes
 *   are ignored.
 * Pool.  The pool has C nodes; S may exceed C - 1.
 * Step 6 on a full pool.  If child (h, a, o) does not exist and the tree holds C nodes, no node is created and nothing in the
 *   tree is written; the mode becomes rollout all the same (k0 = k, the rollout words keyed at t_s + k0 from the next step),
 *   and the path pushed so far and the backup are as always.
 * Step 2.  logn has k->logn_len entries (logn[n] = log(n), entry 0 never read) and Nh is clamped to logn_len - 1.  A node's Nh
 *   grows by at most S per search: a table of (searches since the trees were empty) * S + 1 entries is never clamped.
 * Path.  The in-tree steps of a simulation number at most min(D, C): each is taken at an existing node, the child of the one
 *   before.
 * Outputs.  tree_visits and tree_q are node 0's N and V — kept visits included, so visits[r] may exceed W * S; a->n_nodes and
 *   k->n_nodes both receive the trees' sizes afterwards.  The merge is pomdp_tree_search's, unchanged.
 * Anchor.  From empty trees with C = S + 1 and logn_len = S + 1 every output equals pomdp_tree_search's bit for bit.
 * Refused before anything is enqueued (POMDP_E_BADARG / POMDP_E_BADPARAMS): everything pomdp_tree_search refuses except its
 *   workspace and (S + 1) * A rules; k or k->n_nodes NULL; C < 1; C * A > 2^31 - 1; logn_len < 2; W * (logn_len - 1) > 2^31 - 1
 *   (merged visits are int32); with R > 0 a NULL, misaligned or short k->workspace.  n_roots == 0 returns 0.
 * Two launches: the search (one lane per tree) and pomdp_tree_search's merge.
 *
 * pomdp_tree_advance, for tree i of root r (one lane per tree, no atomics; src is only read):
 *   dst->n_nodes[i] = 0 (an empty tree; its pool in dst->workspace is left as it was) if drop != NULL and drop[r] != 0, or
 *   action[r] is outside [0, A), or src->n_nodes[i] < 1, or (node 0, action[r]) has no child with observation ob[r].
 *   Otherwise the subtree rooted at that child is copied into dst, renumbered breadth-first (a Cheney copy): the kept child is
 *   node 0, with observation 0 and no sibling; a node's actions are scanned in ascending order, and the children of one (h, a)
 *   keep their chain order.  Every copied node keeps its N, V, child links (renumbered) and Nh.  dst->n_nodes[i] = the count.
 *   The destination is its own queue: a pending node's source index waits in the node's spare fourth word.
 *   The copy ends and stays inside both pools for arbitrary workspace contents: every index read from memory is clamped
 *   before use, every chain walk is guarded, and the copy stops at C nodes.
 *   action, ob: device int32 [R]; drop: device uint8 [R] or NULL.  depth is the D both workspaces were sized with.
 * Refused before anything is enqueued: NULL params / src / dst / action / ob, an unknown env or bad params, R < 0, W < 1, D < 0,
 *   R * W > 2^32, either descriptor as for pomdp_tree_search_resume (logn_len is not read), src == dst, src->node_capacity !=
 *   dst->node_capacity, workspaces or count arrays that overlap.  n_roots == 0 returns 0.  One launch. */
typedef struct pomdp_tree_keep {
    void    *workspace;       /* device, 16-byte aligned: the kept trees */
    uint64_t workspace_bytes; /* >= pomdp_tree_keep_workspace(...) */
    int32_t *n_nodes;         /* device int32 [R * W], in/out: nodes held by tree i; < 1 = empty tree */
    int64_t  node_capacity;   /* C >= 1: nodes per tree */
    int64_t  logn_len;        /* entries of a->logn; Nh is clamped to logn_len - 1 */
} pomdp_tree_keep;
size_t pomdp_tree_keep_workspace(int env, const void *params, int64_t n_trees, int64_t node_capacity, int depth);
int pomdp_tree_search_resume(const pomdp_tree_args *a, const pomdp_tree_keep *k, uint64_t t0, void *stream);
int pomdp_tree_advance(int env, const void *params, int64_t n_roots, int trees_per_root, int depth,
                       const pomdp_tree_keep *src, const pomdp_tree_keep *dst,
                       const int32_t *action, const int32_t *ob, const uint8_t *drop, void *stream);

/* ---- the preferred-policy search resumed from kept trees (added to ABI 15: one new entry point, nothing existing changes) ---
 * pomdp_tree_search_preferred_resume is pomdp_tree_search_preferred with pomdp_tree_search_resume's differences applied, word
 * for word as stated there with k: Start (tree i starts from the k->n_nodes[i] nodes k->workspace holds; < 1 = empty: node 0 is
 * cleared and the count becomes 1; a->workspace is ignored), Pool (C nodes; S may exceed C - 1), Step 6 on a full pool (no node,
 * nothing written, rollout mode from k0 = k all the same), Step 2 (logn has k->logn_len entries, Nh is clamped to logn_len - 1),
 * Path (at most min(D, C) in-tree steps) and Outputs (tree_visits / tree_q are node 0's N and V, kept visits and priors
 * included; a->n_nodes and k->n_nodes both receive the sizes afterwards).  pomdp_tree_advance is used between searches as it
 * is.  No float64 operation is added: a prior and a kept statistic are stored values.  On top of the two contracts comes one rule.
 * When a node receives priors (prior_n > 0).  A node is UNPRIMED while its stored Nh == 0.  Take an active lane — not done, with
 *   a non-empty list — that is about to choose an action at a node h that exists in its pool: in tree mode before the
 *   selection, or at the first rollout step after it created h, before the pick.  If h is unprimed, h first receives priors from
 *   THIS step's P(h): the preferred list at the lane's current state and private inputs, the fallback to the legal list
 *   included, exactly as pomdp_tree_search_preferred lays them (N = prior_n, V = prior_v on P(h), 0 and 0.0 elsewhere, no
 *   child, Nh = sum_a N(h,a) = prior_n * |P(h)|, an action the list names twice counted once).  Consequences:
 *   - An empty tree's node 0 is primed by the first simulation that takes a step — simulation 0 for RockSample and Tag, whose
 *     lists are never empty — from that simulation's start state (its particle, with particles) and the root's inputs.
 *   - A kept node 0 keeps the N, V and Nh it has and is not primed again.
 *   - A node created by a simulation's last step (k0 == D) stays unprimed in that search, as in pomdp_tree_search_preferred.
 *     After pomdp_tree_advance it sits one level higher; the first later simulation that stands on it primes it then, from
 *     that simulation's state and private inputs.  The search from empty trees never meets this case.
 *   - On a full pool no node exists, so nothing is primed.
 *   - Nh > 0 means "primed or visited": P(h) is non-empty, so priming sets Nh = prior_n * |P(h)| >= 1, and every backup
 *     increments Nh.  No flag word is needed; the node's spare word stays pomdp_tree_advance's.
 *   A node's Nh can reach (searches since the trees were empty) * S + A * prior_n: priors are laid once per node.
 * Private policy inputs are read from the roots at the start of every simulation, exactly as in pomdp_tree_search_preferred;
 *   after a real step the caller's arrays reflect it.  The kept nodes' priors are the stored values their creating (or
 *   priming) simulation laid; they are not recomputed.
 * Anchor.  From empty trees with C = S + 1 and logn_len = S + 1 + A * prior_n every output equals
 *   pomdp_tree_search_preferred's bit for bit, for every D.  With D == 0 nothing is primed.
 * Refused before anything is enqueued (POMDP_E_BADARG / POMDP_E_BADPARAMS): everything pomdp_tree_search_preferred refuses
 *   except its tree workspace and (S + 1) * A rules (and its W * (S + A * prior_n) rule, which the two below replace);
 *   everything pomdp_tree_search_resume refuses about k; logn_len - 1 < A * prior_n + 1; W * (logn_len - 1) > 2^31 - 1.
 *   n_roots == 0 returns 0.
 * Envs without a policy of their own (Tiger, BattleShip, Network): prior_n == 0 forwards to pomdp_tree_search_resume — the
 *   same result bit for bit, pol's pointers ignored; prior_n > 0 is POMDP_E_BADARG.
 * Two launches: the search (one lane per tree) and pomdp_tree_search's merge. */
int pomdp_tree_search_preferred_resume(const pomdp_tree_args *a, const pomdp_tree_policy *pol, const pomdp_tree_keep *k, uint64_t t0,
                                       void *stream);

int         pomdp_abi_version(void);
const char *pomdp_error_string(int code);
/* introspection: the kernel (name<template arguments>, as a profiler shows it) that the calling thread's most recent
 * pomdp_rollout_synthetic(POMDP_FUSE_STEPS) / pomdp_collect_* / pomdp_finish_episodes launch picked for the batch geometry it was given;
 * "" before the first such call.  The string is thread-local and overwritten by the next call. */
const char *pomdp_last_fused_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
