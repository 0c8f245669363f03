// azul_common.hpp -- what every device header of libazulhip.so shares: integer types, status / pool codes, the sizes of the RandomAgent
// weight table, the optional segment stamps, and the few scalar rule helpers that do not depend on how a game is laid out in a wavefront
// (floor penalty, score clamp, complete wall row, column boards, the compact trajectory record, CPython's seeding).
//
// The rules themselves live in ONE place per game shape:
//   azul_selfplay2.hpp + azul_env2.hpp   two players under the reference's rules (GameRunner's shaped reward, opponent loop, reset): the
//                                        benchmarked self-play loop, every two-player rule entry of the C ABI (azul_ops2.hpp) and the env
//                                        side of the policy rollout -- two games per 64-lane wavefront, state in VGPRs
//   azul_rules_x.hpp                     P = 2..4 players, D = 5 or 2 P + 1 displays, the extended rule switches (row N4), built from the
//                                        same wave primitives (half ballots, LDS-crossbar gathers, wall pricing, parallel factory draw)
//   azul_runner.hpp                      GameRunner.step / reset, the agent step, the policy self-play move and the network-opponent
//                                        protocol, ONCE for both shapes: templates over the adaptors az2::Env2 / azx::EnvX
// The __global__ functions are in headers too (azul_selfplay_kernels.hpp; azul_x_kernels.hpp for the rule kernels of the wide record;
// azul_policy.hpp, azul_rollout2.hpp, azul_learner.hpp), so that the emulation below compiles the kernels themselves; azul_kernels.hip
// holds the host side.
// This is gfx950 device code only: there is no CPU execution path in the product (tests/hostcheck/simt emulates the 64 lanes in lockstep to
// run these headers, unmodified, in the build container).
// Reference lines: azulnet/azul.py:184-191 (is_end_of_game), :200-210 (count_floor), :294-295 (score clamp); CPython 3.10 _randommodule.c
// (init_by_array) for random.seed(int) as used at tests/test_azul.py:36, tests/test_game_runner.py:27.
#pragma once
#include <stdint.h>

typedef uint32_t u32;
typedef int32_t  i32;
typedef uint64_t u64;
typedef int64_t  i64;

#if !defined(__HIPCC__)
#error "libazulhip's headers are gfx950 device code: compile with hipcc --offload-arch=gfx950"
#endif
#include <hip/hip_runtime.h>
#define AZ_FN __device__ __forceinline__
// (member functions: __device__ spelled as the attribute it is -- the lockstep emulation makes the keyword a storage class, which a member cannot take)
#define AZ_MEMBER_FN __attribute__((device)) __forceinline__
#define AZ_UNLIKELY(x) __builtin_expect(!!(x), 0)

namespace wv {
AZ_FN u32 lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Where the hardware put this wave: HW_REG_HW_ID (register 4: wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]) and
// HW_REG_XCC_ID (register 20: XCD [3:0]), whole registers through s_getreg_b32 (simm16 = id | offset << 6 | (size - 1) << 11).
// g++ has no such builtin, and the lockstep emulation (tests/hostcheck/simt) runs one wave at a time -- slot 0 of nowhere: there the read is
// a constant 0, chosen by `if constexpr` (the call sits in a template with a type-dependent argument, so g++ never looks the name up).
// LOCKSTEP_EMULATION is told from the clock builtin's type: gfx950's s_memtime returns unsigned long, the emulation's stand-in is the literal
// 0ull.  azul_kernels.hip asserts that the product is compiled with it false: the device build cannot fall back to the constant.
template <class A, class B> struct same_type { static constexpr bool value = false; };
template <class A> struct same_type<A, A> { static constexpr bool value = true; };
constexpr bool LOCKSTEP_EMULATION = same_type<decltype(__builtin_amdgcn_s_memtime()), unsigned long long>::value;
template <int SIMM16> struct HwReg { static constexpr int value = SIMM16; };
template <class R> AZ_FN u32 getreg(R)
{
    if constexpr (LOCKSTEP_EMULATION) return 0u;
    else return __builtin_amdgcn_s_getreg(R::value);
}
AZ_FN u32 hw_id() { return getreg(HwReg<(4 | (31 << 11))>()); }
AZ_FN u32 hw_xcc_id() { return getreg(HwReg<(20 | (31 << 11))>()); }
// THE TWO WAVES OF A SIMD TAKE TURNS AT PRIORITY 1.  The self-play kernels run one-wave workgroups, two resident per SIMD for the whole
// launch (the registers allow no third), and at equal priority the SIMD's issue arbitration favours the older wave on every conflict:
// measured per wave (tools/wave_timeline.py, profiles/wave_timeline_before.txt) the older one left its 512-move loop after 0.67 of the
// younger one's time, which then ran on alone at a single wave's issue rate -- and the launch ends with the last wave.  A static
// priority for either slot only swaps the roles (no gain); what wins is alternation: the kernels' counted loop is a nest, and at the head
// of every block of PRIO_BLOCK moves a wave sets priority 1 or 0, starting from bit 0 of its hardware wave slot (the two waves of a SIMD
// sit in slots 0 and 1) and flipping each block.  Nothing is added inside a move.  Grids that backfill are not slowed by it
// (profiles/launch_tail_ab.txt).  s_setprio takes an immediate and ignores EXEC: `hi` must be wave-uniform (a scalar branch).
constexpr int PRIO_BLOCK = 128;    // 64: -4.4 %, 96: -6.9 %, 128: -8.1 %, 192: -9.0 %, 256: -7.7 % launch time at 4096 games x 512 moves
AZ_FN void set_prio(bool hi) { if (hi) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
} // namespace wv

namespace az {

enum { ST_OK = 0, ST_ILLEGAL_MOVE = 1, ST_GAME_ENDED = 2, ST_STUCK = 3, ST_BAD_ACTION = 4, ST_BOX_EMPTY = 5,
       ST_TRUNCATED = 6 /* move limit (beyond the reference, off by default): the episode was cut at the end of a round */ };
enum { POOL_RANDOM = 0, POOL_LID = 1 };
#ifndef AZ_DRAW_MARGIN
#define AZ_DRAW_MARGIN 8192ull      // factory draw: > 21.1 * 255, the largest possible fp64 disagreement window
#endif
enum { T_ROWS = 31, T_BINADES = 8, T_STRIDE = 9 /* pairs per row: eight binades + the floor-only pair */, T_PAIRS = T_ROWS * T_STRIDE };   // RandomAgent weight table of the 180-action game: 31 rows (J = 0..30 legal floor moves), see azul_tables.hpp

// ---- optional in-kernel segment stamps (diagnostic build only: -DAZ_PROFILE_SEGMENTS; cdna_hip_programming.md 7) ----
// s_memtime deltas are accumulated per segment and added to a global buffer when the wave ends.  The real kernel
// contains no stamp; never quote the diagnostic build's run time, only its SHARES (tools/segment_profile.py).
enum { SEG_MASK = 0, SEG_SAMPLE, SEG_MOVE, SEG_AFTERMOVE, SEG_TAIL, SEG_NEWROUND, SEG_SCORE, SEG_RESET, SEG_LOOP, SEG_COUNT };
constexpr int AZ_PROF_SLOTS = 48;   // u64 slots of BatchDev::prof: the self-play kernel's SEG_COUNT segments, the rollout kernel's phases (0..8) and matrix sub-phases (16..31)
// The same build also writes ONE RECORD PER WAVE of a self-play launch (tools/wave_timeline.py): AZ_WAVE_REC_WORDS u64 at wave_prof[8 x
// logical wave], lane 0, plain vector stores --
//   [0..3] s_memtime at kernel entry, at loop start, at loop end, after rng2_close      [4] blockIdx.x | HW_REG_HW_ID << 32
//   [5] HW_REG_XCC_ID | logical wave << 32      [6] round ends | rounds dealt << 32      [7] episode resets | regenerations << 32
// (the four counts are GAME-moves of the wave's two games that took the rare block)
enum { WCNT_ROUND_END = 0, WCNT_DEAL, WCNT_RESET, WCNT_COUNT };
constexpr int AZ_WAVE_REC_WORDS = 8;
#if defined(AZ_PROFILE_SEGMENTS)
struct SegProf { u64 last; u64 acc[SEG_COUNT]; u32 cnt[WCNT_COUNT]; };
// `cond` is uniform over each 32-lane half: the ballot's population / 32 is the number of the wave's games it holds for
#define AZ_COUNT(which, cond) do { if (prof_) prof_->cnt[which] += (u32)__popcll(__builtin_amdgcn_ballot_w64(cond)) >> 5; } while (0)
struct WaveStamps { u64 entry, loop_start, loop_end; };
#define AZ_WAVE_STAMP(field) (wstamps.field = __builtin_amdgcn_s_memtime())
// (null-safe: callers outside the self-play kernels pass no SegProf -- an unguarded store would be undefined behaviour, which the
// compiler is free to "optimise" into dropping the code behind the stamp: such a build ran the policy rollout 26 % faster, and wrong)
#define AZ_STAMP(seg) do { if (prof_) { u64 now_ = __builtin_amdgcn_s_memtime(); prof_->acc[seg] += now_ - prof_->last; prof_->last = now_; } } while (0)
#else
struct SegProf { int unused; };
#define AZ_STAMP(seg) do { } while (0)
#define AZ_COUNT(which, cond) do { } while (0)
#define AZ_WAVE_STAMP(field) do { } while (0)
#endif

struct Rules {
    u32 first_player;   // 0 = "Random", 1..2 = fixed
    u32 tile_pool;      // POOL_RANDOM / POOL_LID
};

// wall cells lying in board column `col` (walls are colour-indexed like the reference's: bit 5 r + c sits in board column (c + r) % 5)
constexpr u32 column_board_c(int col)
{
    u32 m = 0;
    for (int j = 0; j < 5; j++) m |= 1u << (5 * j + ((col - j + 5) % 5));
    return m;
}
static_assert(column_board_c(0) == 0x222201u && column_board_c(4) == 0x111110u, "column boards");

AZ_FN i32 floor_penalty(u32 floor_tiles)
{
    u32 f = floor_tiles > 7u ? 7u : floor_tiles;         // count_floor, azul.py:200-210: 0,-1,-2,-4,-6,-8,-11,-14
    return -(i32)((0x0e0b080604020100ull >> (8u * f)) & 0xffu);
}

AZ_FN i32 clamp0(i32 s) { return s < 0 ? 0 : s; }       // azul.py:294-295

AZ_FN bool any_row_full(u32 w) { return ((w & (w >> 1) & (w >> 2) & (w >> 3) & (w >> 4)) & 0x108421u) != 0u; }     // azul.py:184-191

AZ_FN u32 byte_sum5(u64 v)
{
    // (no eight-bit limit on the sum: a bag refilled from the lid holds five bytes of up to 255 tiles each)
    const u32 lo = (u32)v, s = (lo & 0x00ff00ffu) + ((lo >> 8) & 0x00ff00ffu);
    return (s & 0xffffu) + (s >> 16) + ((u32)(v >> 32) & 0xffu);
}

// compact trajectory record of one move (what the multi-GPU all-gather ships): action (0xff = none) | done << 8 | reward << 16
AZ_FN u32 pack_move(i32 a, u32 dn, i32 reward) { return ((u32)(a >= 0 ? a : 0xff) & 0xffu) | ((dn & 0xffu) << 8) | (((u32)reward & 0xffffu) << 16); }

// ---- random.seed(int): CPython init_by_array over the 32-bit words of the seed (one stream per THREAD) ----
AZ_FN void seed_stream(u32 *mt, u64 seed)
{
    u32 key0 = (u32)(seed & 0xffffffffu), key1 = (u32)(seed >> 32);
    u32 len = key1 ? 2u : 1u;
    u32 prev = 19650218u;
    mt[0] = prev;
    for (u32 i = 1; i < 624u; i++) { prev = 1812433253u * (prev ^ (prev >> 30)) + i; mt[i] = prev; }   // init_genrand
    u32 i = 1, j = 0;
    prev = mt[0];
    for (u32 k = 624u; k; k--) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + (j ? key1 : key0) + j;
        mt[i] = prev;
        i++; j++;
        if (i >= 624u) { mt[0] = prev; i = 1; }
        if (j >= len) j = 0;
    }
    for (u32 k = 623u; k; k--) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - i;
        mt[i] = prev;
        i++;
        if (i >= 624u) { mt[0] = prev; i = 1; }
    }
    mt[0] = 0x80000000u;
}

// ---- flat self-play (host side): which trajectory streams a launch writes -> the <OUT, PAD, BITS> of the kernel that writes them, for
// both record families (the selectors: selfplay2_kernel in azul_selfplay_kernels.hpp, x_selfplay_kernel in azul_x_kernels.hpp).
// none: no stream at all; core: mask, action, reward, done and packed without the records; full: core + the mask bits; pad: mask rows
// that take the one-store-per-row path.  OUT 2 is the run-time subset.
struct SelfplayVariant { int out; bool pad, bits; };
static SelfplayVariant selfplay_variant(bool none, bool core, bool full, bool pad)
{
    if (none) return {0, false, false};
    if (full && pad) return {1, true, true};
    if (core && pad) return {1, true, false};
    if (full) return {1, false, true};
    return {2, false, false};
}

} // namespace az
