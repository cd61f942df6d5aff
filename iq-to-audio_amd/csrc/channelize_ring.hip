// channelize_ring.hip -- int8-MFMA channelizer with a block-wide contiguous LDS-DMA ring (gfx950).
//
// Same mathematics, tap fragments, accumulators and emission as channelize_mfma.hip (reference
// processing.py:268-279, 289-297, 325-346, 354-360); what changes is how the capture reaches the matrix
// cores.  The kernels of channelize_mfma.hip let every lane (or every group of four lanes) fetch its own
// row, so one wave-instruction touches 16-64 different 416-byte rows: measured, that address pattern alone
// caps the data path at ~3.8 TB/s.  Here the block streams the capture exactly as it lies in memory:
//
//   * the data columns a block needs are ONE contiguous run of the capture; it is cut into tiles of 32 rows
//     (32*D frames) and copied into LDS slots by global_load_lds_dwordx4 in chunks of 1 KiB per
//     wave-instruction (64 lanes x 16 consecutive bytes): 8-9 cache lines per instruction instead of 64;
//   * 8 waves, two per SIMD.  Wave (rt, cp): rt = one of the four tap-row tiles (32 of the 128 rows),
//     cp = column-tile parity.  A round = two column tiles (cp 0/1); the four waves of a parity read the
//     same slot (ds_read_b128 at row stride 4*D) and each multiplies it with ITS 32 tap rows, whose
//     fragments (8*KS registers) stay in registers for the whole block -- no tap traffic through LDS;
//   * ring of R rounds (as many as LDS holds, <= 5): the DMAs of round r+R-1 are issued during round r, one
//     per k step, by two waves of each parity (one issuing wave per SIMD), behind a counted s_waitcnt vmcnt;
//     one s_barrier per round publishes the landed slots and frees the oldest;
//   * the sums live in a 512-position sliding window (one int32 = 256*S1 + S2 per component): a round's
//     scatter reaches 127 positions ahead, the 64 outputs completed two rounds ago are converted, rotated
//     and stored by one wave while the others multiply, and their slots are reused 8 rounds later.  So a
//     block is not bounded by LDS: every CU gets ONE contiguous range of the launch (persistent blocks:
//     one prologue per CU, 63 rows of halo per CU).
//
// Round 3: up to 13 k steps (and in every row-staged int16 kernel) LOADER WAVES feed the ring: they fetch the tiles into
// registers, split every int16 into its high byte and its biased low byte once per tile and write two byte planes per slot;
// the multiplying waves read their MFMA operands as they lie in LDS (RingGeo::SPLIT says what that bought).  The ring of
// such a kernel is two slots per parity in LDS plus two rounds (lane pairs: three) of loads in the loaders' registers; the
// loaders also emit.  The text above describes the LDS-DMA form, which remains at 14..16 k steps (the multiplying waves
// issue the DMAs) and for uint8 captures (two loader waves issue them, ring_loader).  Up to 8 k steps a row whose last k
// step is at most half full (the ..._half kernels, D = 104 among them) runs on v_mfma_i32_16x16x64_i8 instead of 32x32x32:
// the same tile per wave as four 16x16 blocks, the two off-diagonal ones in one accumulator, an odd last k step as seven
// 16x16x32 (ring_main_h16) -- equal cycles per product, but at its power limit the chip holds a higher clock on that shape.
// Round 7: in launches of a single lane the loaders of the contiguous slots fetch with non-temporal loads (ring_load16; the
// stream alone 6.0 -> 6.6 TB/s, probe/stream_probe.hip); the stream's phase against a 16-byte boundary costs nothing, aligned
// loads with the shift done in registers and a second pass through LDS were slower.
// Round 8: single-lane launches of the ..._half kernels whose lane carries rotated fragments (zrot) do not multiply the
// all-zero high tap bytes of the filter's edge rows (ring_main_h16_light; 15 % less matrix-pipe time, 0.7 % at the step).
// The forms measured against these and rejected are recorded in DESIGN.md section 6.
//
// Every launch goes through the lane table of mfma_ring_launch_multi (k_channelize_mfma_s16_ring_multi / _multi_half /
// _pairs, ..._s16_ring_rows_multi, ..._u8_ring_rows_multi): a single-channel pass (iqa_channelize_mfma) is a launch of one
// lane, 8 * ceil(ranges / 8) workgroups.  So traces name no kernel of their own for single channels or for the short
// mixer-sign probes; the probes are the launches with a small grid.
//
// A contiguous slot is 1024*(2*KS + 1) bytes >= 32 rows at a pitch of D/4 (+1) 16-byte units (KS = ceil(2D/32) k steps;
// the K padding of the last k step reads on into the next row, against zero taps); a tile takes 2*KS + 1 DMA
// instructions; it needs D % 4 == 0 (16-byte aligned rows for ds_read_b128) and KS <= 16.
// Every other decimation (odd D, D > 256 in several k-step ranges) uses row-staged slots, see RingGeo.
#include "mfma_common.h"

#include <atomic>
#include <mutex>
#include <cmath>
#include <type_traits>

namespace iqa {

typedef __attribute__((address_space(3))) void ring_lds_t;

constexpr int RG_WAVES = 8;

constexpr int RG_MAX_KS = 16;
constexpr int RG_ROWS_MAX_KS_C = 11;  // most k steps a pass of the row-staged kernels takes
constexpr int RG_W = 512;      // sliding window of output sums (positions mod 512), per component
constexpr int RG_GUARD = 64;   // a tile's scatter reaches at most 59 positions past its lane base: aliases of slots 0..63
constexpr int RG_AS = RG_W + RG_GUARD;
constexpr int RG_ACC_BYTES = 2 * RG_AS * 8;  // sized for the 64-bit sums; the 32-bit form uses half of it
constexpr int RG_EMIT_WAVE = 2;  // (rt 2, parity 0): not an issuing wave
// Parity-1 waves scatter a tile one round late (at the start of the next round, while their SIMD partner of parity 0
// is already multiplying -- the two waves of a SIMD then alternate between the matrix pipe and the LDS instead of
// meeting in both), so a group of 64 outputs is final three rounds after its first tile.
constexpr int RG_EMIT_LAG = 3;
constexpr unsigned int RG_PACE_AHEAD = 2;  // publications (of every second round) a workgroup may be in front of its range's slowest
constexpr int RG_PACE_SPINS = 20000;
constexpr int RG_PACE_WORDS = 16384;       // words of the pacing buffer: ranges x units of a launch must fit
constexpr int RG_PAIR_IDLE = 1 << 28;  // MfmaArgs::pair_shift of the half of a pair that has no lane
// Loader waves (extra waves that feed the ring and emit) up to this many k steps; 14..16 k steps need more registers than
// twelve waves leave each other (168), there the multiplying waves issue LDS-DMAs themselves.  Banks at 9..16 k steps run
// as lane pairs, so this concerns the kernels with one lane per workgroup.
constexpr int RG_LOADERS_MAX_KS = 13;
constexpr int RG_ROUNDS_MAX = 5;  // ring depth of the one-lane-per-workgroup kernels in rounds of two tiles, where LDS allows it
// Ring depth of the lane-pair kernel in rounds (2..5).  Its speed does not depend on it (2, 3, 5: 9.19 / 9.08 / 9.08 ms at
// config 3); at 3 a workgroup leaves 59 KB of a CU's LDS to the small kernels of the previous capture's tail (the resampler
// wants 20), at 5 only 3.
constexpr int RG_PAIR_ROUNDS = 3;
constexpr int RG_PD = 2;  // k steps the fragment reads run ahead of the MFMAs

// One LDS-DMA instruction: 64 lanes x 16 bytes, global -> LDS (global_load_lds_dwordx4).  The 16-byte form exists on
// gfx950 only; the HOST pass of the compilation checks the builtin's size argument against ITS target and, inside
// function templates, turns that into spurious "no matching function" errors -- it never needs the body.  Default cache
// policy: the others (nt, sc1, sc0 sc1, sc1 nt) measured the same.
__device__ __forceinline__ void ring_dma16(const void *src, ring_lds_t *dst)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
#else
    (void)src;
    (void)dst;
#endif
}

__device__ __forceinline__ unsigned lds_addr(const void *p)
{
    return static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)p));
}

// Two ways a tile (32 data rows) sits in a ring slot:
//   contiguous (ROWS = false): the 32*D frames of the tile, one contiguous run of the capture, fetched by 2*KS + 1
//     DMA instructions of 1 KiB (64 lanes x 16 bytes) -- needs 16-byte aligned rows (D % 4 == 0) and all k steps of a
//     row in one pass (KS <= 16).  In LDS the rows sit at a pitch of an ODD number of 16-byte units (the row's own D/4
//     units, plus one of padding when that is even): the fragment reads of a wave -- ds_read_b128, lane = row, served
//     in four groups of 16 lanes -- then touch 16 different bank quads per group.  At the capture's own pitch they are
//     2-way conflicts at D = 104 and 4-way at D = 208 (16 LDS cycles per wave-instruction instead of 4: with 26 of them
//     per wave and tile the LDS, not the matrix pipe, bounded a CU as soon as the data came from L2).  An LDS-DMA lane
//     writes to (instruction base + 16 * lane) but fetches from any address, so the padding costs nothing but the
//     per-lane source offsets (`ring_src_off`, computed once per workgroup);
//   row-staged (ROWS = true): row j's k-step range of THIS pass, 64*KS bytes, at a pitch of 64*KS + 16 bytes (16 bytes
//     of padding: rows 4 banks apart, conflict-free reads), filled 64 units per DMA instruction like the contiguous slots (RingGeo::NI_ROWS).  Any D, and the
//     k-step ranges of a long row (D = 521: 33 k steps in three passes of 11) each fetch only their own third of every
//     row, so three passes read the capture about once instead of three times.  Always with loader waves.
// U8 (row-staged only): uint8 I/Q captures -- a k step is 32 bytes of a row, one 16-byte fragment per lane, the
// offset-binary bytes become int8 with one XOR, and there is a single data piece: two MFMAs per k step (q1*v, q2*v).
// PAIR (contiguous slots only): the workgroup holds TWO lanes -- the four waves of parity 0 the tap
// rows of one, the four of parity 1 those of the other -- and all eight read the SAME staged tile: one tile per round
// instead of two, so the ring is twice as deep in rounds at the same LDS (five rounds instead of two at 13 k steps: the
// refill of a slot has four rounds to land instead of one) and a tile crosses L2 -> LDS once per two lanes; two windows
// of sums.  The lanes of a pair share their tap-row group index (the staged stream depends on it).
// H16 (single lanes over contiguous byte-plane slots): the kernels whose multiplying waves work on 16x16x64 matrix tiles
// (ring_main_h16); their planes have a pitch of their own.
template <int KS, bool ROWS, bool U8 = false, bool PAIR = false, bool H16 = false>
struct RingGeo {
    static_assert(ROWS || !U8, "uint8 captures use row-staged slots");
    static_assert(!PAIR || (!ROWS && !U8), "lane pairs: contiguous slots only");
    static_assert(!H16 || (!ROWS && !U8 && !PAIR && KS <= 8), "16x16x64 tiles: single lanes, contiguous byte-plane slots, up to 8 k steps");
    static constexpr int TPR = PAIR ? 1 : 2;  // tiles per round
    static constexpr int ACCS = PAIR ? 2 : 1;  // windows of sums
    static constexpr int KBYTES = U8 ? 32 : 64;  // bytes of a row per k step
    static constexpr int PITCH = KBYTES * KS + 16;
    static constexpr bool PADDED = KS <= 13;  // contiguous slots: rows at an odd pitch in LDS (conflict-free fragment reads)
    static constexpr int NI = 2 * KS + 1;  // contiguous slots: 1 KiB DMA instructions per tile (32 rows at a padded pitch)
    // row-staged slots are filled like the contiguous ones: 64 consecutive 16-byte units of the slot per DMA instruction,
    // every lane fetching ITS unit from wherever it lies in the capture (unit q = unit q % UNITS_ROW of row q / UNITS_ROW; a
    // row's padding unit and the units behind row 31 re-fetch a neighbour) -- 32 (4 KS + 1) / 64 instructions per tile
    // instead of one per row with 4 KS of 64 lanes active (2 k steps: 5 instead of 32)
    static constexpr int UNITS_ROW = PITCH / 16;
    static constexpr int NI_ROWS = (32 * UNITS_ROW + 63) / 64;
    static constexpr int SLOT_RAW = ROWS ? (32 * PITCH > 1024 * NI_ROWS ? 32 * PITCH : 1024 * NI_ROWS) : 1024 * NI;
    // extra waves that feed the ring and emit (a wave then has 168 registers).  Lane pairs: up to 13 k steps -- four loader
    // waves share the round's ONE tile, the first two emit a lane each
    static constexpr bool LOADERS = (!PAIR && (ROWS || KS <= RG_LOADERS_MAX_KS)) || (PAIR && KS <= 13);
    // byte-plane staging (every int16 kernel with loader waves): a slot is [high bytes: 32 rows at PLANE_PITCH][biased low
    // bytes: ditto], the same 1024 * NI bytes; the pitch is an odd number of 16-byte units (conflict-free ds_read_b128, lane =
    // row).  FOUR loader waves, two per parity (wave `half` of a parity takes the tile's 1 KiB pieces 2 j + half, j < KS),
    // SPLIT_F rounds of loads in flight in their registers (4 KS SPLIT_F of them), two slots per parity in LDS (one read, one
    // written).  With raw tiles in LDS each of a parity's four multiplying waves split the same fragment again: 12 VALU
    // instructions per k step and wave beside 3 MFMAs, 8.5 % of config 2's kernel time
    // (profiles/r03_sustained_ablation_splits.txt).
    static constexpr bool SPLIT = LOADERS && !U8;
    // H16: lane l reads row l & 15 at unit 4 c + (l >> 4) of its row (ds_read_b128 serves lanes {0-3, 12-15, 20-27}, ... in one
    // LDS cycle each): an odd pitch is a 2-way conflict for that pattern, a pitch of 4 n + 2 units -- 2 KS for odd KS, 2 KS + 2
    // for even -- puts the 16 lanes of a group on 16 different bank quads
    static constexpr int PLANE_PITCH = H16 ? 32 * (KS + 1 - (KS & 1)) : 32 * KS + 16;
    // (a loader wave has 168 registers: 4 KS SPLIT_F of data, 2 KS of offsets, the emission.)  Single lanes: two rounds in
    // flight -- config 2's kernel measures the same with three (profiles/r03b_ab_rounds_in_flight.txt), and with two a
    // workgroup of the 7-k-step kernel leaves room for the 80-register kernels of a capture's tail
    static constexpr int SPLIT_F = PAIR ? 3 : 2;
    static constexpr int NLOADERS = SPLIT ? 4 : (LOADERS ? 2 : 0);
    static constexpr int SLOT = SPLIT ? 64 * PLANE_PITCH : SLOT_RAW;
    static constexpr int NDMA = ROWS ? NI_ROWS : (LOADERS ? NI : KS + 1);  // DMAs per issuing wave and round
    static constexpr int FIT = (160 * 1024 - ACCS * RG_ACC_BYTES) / (TPR * SLOT);
    static constexpr int RMAX = 63 / NDMA + 2;  // (R - 2) * NDMA must fit the 6-bit vmcnt
    static constexpr int R0 = FIT < RMAX ? FIT : RMAX;
    static constexpr int RCAP = PAIR ? RG_PAIR_ROUNDS : RG_ROUNDS_MAX;
    static constexpr int R = SPLIT ? 2 : R0 > RCAP ? RCAP : (R0 < 2 ? 2 : R0);  // rounds (of two tiles; PAIR: of one) the ring holds
    static constexpr int THREADS = (RG_WAVES + NLOADERS) * kWave;
    static constexpr int LDS_BYTES = R * TPR * SLOT + ACCS * RG_ACC_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "ring + window exceed LDS");
    static_assert((R - 2) * NDMA <= 63, "vmcnt is a 6-bit counter");
};

struct RingCtx {
    char *smem;
    int *s_acc;           // [Sre | Sim], RG_AS entries each, output position p at slot p mod RG_W.  ACC64: one int64
                          // S1*2^32 + S2 per entry (16-bit taps, exact); else one int32 256*S1 + S2 (~14-bit taps)
    const char *stream0;  // row-staged slots: this lane's source byte of row 0 of tile 0; contiguous: tile 0's first byte
    long long tile_bytes, i0, m0;
    int tiles, rounds, cnt, lane_off, rt, cp, col, h, lane;
    int row_units, pitch_units;  // contiguous slots: 16-byte units per data row in the capture / in LDS (odd)
    int tshift;  // lane pairs: this wave's own tile t is the staged tile of round t + tshift (0 without pairs)
};

// Source offset (bytes from the tile's first byte) of the 16 bytes lane `lane` of DMA instruction `idx` fetches: the
// instruction fills LDS units 64*idx .. 64*idx + 63 of the slot, unit q holds unit q % pitch of row q / pitch; the
// padding unit of a row and the units behind row 31 re-fetch a neighbour (they are read, if at all, against zero taps).
__device__ __forceinline__ int ring_src_off(int idx, int lane, int row_units, int pitch_units)
{
    const int q = 64 * idx + lane;
    int r = q / pitch_units;
    int u = q - r * pitch_units;
    if (r > 31) {
        r = 31;
        u = row_units - 1;
    }
    return (r * row_units + min(u, row_units - 1)) * 16;
}

// Emission state of the emitting wave: lane l owns position 64 k + 1 + l of group k; its rotation advances by
// the host-computed step of 64 outputs per group (float64 recurrence, ~1e-16 per step).
struct RingEmit {
    double wc, ws;
};

// A group of 64 finished outputs leaves the window in two steps, so that the multiplying wave that also emits (the
// kernels without loader waves) can put its own matrix work between them: `ring_emit_load` reads the sums out of the
// window (and the partial sums of earlier passes out of memory) and clears the slots; `ring_emit_store` -- a dozen
// k steps later, when those reads have long returned -- scales, rotates and stores.  Back to back they are the one-step
// emission of the loader waves.  (Done in one piece at the top of a round, the chain LDS read -> wait -> float64 maths ->
// store made the emitting wave ~500 cycles late for its tile, and seven waves waited for it at every barrier.)
struct RingEmitRegs {
    double v_re, v_im;  // 256*S1 + S2 per component
    double2 pr;         // partial sums of the earlier passes (0 when there are none)
    int i;              // output index inside the block
};

template <bool ACC64, bool EARLY>
__device__ __forceinline__ void ring_emit_load(const MfmaArgs &a, const RingCtx &c, int k, RingEmitRegs &g)
{
    const int pos = 64 * k + 1 + c.lane;
    g.i = pos - MF_Q;
    const int s = pos & (RG_W - 1);
    if constexpr (ACC64) {
        long long *acc = reinterpret_cast<long long *>(c.s_acc);
        long long sr = acc[s], si = acc[RG_AS + s];
        if (s < RG_GUARD) {
            sr += acc[RG_W + s];
            si += acc[RG_AS + RG_W + s];
            acc[RG_W + s] = 0;
            acc[RG_AS + RG_W + s] = 0;
        }
        acc[s] = 0;  // the slot is scattered into again 8 rounds from now
        acc[RG_AS + s] = 0;
        // the adds were (S1 << 32) + sign-extended S2: the low word is S2 itself (|S2| < 2^31), the rest is S1
        const int s2r = static_cast<int>(sr), s2i = static_cast<int>(si);
        const long long s1r = (sr - s2r) >> 32, s1i = (si - s2i) >> 32;
        g.v_re = static_cast<double>(s1r) * 256.0 + static_cast<double>(s2r);
        g.v_im = static_cast<double>(s1i) * 256.0 + static_cast<double>(s2i);
    } else {
        int *acc = c.s_acc;
        int sr = acc[s], si = acc[RG_AS + s];
        if (s < RG_GUARD) {
            sr += acc[RG_W + s];
            si += acc[RG_AS + RG_W + s];
            acc[RG_W + s] = 0;
            acc[RG_AS + RG_W + s] = 0;
        }
        acc[s] = 0;
        acc[RG_AS + s] = 0;
        g.v_re = static_cast<double>(sr);
        g.v_im = static_cast<double>(si);
    }
    g.pr = make_double2(0.0, 0.0);
    // EARLY: the earlier passes' partial sums are requested here, a dozen k steps before they are used (the emitting
    // MULTIPLYING wave: it issues no LDS-DMAs, a wait for this load costs it nothing).  A loader wave must not: the wait
    // for the load would be a vmcnt(0) in the middle of its counted DMA sequence -- the whole ring drained once per round
    // (measured: 0.653 against 0.585 ms at D = 104).  It loads them where it uses them, inside the branch.
    if constexpr (EARLY) {
        if (a.partial_in != nullptr && g.i >= 0 && g.i < c.cnt) g.pr = a.partial_in[c.i0 + g.i];
    }
}

template <bool EARLY>
__device__ __forceinline__ void ring_emit_store(const MfmaArgs &a, const RingCtx &c, RingEmit &e, const RingEmitRegs &g)
{
    const int i = g.i;
    if (i >= 0 && i < c.cnt) {
        double d_re = mfma_scaled_sum(g.v_re, a.c_re, a.unit);
        double d_im = mfma_scaled_sum(g.v_im, a.c_im, a.unit);
        if (a.partial_in != nullptr) {
            const double2 pr = EARLY ? g.pr : a.partial_in[c.i0 + i];
            d_re = __dadd_rn(d_re, pr.x);
            d_im = __dadd_rn(d_im, pr.y);
        }
        if (!a.finalize) {
            if (a.raw_partials)  // the integer sums themselves (exact: int32 by construction); iqa_mfma_combine scales them
                reinterpret_cast<int2 *>(a.partial_out)[c.i0 + i] = make_int2(static_cast<int>(g.v_re), static_cast<int>(g.v_im));
            else
                a.partial_out[c.i0 + i] = make_double2(d_re, d_im);
        } else {
            a.out[c.i0 + i] = mfma_finish(d_re, d_im, a.conj_sum, a.rotate, e.wc, e.ws, a.sc_re, a.sc_im);
        }
    }
    const double nc = e.wc * a.rot64_re - e.ws * a.rot64_im;
    e.ws = fma(e.wc, a.rot64_im, e.ws * a.rot64_re);
    e.wc = nc;
}

template <bool ACC64>
__device__ __forceinline__ void ring_emit_group(const MfmaArgs &a, const RingCtx &c, RingEmit &e, int k)
{
    RingEmitRegs g;
    ring_emit_load<ACC64, false>(a, c, k, g);
    ring_emit_store<false>(a, c, e, g);
}

template <int KS, bool ROWS, bool U8, bool PAIR = false>
__device__ __forceinline__ void ring_wait_and_barrier(int younger)
{
    // an issuing wave's DMAs of round r have landed once only those of the younger rounds are outstanding
    using G = RingGeo<KS, ROWS, U8, PAIR>;
    constexpr int R = G::R, N = G::NDMA;
    if (R >= 5 && younger == 3) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(R >= 5 ? 3 * N : 0) : "memory");
    else if (R >= 4 && younger == 2) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(R >= 4 ? 2 * N : 0) : "memory");
    else if (R >= 3 && younger == 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(R >= 3 ? N : 0) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
}

// A loader wave of the uint8 kernels (row-staged slots, LDS-DMA; the int16 kernels stage byte planes, ring_loader_split),
// parity cp: per round, wait for its DMAs of this round, join the barrier, refill the slot the previous round has left
// with the tile R-1 rounds ahead, and emit the group of 64 outputs that became complete two rounds ago when that group's
// parity is its own.
template <int KS, bool ACC64>
__device__ __forceinline__ void ring_loader(const MfmaArgs &a, const RingCtx &c)
{
    using G = RingGeo<KS, true, true>;
    constexpr int R = G::R, SLOT = G::SLOT;
    const int cp = c.cp;
    int soff[G::NI_ROWS];
    const int row_bytes = static_cast<int>(c.tile_bytes >> 5);
#pragma unroll
    for (int i = 0; i < G::NI_ROWS; ++i) {
        const int q = 64 * i + c.lane;
        int r = q / G::UNITS_ROW;
        int u = q - r * G::UNITS_ROW;
        if (r > 31) {
            r = 31;
            u = G::UNITS_ROW - 2;
        }
        soff[i] = r * row_bytes + min(u, G::UNITS_ROW - 2) * 16;  // (the last data unit again for the padding unit)
    }
    auto issue_tile = [&](int tile, int slot) {
        const char *src = c.stream0 + static_cast<long long>(min(tile, c.tiles - 1)) * c.tile_bytes;
        char *dst = c.smem + (slot * 2 + cp) * SLOT;
#pragma unroll
        for (int i = 0; i < G::NI_ROWS; ++i)
            ring_dma16(src + soff[i], (ring_lds_t *)(dst + i * 1024));
    };
#pragma unroll
    for (int rr = 0; rr < R - 1; ++rr) issue_tile(2 * rr + cp, rr);
    RingEmit em{1.0, 0.0};
    double st_re = a.rot64_re * a.rot64_re - a.rot64_im * a.rot64_im, st_im = 2.0 * a.rot64_re * a.rot64_im;  // 128 outputs
    if (a.finalize && a.rotate) {
        const unsigned long long m = static_cast<unsigned long long>(c.m0 + (64 * cp + 1 + c.lane - MF_Q));  // group cp
        const unsigned long long ph = a.rot_base + m * a.rot_step;
        sincospi(2.0 * (static_cast<double>(ph >> 11) * (1.0 / 9007199254740992.0)), &em.ws, &em.wc);
    }
    MfmaArgs a2 = a;  // ring_emit_group advances the rotation by (rot64_re, rot64_im): this wave owns every other group
    a2.rot64_re = st_re;
    a2.rot64_im = st_im;
    int slot = 0;
    for (int r = 0; r < c.rounds; ++r) {
        ring_wait_and_barrier<KS, true, true>(min(R - 2, c.rounds - 1 - r));
        if (r + R - 1 < c.rounds) issue_tile(2 * (r + R - 1) + cp, (slot == 0) ? R - 1 : slot - 1);
        if (r >= RG_EMIT_LAG && ((r - RG_EMIT_LAG) & 1) == cp) {
            // every wave has ISSUED the LDS adds of its round r-2 tile before this barrier (parity 1 defers a tile's
            // adds to the start of the next round); a wave has at most 15 LDS operations outstanding and they complete
            // in order, so the adds of the tiles of round r-3 and earlier -- everything that reaches positions
            // <= 64 (r-2) -- have landed.
            asm volatile("" ::: "memory");
            ring_emit_group<ACC64>(a2, c, em, r - RG_EMIT_LAG);
            asm volatile("" ::: "memory");
        }
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int k_last = (c.cnt + 62) >> 6;
    for (int k = max(c.rounds - RG_EMIT_LAG, 0); k <= k_last; ++k)
        if ((k & 1) == cp) ring_emit_group<ACC64>(a2, c, em, k);
}

// A loader wave of the byte-plane kernels (RingGeo::SPLIT): parity cp, half `half`.  Round r: behind the barrier it waits
// for ITS pieces of the tile of round r + 1 (requested SPLIT_F rounds ago), splits them and writes the planes of slot
// (r + 1) % 2 -- the slot round r - 1 has just left --, requests the tile of round r + 1 + SPLIT_F into the registers that
// became free, and (half 0) emits like ring_loader.  Loads into registers (contiguous slots, launches of a single lane: nt,
// ring_load16): the compiler counts vmcnt itself, the emission's store included.  Pieces beyond the tile's last unit (a tile
// is D / 8 pieces, a wave pair fetches 2 KS) re-fetch the last unit and are not written.
struct __attribute__((packed, aligned(4))) ring_raw16 {  // 16 bytes of the capture: dword-aligned (the stream starts at frame row*D + 1)
    int x, y, z, w;
};
typedef int ring_raw16v __attribute__((ext_vector_type(4), aligned(4)));  // the same for __builtin_nontemporal_load

// NT: global_load_dwordx4 nt -- the contiguous slots' stream in launches of a SINGLE lane (the kernel variants ONCE: one
// workgroup streams each range, every byte is fetched once by the whole launch).  Alone, with config 2's loader geometry,
// the stream runs at 6.6 TB/s with it against 6.1 without (probe/stream_probe.hip, profiles/r07_stream_probe.txt).  Where
// several lanes' workgroups stream the same range the later ones are meant to hit in L2, and nt loads cost config 3's pair
// launches 3 %: those, and the row-staged kernels, keep the default policy.  A variant and
// not a kernel argument: a uniform branch between the two forms of the requests cost the loaders of 10 - 13 k steps 8 - 190
// bytes of scratch and every kernel its load schedule (config 2 +14 us, config 4's unit 1.10 -> 1.66 ms).
template <bool NT>
__device__ __forceinline__ int4 ring_load16(const char *p)
{
    if constexpr (NT) {
        const ring_raw16v t = __builtin_nontemporal_load(reinterpret_cast<const ring_raw16v *>(p));
        return make_int4(t.x, t.y, t.z, t.w);
    } else {
        const ring_raw16 t = *reinterpret_cast<const ring_raw16 *>(p);
        return make_int4(t.x, t.y, t.z, t.w);
    }
}

// PAIR: the four loader waves (HALF 0..3) share the round's one tile, piece 4 j + HALF each; waves 0 and 1 emit lane 0's and
// lane 1's outputs (c.cp = the lane; a, c.s_acc, c.tshift are that lane's), every group of their lane.
template <int KS, bool ACC64, bool ROWS, int HALF, bool PAIR = false, bool H16 = false, bool NT = false>
__device__ __forceinline__ void ring_loader_split(const MfmaArgs &a, const RingCtx &c)
{
    static_assert(!NT || (!ROWS && !PAIR), "nt loads: the single-lane kernels over contiguous slots");
    constexpr bool EMITTER = PAIR ? HALF < 2 : HALF == 0;
    // pieces of a tile this wave takes: every second one, or -- from 12 k steps on, where 8 KS registers of data in flight
    // and the emission's float64 state do not fit one wave -- the emitting wave (half 0) the first KS - 2, the other the rest
    constexpr bool UNEVEN = !PAIR && KS >= 12;
    constexpr int P0 = KS >= 12 ? KS - 2 : KS;
    constexpr int STRIDE = PAIR ? RingGeo<KS, ROWS, false, PAIR>::NLOADERS : 2;
    constexpr int NP = UNEVEN ? (HALF ? 2 * KS - P0 : P0) : (2 * KS + STRIDE - 1) / STRIDE;
    auto piece = [](int j) { return UNEVEN ? (HALF ? P0 + j : j) : STRIDE * j + HALF; };
    using G = RingGeo<KS, ROWS, false, PAIR, H16>;
    constexpr int SLOT = G::SLOT, PP = G::PLANE_PITCH, F = G::SPLIT_F;
    const int cp = c.cp;
    // 16-byte units of a data row that are staged: the whole row (contiguous slots: rows follow one another in the capture)
    // or this pass's 4 KS units of it (row-staged slots); a tile is 32 rows of them, unit q = unit q % upr of row q / upr
    const int upr = ROWS ? 4 * KS : c.row_units;
    const int row_bytes = static_cast<int>(c.tile_bytes >> 5);
    // piece j of this wave is unit q = 64 piece(j) + lane = unit u of row `row`.  Up to 8 k steps its source and
    // destination offsets sit in two tables; longer rows keep 16 bits (row, u) per piece and spend a few
    // VALU instructions on them -- 2 KS registers the loader does not have beside 8 KS of data in flight.  (Walking (row, u) from
    // piece to piece instead, with its lane-divergent carry loop, made the loaders the slowest waves of the workgroup:
    // 1.55 against 1.09 ms at 13 k steps.)
    constexpr bool TABLE = KS <= 8;
    int doff[TABLE ? NP : 1], soff[TABLE ? NP : 1];
    unsigned rowu[TABLE ? 1 : (NP + 1) / 2];  // two pieces per word: u (6 bits: a row holds <= 64 units), row (5), "not written" (1)
    if constexpr (!TABLE) {
#pragma unroll
        for (int j = 0; j < (NP + 1) / 2; ++j) rowu[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int q = 64 * piece(j) + c.lane;
        const int row = q / upr, u = q - row * upr;
        if constexpr (TABLE) {
            doff[j] = row < 32 ? row * PP + 8 * u : -1;
            soff[j] = row < 32 ? row * row_bytes + 16 * u : 31 * row_bytes + 16 * (upr - 1);
        } else {
            const unsigned f = row < 32 ? static_cast<unsigned>((row << 6) | u) : static_cast<unsigned>((31 << 6) | (upr - 1) | (1 << 11));
            rowu[j >> 1] |= f << (16 * (j & 1));
        }
    }
    int4 buf[F][NP];
    auto request = [&](int round, auto set) {
        constexpr int S = decltype(set)::value;
        // (PAIR: the stream runs on past this lane's own last tile for the partner that works pair_extra rounds behind)
        const char *src = c.stream0 + static_cast<long long>(PAIR ? min(round, c.rounds - 1) : min(2 * round + cp, c.tiles - 1)) * c.tile_bytes;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            int so;
            if constexpr (TABLE) so = soff[j];
            else {
                const unsigned f = rowu[j >> 1] >> (16 * (j & 1));
                so = static_cast<int>((f >> 6) & 31u) * row_bytes + 16 * static_cast<int>(f & 63u);
            }
            buf[S][j] = ring_load16<NT>(src + so);
        }
    };
    auto stage = [&](int slot, auto set) {
        constexpr int S = decltype(set)::value;
        char *hi0 = c.smem + (PAIR ? slot : slot * 2 + cp) * SLOT;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int4 d = buf[S][j];
            int2 hi, lo;
            hi.x = __builtin_amdgcn_perm(d.y, d.x, 0x07050301);
            hi.y = __builtin_amdgcn_perm(d.w, d.z, 0x07050301);
            lo.x = __builtin_amdgcn_perm(d.y, d.x, 0x06040200) ^ 0x80808080;
            lo.y = __builtin_amdgcn_perm(d.w, d.z, 0x06040200) ^ 0x80808080;
            int dq;
            if constexpr (TABLE) dq = doff[j];
            else {
                const unsigned f = rowu[j >> 1] >> (16 * (j & 1));
                dq = (f & 2048u) ? -1 : static_cast<int>((f >> 6) & 31u) * PP + 8 * static_cast<int>(f & 63u);
            }
            if (dq >= 0) {
                *reinterpret_cast<int2 *>(hi0 + dq) = hi;
                *reinterpret_cast<int2 *>(hi0 + 32 * PP + dq) = lo;
            }
        }
    };
    // prologue: the tile of round 0 into slot 0 (before the block's first barrier), rounds 1 .. F requested
    request(0, std::integral_constant<int, 0>{});
    stage(0, std::integral_constant<int, 0>{});
    request(1, std::integral_constant<int, 1 % F>{});
    request(2, std::integral_constant<int, 2 % F>{});
    if constexpr (F == 3) request(3, std::integral_constant<int, 0>{});
    static_assert(F == 2 || F == 3, "the prologue and the unrolled loop below are written for two or three rounds in flight");
    RingEmit em{1.0, 0.0};
    double st_re = a.rot64_re * a.rot64_re - a.rot64_im * a.rot64_im, st_im = 2.0 * a.rot64_re * a.rot64_im;  // 128 outputs
    if (EMITTER && a.finalize && a.rotate) {
        const unsigned long long m = static_cast<unsigned long long>(c.m0 + ((PAIR ? 0 : 64 * cp) + 1 + c.lane - MF_Q));  // its first group
        const unsigned long long ph = a.rot_base + m * a.rot_step;
        sincospi(2.0 * (static_cast<double>(ph >> 11) * (1.0 / 9007199254740992.0)), &em.ws, &em.wc);
    }
    MfmaArgs a2 = a;  // ring_emit_group advances the rotation by (rot64_re, rot64_im): without pairs this wave owns every other group
    if constexpr (!PAIR) {
        a2.rot64_re = st_re;
        a2.rot64_im = st_im;
    }
    // the group of 64 outputs this wave emits in round r, or -1.  PAIR: a lane's group k (its tiles 2k, 2k + 1) in round
    // 2k + 5 (lane 0) / 2k + 6 (lane 1) of the lane's own count, as ring_main's emitting waves did
    auto group_of = [&](int r) {
        if constexpr (PAIR) {
            const int re = r - c.tshift, lag = 5 + cp;
            return (re >= lag && ((re - lag) & 1) == 0) ? (re - lag) >> 1 : -1;
        } else {
            return (r >= RG_EMIT_LAG && ((r - RG_EMIT_LAG) & 1) == cp) ? r - RG_EMIT_LAG : -1;
        }
    };
    // The partial sums of the earlier passes (a long row's k-step ranges) are requested ONE ROUND AHEAD of their emission and
    // in front of that round's tile request: loads return in order, so waiting for a load issued behind the tile requests
    // -- where the emission uses it -- would wait for every tile in flight: the prefetch drained every other round.
    // (Up to 11 k steps; at 12 and 13 the four registers are not there, and the partial sums are loaded where they are used.)
    constexpr bool PR_AHEAD = PAIR || KS <= 11;
    double2 pr_next = make_double2(0.0, 0.0);
    auto round_body = [&](int r, auto set) {
        // (the planes of round r were written before this barrier: lgkmcnt(0) in front of it)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (r + 1 < c.rounds) stage((r + 1) & 1, set);
        const double2 pr_now = pr_next;
        if (PR_AHEAD && EMITTER && a.partial_in != nullptr) {
            const int kn = group_of(r + 1);
            if (kn >= 0) {
                const int i = 64 * kn + 1 + c.lane - MF_Q;
                pr_next = (i >= 0 && i < c.cnt) ? a.partial_in[c.i0 + i] : make_double2(0.0, 0.0);
            }
        }
        request(r + 1 + F, set);  // (beyond the last tile: the last tile again, never staged)
        const int k = EMITTER ? group_of(r) : -1;
        if (k >= 0) {
            asm volatile("" ::: "memory");
            if constexpr (PR_AHEAD) {
                RingEmitRegs g;  // (see ring_loader for why these sums are final)
                ring_emit_load<ACC64, false>(a2, c, k, g);
                g.pr = pr_now;
                ring_emit_store<true>(a2, c, em, g);
            } else {
                ring_emit_group<ACC64>(a2, c, em, k);
            }
            asm volatile("" ::: "memory");
        }
    };
    // round r stages the tile of round r + 1, which sits in register set (r + 1) % F
    int r = 0;
    if constexpr (F == 3) {
        for (; r + 3 <= c.rounds; r += 3) {
            round_body(r, std::integral_constant<int, 1>{});
            round_body(r + 1, std::integral_constant<int, 2>{});
            round_body(r + 2, std::integral_constant<int, 0>{});
        }
        if (r < c.rounds) {
            round_body(r, std::integral_constant<int, 1>{});
            if (r + 1 < c.rounds) round_body(r + 1, std::integral_constant<int, 2>{});
        }
    } else {
        for (; r + 2 <= c.rounds; r += 2) {
            round_body(r, std::integral_constant<int, 1>{});
            round_body(r + 1, std::integral_constant<int, 0>{});
        }
        if (r < c.rounds) round_body(r, std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if constexpr (EMITTER) {
        const int k_last = (c.cnt + 62) >> 6;
        if constexpr (PAIR) {
            const int own = c.rounds - c.tshift, lag = 5 + cp;  // rounds in this lane's own count
            const int k_next = own > lag ? ((own - 1 - lag) >> 1) + 1 : 0;
            if (c.tshift < RG_PAIR_IDLE)  // (the idle half of a pair without a second lane emits nothing)
                for (int k = k_next; k <= k_last; ++k) ring_emit_group<ACC64>(a2, c, em, k);
        } else {
            for (int k = max(c.rounds - RG_EMIT_LAG, 0); k <= k_last; ++k)
                if ((k & 1) == cp) ring_emit_group<ACC64>(a2, c, em, k);
        }
    }
}

// The main loop of a multiplying wave.  ISSUER (kernels without loader waves): this wave also feeds the ring
// (chunks 2i + (rt & 1) of its parity's slot).  EMIT (ditto): this wave also converts, rotates and stores the 64
// outputs that became complete two rounds ago.
// SKIP: what this wave does with the q2*hi product (the third matrix instruction of a k step): 0 = always computes it;
// 2 = never (its lane's low tap byte is zero throughout: the first lane of a "fine" / "full" tap-row group); 1 = asks the
// lane's flag at run time (both bodies in the code: ~30 registers more, so only the kernels of such launches carry it).
template <int KS, bool ACC64, bool ROWS, bool U8, bool ISSUER, bool EMIT, bool DEFER, bool PAIR, typename SKIPT>
__device__ __forceinline__ void ring_main(const MfmaArgs &a, const RingCtx &c, const v4i_t (&fq)[KS][2], SKIPT)
{
    constexpr int SKIP = SKIPT::value;
    using G = RingGeo<KS, ROWS, U8, PAIR>;
    constexpr int R = G::R, SLOT = G::SLOT;
    static_assert(!(ROWS && ISSUER), "row-staged slots are always fed by loader waves");
    // PAIR: round r works on tile r (both parities: two lanes' tap rows), whose slot is ring slot r mod R; a lane's group k
    // of 64 outputs (tiles 2k, 2k + 1) is emitted by that lane's emitting wave in round 2k + 5 (parity 0) / 2k + 6 (parity
    // 1): the two lanes' emissions fall into alternate rounds
    const int RG_EMIT_LAG_PAIR = 5 + c.cp;  // (PAIR only)
    const int rt = c.rt, cp = c.cp;
    // the two issuing waves of a parity share the tile's 2*KS + 1 DMA instructions: wave p = rt & 1 issues numbers
    // p, p + 2, ...; both issue KS + 1 (the counted s_waitcnt wants one number for both), so the odd wave's last one
    // repeats the even wave's last (same bytes to the same place)
    // Source offsets of this wave's KS + 1 instructions: a table in registers where the rows are padded (G::PADDED);
    // the longest rows (KS >= 14, already at the 256-register limit -- a spill would put scratch loads into the vmcnt
    // sequence the counted waits rely on) keep the capture's own pitch: unit q of the slot is unit q of the tile.
    int soff[(ISSUER && G::PADDED) ? KS + 1 : 1];
    if constexpr (ISSUER && G::PADDED) {
#pragma unroll
        for (int i = 0; i <= KS; ++i) soff[i] = ring_src_off(min(2 * i + (rt & 1), 2 * KS), c.lane, c.row_units, c.pitch_units);
    } else {
        soff[0] = c.lane * 16;
    }
    const int odd_kib = (rt & 1) * 1024;
    auto issue = [&](int tile, int slot, int i) {  // `i` is a compile-time constant at every call site
        // (PAIR: the stream runs on past this lane's own last tile for the partner that works pair_extra rounds behind)
        const char *tile0 = c.stream0 + static_cast<long long>(min(tile, (PAIR ? c.rounds : c.tiles) - 1)) * c.tile_bytes;
        char *slot0 = c.smem + (PAIR ? slot : slot * 2 + cp) * SLOT;
        const int at = (i < KS) ? odd_kib + i * 2048 : 2 * KS * 1024;  // instruction numbers p, p + 2, ..., then 2*KS
        if constexpr (ISSUER && G::PADDED) {
            ring_dma16(tile0 + soff[i], (ring_lds_t *)(slot0 + at));
        } else {
            ring_dma16(tile0 + soff[0] + at, (ring_lds_t *)(slot0 + at));
        }
    };
    if (ISSUER) {
#pragma unroll
        for (int rr = 0; rr < R - 1; ++rr)
#pragma unroll
            for (int i = 0; i <= KS; ++i) issue(PAIR ? rr : 2 * rr + cp, rr, i);
    }
    RingEmit em{1.0, 0.0};
    if (EMIT && a.finalize && a.rotate) {
        const unsigned long long m = static_cast<unsigned long long>(c.m0 + (1 + c.lane - MF_Q));  // group 0
        const unsigned long long ph = a.rot_base + m * a.rot_step;
        sincospi(2.0 * (static_cast<double>(ph >> 11) * (1.0 / 9007199254740992.0)), &em.ws, &em.wc);
    }
    const v16i_t zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // diagonal scatter of a finished tile into the window of sums (row = q, column = data row: output = row + column).
    // Written as inline asm on purpose: the compiler drains vmcnt to 0 before any LDS store it can see while LDS-DMAs
    // are in flight (it cannot tell the ring from the window), which would serialise the whole prefetch pipeline once
    // per round.  These adds touch the window only, never the ring.
    auto scatter = [&](int t, const v16i_t &acc1, const v16i_t &acc2) {
        const int slot_idx = ((t * 32 + c.col + 4 * c.h + 1) & (RG_W - 1)) + (rt >> 1) * RG_AS + (rt & 1) * 32;
        if constexpr (ACC64) {
            // exact for 16-bit taps: ONE 64-bit add of (S1 << 32) + sign-extended S2 per element (3 dwords through the
            // LDS data path instead of 2 x 2 for separate S1/S2 adds); the carry out of the low word is undone at emission
            const unsigned p = lds_addr(reinterpret_cast<long long *>(c.s_acc) + slot_idx);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const long long comb = (static_cast<long long>(acc1[q]) << 32) + static_cast<long long>(acc2[q]);
                const int off = 8 * ((q & 3) + 8 * (q >> 2));
                asm volatile("ds_add_u64 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(off));
            }
        } else {
            const unsigned p = lds_addr(c.s_acc + slot_idx);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                // 256*S1 + S2 in ONE int32 (the host bounds the tap magnitudes so that this cannot overflow for any
                // input, dsp_plan.plan_mfma(acc32=True)); the shift-add is a VALU op the compiler can see, so the
                // MFMA -> VALU hazard distance is its business and the asm reads a VALU result
                const int comb = (acc1[q] << 8) + acc2[q];
                const int off = 4 * ((q & 3) + 8 * (q >> 2));
                asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(off));
            }
        }
    };
    // Parity-1 waves scatter a tile at the start of the next round (DEFER).  Not in the byte-plane kernels: with three waves
    // per SIMD and no byte splits it buys nothing, and its 32 held registers made the 64-bit-sum lane pairs spill
    // (profiles/r03_ab_defer.txt)
    constexpr bool DEFER_ADDS = DEFER && !G::SPLIT;
    v16i_t held1 = zero16, held2 = zero16;  // DEFER_ADDS: the previous tile's sums, scattered at the start of the next round
    int held_t = -1;
    int slot = 0;
    bool pace_on = PAIR && a.pace != nullptr && a.pace_units > 1 && c.rounds < 8000;  // (12 bits of publication count)
    for (int r = 0; r < c.rounds; ++r) {
        if (ISSUER) ring_wait_and_barrier<KS, ROWS, U8, PAIR>(min(R - 2, c.rounds - 1 - r));
        else asm volatile("s_barrier" ::: "memory");
        if constexpr (PAIR && !ISSUER && !EMIT && !DEFER) {
            // Pacing (wave rt 3 of parity 0: no counted waits of its own to disturb).  The workgroups of a range share the
            // capture through their XCD's L2, which at this rate keeps a line for ~10 us = a few rounds; single-lane
            // workgroups stay that close by themselves (the one in front misses in L2 and waits for HBM, the others hit),
            // a pair's DMAs are off its critical path and nothing holds the workgroups of a range together: 1.9x - 4.3x
            // the capture in HBM reads.  So every second round a workgroup publishes its round and the one that is more
            // than RG_PACE_AHEAD publications in front of the slowest STARTED workgroup of its range waits for it -- the
            // slowest never waits, a workgroup that has not started is not waited for: no cycle.
            if (c.rt == 3 && c.cp == 0 && pace_on && (r & 1) == 0) {  // (every second tile)
                const unsigned int mine = static_cast<unsigned int>(r >> 1);
                if (c.lane == 0) __hip_atomic_store(a.pace + a.pace_slot, (a.pace_token << 12) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (int spin = 0;; ++spin) {
                    unsigned int q = mine;
                    if (c.lane < a.pace_units) {
                        const unsigned int v = __hip_atomic_load(a.pace + (a.pace_slot - a.pace_slot % a.pace_units) + c.lane, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT);
                        if ((v >> 12) == a.pace_token) q = v & 0xFFFu;
                    }
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) q = min(q, static_cast<unsigned int>(__shfl_xor(static_cast<int>(q), o, kWave)));
                    q = static_cast<unsigned int>(__builtin_amdgcn_readfirstlane(static_cast<int>(q)));
                    if (mine <= q + RG_PACE_AHEAD) break;
                    if (spin >= RG_PACE_SPINS) {  // (a peer that stopped moving: do without)
                        pace_on = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(32);
                }
            }
        }
        const bool pf = ISSUER && (r + R - 1 < c.rounds);
        const int pf_tile = PAIR ? r + R - 1 : 2 * (r + R - 1) + cp;
        const int pf_slot = (slot == 0) ? R - 1 : slot - 1;  // the slot round r-1 has just left
        // The refill of that slot goes out FIRST, all KS + 1 instructions of it, before this round's matrix work: at
        // 13 k steps the ring holds two rounds only, so a DMA issued late in round r (one per k step, as this loop used
        // to do) had to land before the barrier of round r + 1 -- its whole L2/HBM latency, ~1000 cycles of a ~2500-cycle
        // round, stood exposed at every barrier (measured on the five-target launch: the matrix pipe 52 % busy with no
        // bank conflict and the LDS 23 % busy).  Issued here, a refill has the whole round to land.
        if (pf) {
#pragma unroll
            for (int i = 0; i <= KS; ++i) issue(pf_tile, pf_slot, i);
        }
        const int re = r - c.tshift;  // PAIR: the round in this lane's own count (its tile(s) of round re are staged now)
        const bool emit_now = EMIT && (PAIR ? (re >= RG_EMIT_LAG_PAIR && ((re - RG_EMIT_LAG_PAIR) & 1) == 0) : re >= RG_EMIT_LAG);
        RingEmitRegs eg;
        if (emit_now) {
            asm volatile("" ::: "memory");
            // see ring_loader for why these sums are final (PAIR: the group's last tile was round r - 4's, whose adds --
            // deferred by one round at most -- went out before the barrier of round r - 2)
            ring_emit_load<ACC64, true>(a, c, PAIR ? (re - RG_EMIT_LAG_PAIR) >> 1 : re - RG_EMIT_LAG, eg);
            asm volatile("" ::: "memory");
        }
        if (DEFER_ADDS && held_t >= 0) {
            scatter(held_t, held1, held2);
            held_t = -1;
        }
        bool store_pending = emit_now;  // the emitting wave finishes its group inside its tile of the round
        // This wave's one tile of the round.  (A loop of one iteration: without it the compiler orders the tile's address
        // arithmetic differently and 62 of the kernels come out with other registers and schedules.)
#pragma unroll
        for (int j = 0; j < 1; ++j) {
        const int t = PAIR ? re : 2 * r + cp;
        if (t >= 0 && t < c.tiles) {
            const bool store_here = store_pending;
            store_pending = false;
            const char *la = c.smem + (PAIR ? slot : slot * 2 + cp) * SLOT + c.lane_off;
            // The data fragments are read PD k steps ahead by hand (an LDS-DMA is a store to LDS as far as the compiler knows,
            // so it never moves a ds_read above an earlier issue(): the refill in front of this loop is a fence for them).
            // No scheduling barriers between the k steps: the compiler's own interleaving of fragment reads, byte splits and
            // MFMAs measured faster (probe/kstep_probe.hip: 1483 against 1842 ns per tile pair and SIMD).
            auto tile_body = [&](auto skip_low) {
                constexpr bool SKIP_LOW = decltype(skip_low)::value;  // q2 == 0 throughout: no q2*hi product
                constexpr int PD = KS < RG_PD ? KS : RG_PD;
                v16i_t acc1, acc2;
                if constexpr (U8) {
                    // uint8 frames: this lane's 16 bytes of a k step are 8 frames; u ^ 0x80 = u - 128 as int8
                    v4i_t du[KS];
#pragma unroll
                    for (int ks = 0; ks < PD; ++ks) du[ks] = *reinterpret_cast<const v4i_t *>(la + 32 * ks);
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        v4i_t v = du[ks];
                        v.x ^= 0x80808080;
                        v.y ^= 0x80808080;
                        v.z ^= 0x80808080;
                        v.w ^= 0x80808080;
                        if (ks + PD < KS) du[ks + PD] = *reinterpret_cast<const v4i_t *>(la + 32 * (ks + PD));
                        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], v, ks ? acc1 : zero16, 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][1], v, ks ? acc2 : zero16, 0, 0, 0);
                    }
                } else if constexpr (G::SPLIT) {
                    // byte planes: the operands as they lie in the slot (high bytes at la, biased low bytes 32 rows further)
                    v4i_t hh[KS], ll[KS];
                    auto fetch = [&](int ks) {  // `ks` is a compile-time constant at every call site
                        hh[ks] = *reinterpret_cast<const v4i_t *>(la + 32 * ks);
                        ll[ks] = *reinterpret_cast<const v4i_t *>(la + 32 * G::PLANE_PITCH + 32 * ks);
                    };
#pragma unroll
                    for (int ks = 0; ks < PD; ++ks) fetch(ks);
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const v4i_t hi = hh[ks], lo = ll[ks];
                        if (ks + PD < KS) fetch(ks + PD);
                        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], hi, ks ? acc1 : zero16, 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], lo, ks ? acc2 : zero16, 0, 0, 0);
                        if constexpr (!SKIP_LOW) acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][1], hi, acc2, 0, 0, 0);
                    }
                } else {
                    // raw int16 tiles (14..16 k steps): every wave splits its fragments into high and biased low bytes itself
                    v4i_t dd[KS][2];
#pragma unroll
                    for (int ks = 0; ks < PD; ++ks) {
                        dd[ks][0] = *reinterpret_cast<const v4i_t *>(la + 64 * ks);
                        dd[ks][1] = *reinterpret_cast<const v4i_t *>(la + 64 * ks + 16);
                    }
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        if (EMIT && ks == KS - 3 && store_here) ring_emit_store<true>(a, c, em, eg);  // (its reads went out before k step 0)
                        const v4i_t d0 = dd[ks][0], d1 = dd[ks][1];
                        v4i_t hi, lo;
                        hi.x = __builtin_amdgcn_perm(d0.y, d0.x, 0x07050301);
                        hi.y = __builtin_amdgcn_perm(d0.w, d0.z, 0x07050301);
                        hi.z = __builtin_amdgcn_perm(d1.y, d1.x, 0x07050301);
                        hi.w = __builtin_amdgcn_perm(d1.w, d1.z, 0x07050301);
                        lo.x = __builtin_amdgcn_perm(d0.y, d0.x, 0x06040200) ^ 0x80808080;
                        lo.y = __builtin_amdgcn_perm(d0.w, d0.z, 0x06040200) ^ 0x80808080;
                        lo.z = __builtin_amdgcn_perm(d1.y, d1.x, 0x06040200) ^ 0x80808080;
                        lo.w = __builtin_amdgcn_perm(d1.w, d1.z, 0x06040200) ^ 0x80808080;
                        if (ks + PD < KS) {
                            dd[ks + PD][0] = *reinterpret_cast<const v4i_t *>(la + 64 * (ks + PD));
                            dd[ks + PD][1] = *reinterpret_cast<const v4i_t *>(la + 64 * (ks + PD) + 16);
                        }
                        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], hi, ks ? acc1 : zero16, 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], lo, ks ? acc2 : zero16, 0, 0, 0);
                        if constexpr (!SKIP_LOW) acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][1], hi, acc2, 0, 0, 0);
                    }
                }
                if (DEFER_ADDS) {
                    held1 = acc1;
                    held2 = acc2;
                    held_t = t;
                } else {
                    scatter(t, acc1, acc2);
                }
            };
            if constexpr (SKIP == 2 && !U8) {
                tile_body(std::true_type{});
            } else if constexpr (SKIP == 1 && !U8) {  // (a uniform branch: one lane's waves all take the same side)
                if (a.high_taps_only) tile_body(std::true_type{});
                else tile_body(std::false_type{});
            } else {
                tile_body(std::false_type{});
            }
        }
        }
        if (store_pending) ring_emit_store<true>(a, c, em, eg);  // (no tile of its own this round)
        slot = (slot + 1 == R) ? 0 : slot + 1;
    }
    if (DEFER_ADDS && held_t >= 0) scatter(held_t, held1, held2);
    // the last groups: everything has landed behind a full wait and one more barrier
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (EMIT) {
        const int k_last = (c.cnt + 62) >> 6;
        // the groups the loop has not emitted: PAIR emitted group k in round 2k + RG_EMIT_LAG_PAIR
        const int own = c.rounds - c.tshift;  // rounds in this lane's own count
        const int k_next = PAIR ? (own > RG_EMIT_LAG_PAIR ? ((own - 1 - RG_EMIT_LAG_PAIR) >> 1) + 1 : 0) : max(own - RG_EMIT_LAG, 0);
        if (!PAIR || c.tshift < RG_PAIR_IDLE)  // (the idle half of a pair without a second lane emits nothing)
            for (int k = k_next; k <= k_last; ++k) ring_emit_group<ACC64>(a, c, em, k);
    }
}

// The main loop of a multiplying wave of the half-step kernels (k_channelize_mfma_s16_ring_multi_half: byte planes fed by
// loader waves, int32 sums, one lane per workgroup): the wave's tile of 32 tap rows x 32 data rows as 16x16 blocks --
// tap-row halves bi, data-row halves bj -- on v_mfma_i32_16x16x64_i8: a chunk of 64 values (two k steps) per instruction,
// twelve per chunk; an odd last k step (at most 16 values) on seven v_mfma_i32_16x16x32_i8.  Held at its power limit the chip
// keeps a higher clock on this shape than on 32x32x32 (probe/kstep_probe.hip `shape`).
//   * Element r of lane l of block (bi, bj) is tap row 16 bi + 4 (l >> 4) + r against data row 16 bj + (l & 15): output
//     position 16 (bi + bj) + (l & 15) + 4 (l >> 4) + r of the tile.  Blocks (0, 1) and (1, 0) are the same positions and
//     share their accumulators: three blocks per sum, 12 adds per tile.  (dsp_plan.plan_mfma(acc32=True) bounds any
//     partial sum of an output's terms, so no such sum overflows.)
//   * Tap operand of chunk c, half bi: values 64 c + 16 (l >> 4) .. + 15 of tap row 16 bi + (l & 15) -- in the planner's
//     fragments (32x32x32 order: lane = row + 32 * (value >> 4) of the k step) that is lane 16 bi + (l & 15) + 32 ((l >> 4) & 1)
//     of k step 2 c + (l >> 5).  Gathered once per wave.
//   * Data operand: 16 bytes at 64 c + 16 (l >> 4) of row 16 bj + (l & 15) of either plane (RingGeo::PLANE_PITCH keeps these
//     reads conflict-free).  What a row holds past its 2 D values meets zero taps.
//   * The odd last step holds 16 values, and the K = 32 instruction issues in the cycles of K = 64: one
//     instruction per product would multiply half of every operand by zero taps.  So two products that add into the same
//     accumulator share an instruction, concatenated along K -- operand [x | y] . [u ; v]: lane groups l >> 4 = 0, 1 hold
//     values 8 ((l >> 4) & 1) .. + 7 of tap piece x and of data bytes u, groups 2, 3 those of y and v:
//         S1[0] = [0 | q1_0] . [lo_0 ; hi_0]         S2[0] = [q1_0 | q2_0] . [lo_0 ; hi_0]
//         S1[1] = [q1_0 | q1_1] . [hi_1 ; hi_0]      S2[1] = [q1_0 | q1_1] . [lo_1 ; lo_0] + [q2_0 | q2_1] . [hi_1 ; hi_0]
//         S1[2] = [0 | q1_1] . [lo_1 ; hi_1]         S2[2] = [q1_1 | q2_1] . [lo_1 ; hi_1]
//     (q1, q2 of tap-row half 0 / 1, hi, lo of data-row half 0 / 1, S[s] the block sum bi + bj = s): seven instructions for
//     the twelve products, the same integer terms in every sum; six tap operands of 8 bytes gathered once per wave, four
//     data operands of 8 bytes read per tile.
//   * ZEDGE (launches whose lane carries zrot != 0, dsp_plan's afrag_rot): the first and last tap rows of a Kaiser design
//     are tiny, their high tap byte q1 is zero throughout, and of such a row's three products only q2 * hi is left.  The
//     planner has rotated the rows of either component by zrot slots (slot s holds tap row (s - zrot) mod 64) so that
//     slots 0..15 are such rows: the waves of even rt run ring_main_h16_light on them, the waves of odd rt this body,
//     their rows moved by the rotation.
template <int KS>
__device__ __forceinline__ void ring_main_h16_light(const MfmaArgs &a, const RingCtx &c);

template <int KS, bool ZEDGE = false>
__device__ __forceinline__ void ring_main_h16(const MfmaArgs &a, const RingCtx &c)
{
    if constexpr (ZEDGE) {
        if (!(c.rt & 1)) {  // (wave-uniform, like loader against multiplier)
            ring_main_h16_light<KS>(a, c);
            return;
        }
    }
    const int zrot = ZEDGE ? a.zrot : 0;  // (odd rt: slots 32.. of a component, behind the wrap: tap rows 32 - zrot ..)
    using G = RingGeo<KS, false, false, false, true>;
    static_assert(G::SPLIT && G::R == 2, "byte planes, two slots per parity");
    constexpr int SLOT = G::SLOT, PP = G::PLANE_PITCH, NC = KS / 2, ODD = KS & 1;
    const int r16 = c.lane & 15, g = c.lane >> 4;
    v4i_t tq[NC ? NC : 1][2][2];  // [chunk][tap-row half][piece q1, q2]
    long tf[6] = {};              // the odd last k step: TF_*
    enum { TF_Z_Q10, TF_Q10_Q11, TF_Z_Q11, TF_Q10_Q20, TF_Q20_Q21, TF_Q11_Q21 };  // [x | y]: q<piece><tap-row half>, Z = zeros
    const v4i_t *fa = a.afrag + c.rt * 128;
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) tq[ch][bi][pc] = fa[((2 * ch + (g >> 1)) * 8 + pc) * 64 + 16 * bi + r16 + 32 * (g & 1)];
    if constexpr (ODD) {
        long s[2][2];  // [tap-row half][piece]: values 8 (g & 1) .. + 7 of the last k step
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) s[bi][pc] = reinterpret_cast<const long *>(fa + ((KS - 1) * 8 + pc) * 64 + 16 * bi + r16)[g & 1];
        const bool up = g >> 1;  // lane groups 2, 3: the operand's second piece
        tf[TF_Z_Q10] = up ? s[0][0] : 0;
        tf[TF_Q10_Q11] = up ? s[1][0] : s[0][0];
        tf[TF_Z_Q11] = up ? s[1][0] : 0;
        tf[TF_Q10_Q20] = up ? s[0][1] : s[0][0];
        tf[TF_Q20_Q21] = up ? s[1][1] : s[0][1];
        tf[TF_Q11_Q21] = up ? s[1][1] : s[1][0];
    }
    // have them arrive here: a wait for them inside the round loop would be met in every round
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
#pragma unroll
        for (int bi = 0; bi < 2; ++bi) asm volatile("" ::"v"(tq[ch][bi][0]), "v"(tq[ch][bi][1]));
    asm volatile("" ::"v"(tf[0]), "v"(tf[1]), "v"(tf[2]), "v"(tf[3]), "v"(tf[4]), "v"(tf[5]));
    const int lane_off = r16 * PP + 16 * g;
    // The odd step's four 8-byte data operands [u ; v]: lane groups 0, 1 read bytes 8 (g & 1) .. + 7 of the last k step of u,
    // groups 2, 3 those of v (u, v: a plane and a data-row half each).  Each read gets an offset register of its own, and the
    // compiler is not told how they relate: it would pair them into ds_read2st64_b64, whose 16-lane groups and 32 banks make
    // this pitch a 4-way conflict (measured: 24 extra LDS cycles per instruction against 2 for a plain ds_read_b64)
    enum { DF_L0_H0, DF_L1_L0, DF_H1_H0, DF_L1_H1 };  // [u ; v]: H / L = high / biased low bytes, of data-row half 0 / 1
    int lane_off_odd[4];
    {
        const int up = g >> 1, at = r16 * PP + 32 * (KS - 1) + 8 * (g & 1);
        const int hi_pl = 0, lo_pl = 32 * PP, bj1 = 16 * PP;
        lane_off_odd[DF_L0_H0] = at + (up ? hi_pl : lo_pl);
        lane_off_odd[DF_L1_L0] = at + lo_pl + (up ? 0 : bj1);
        lane_off_odd[DF_H1_H0] = at + hi_pl + (up ? 0 : bj1);
        lane_off_odd[DF_L1_H1] = at + bj1 + (up ? hi_pl : lo_pl);
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(lane_off_odd[i]));
    }
    const v4i_t zero4 = {0, 0, 0, 0};
    int slot = 0;
    for (int r = 0; r < c.rounds; ++r) {
        asm volatile("s_barrier" ::: "memory");
        const int t = 2 * r + c.cp;
        if (t < c.tiles) {
            const char *la = c.smem + (slot * 2 + c.cp) * SLOT + lane_off;
            const char *lb = c.smem + (slot * 2 + c.cp) * SLOT;
            v4i_t hh[NC ? NC : 1][2], ll[NC ? NC : 1][2];  // [chunk][data-row half]: high bytes, biased low bytes
            long df[4] = {};     // the odd last k step: DF_*
            v4i_t a1[3], a2[3];  // S1, S2 of the blocks bi + bj = 0, 1, 2
            auto fetch = [&](int ch) {  // `ch` is a compile-time constant at every call site
                if (ch < NC) {
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) {
                        hh[ch][bj] = *reinterpret_cast<const v4i_t *>(la + 16 * PP * bj + 64 * ch);
                        ll[ch][bj] = *reinterpret_cast<const v4i_t *>(la + 32 * PP + 16 * PP * bj + 64 * ch);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) df[i] = *reinterpret_cast<const long *>(lb + lane_off_odd[i]);
                }
            };
            // the twelve products of a chunk (q1*hi into S1; q1*lo and q2*hi into S2); an accumulator's uses lie at least two
            // instructions apart
            auto step = [&](auto mf, const auto &q, const auto &hi, const auto &lw, bool first) {
                a2[1] = mf(q[0][0], lw[1], first ? zero4 : a2[1]);
                a1[0] = mf(q[0][0], hi[0], first ? zero4 : a1[0]);
                a2[0] = mf(q[0][0], lw[0], first ? zero4 : a2[0]);
                a2[1] = mf(q[1][0], lw[0], a2[1]);
                a1[1] = mf(q[0][0], hi[1], first ? zero4 : a1[1]);
                a1[2] = mf(q[1][0], hi[1], first ? zero4 : a1[2]);
                a2[1] = mf(q[0][1], hi[1], a2[1]);
                a2[2] = mf(q[1][0], lw[1], first ? zero4 : a2[2]);
                a1[1] = mf(q[1][0], hi[0], a1[1]);
                a2[1] = mf(q[1][1], hi[0], a2[1]);
                a2[0] = mf(q[0][1], hi[0], a2[0]);
                a2[2] = mf(q[1][1], hi[1], a2[2]);
            };
            auto mf64 = [](v4i_t x, v4i_t y, v4i_t z) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(x, y, z, 0, 0, 0); };
            // The same twelve products of the odd last k step, 16 values each, folded along K into seven instructions of 32: two
            // products that add into one accumulator are one [x | y] . [u ; v].  a1[0] and a1[2] have one product each and
            // borrow the operands of a2[0] and a2[2] with the other half of the taps zero.  The order keeps the two uses of
            // a2[1], and every accumulator's last use in the chunk before, at least two instructions apart.
            auto step_odd = [&](bool first) {
                auto mf32 = [](long x, long y, v4i_t z) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(x, y, z, 0, 0, 0); };
                a1[0] = mf32(tf[TF_Z_Q10], df[DF_L0_H0], first ? zero4 : a1[0]);
                a2[1] = mf32(tf[TF_Q10_Q11], df[DF_L1_L0], first ? zero4 : a2[1]);
                a1[1] = mf32(tf[TF_Q10_Q11], df[DF_H1_H0], first ? zero4 : a1[1]);
                a2[0] = mf32(tf[TF_Q10_Q20], df[DF_L0_H0], first ? zero4 : a2[0]);
                a2[1] = mf32(tf[TF_Q20_Q21], df[DF_H1_H0], a2[1]);
                a1[2] = mf32(tf[TF_Z_Q11], df[DF_L1_H1], first ? zero4 : a1[2]);
                a2[2] = mf32(tf[TF_Q11_Q21], df[DF_L1_H1], first ? zero4 : a2[2]);
            };
            fetch(0);  // reads run one step ahead of the MFMAs
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                if (ch + 1 < NC + ODD) fetch(ch + 1);
                step(mf64, tq[ch], hh[ch], ll[ch], ch == 0);
            }
            if constexpr (ODD) step_odd(NC == 0);
            // diagonal scatter into the window of sums, 256*S1 + S2 in one int32 as in ring_main (inline asm for the same reason)
            // (lanes 16 apart meet on 12 of a half wave's 20 addresses: a 2-way serialisation per add.  Sending the lanes of odd
            // l >> 4 into a second window that the emission adds measured the same)
            const unsigned p = lds_addr(c.s_acc + ((t * 32 + 32 * (c.rt & 1) - zrot + r16 + 4 * g + 1) & (RG_W - 1)) + (c.rt >> 1) * RG_AS);
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int comb = (a1[s][q] << 8) + a2[s][q];
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(4 * (16 * s + q)));
                }
        }
        slot ^= 1;
    }
    // the loader waves emit the last groups behind a full wait and one more barrier
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The light wave of a ZEDGE launch (even rt): slots 0..31 of a component, of which 0..15 (tap-row half 0) have q1 = 0.
//   * Per chunk eight instructions instead of twelve:
//         Z[bj] = q2_0 . hi_bj                      (half 0: S2 alone; no S1 accumulator, no q1 fragments)
//         S1[bj] = q1_1 . hi_bj        S2[bj] = q1_1 . lo_bj + q2_1 . hi_bj        (half 1)
//     and on the folded odd step six instead of seven, from two of the four 8-byte reads:
//         Z[bj] = [0 | q2_0] . [lo_bj ; hi_bj]    S1[bj] = [0 | q1_1] . [lo_bj ; hi_bj]    S2[bj] = [q1_1 | q2_1] . [lo_bj ; hi_bj]
//   * Half 0's rows are two runs -- the filter's last rows, then its first: slots 4 g .. + 3 of a lane group hold tap rows
//     64 - zrot + 4 g .. while 4 g < zrot and 4 g - zrot .. behind (zrot a multiple of 4, at most 32: the launcher checks) --
//     so the scatter base differs per lane group; it is computed once per wave.  Half 1 may wrap the same way.  The halves
//     share no output positions (the (0, 1) / (1, 0) sharing of the heavy body needs consecutive rows): 16 adds per tile.
//   * Z goes to the add through a VALU instruction the compiler sees (+ an opaque zero): the compiler places the wait
//     states a matrix result needs in front of its own instructions, not in front of inline asm -- fed directly, the adds
//     sent stale registers (probe/kstep_probe.hip `zedge`).
template <int KS>
__device__ __forceinline__ void ring_main_h16_light(const MfmaArgs &a, const RingCtx &c)
{
    using G = RingGeo<KS, false, false, false, true>;
    constexpr int SLOT = G::SLOT, PP = G::PLANE_PITCH, NC = KS / 2, ODD = KS & 1;
    const int r16 = c.lane & 15, g = c.lane >> 4;
    v4i_t t20[NC ? NC : 1], t1[NC ? NC : 1][2];  // q2 of tap-row half 0; q1, q2 of half 1
    long tf[3] = {};
    enum { TF_Z_Q20, TF_Z_Q11, TF_Q11_Q21 };  // [x | y] as in ring_main_h16
    const v4i_t *fa = a.afrag + c.rt * 128;
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        const v4i_t *f = fa + (2 * ch + (g >> 1)) * 8 * 64 + r16 + 32 * (g & 1);
        t20[ch] = f[64], t1[ch][0] = f[16], t1[ch][1] = f[64 + 16];
    }
    if constexpr (ODD) {
        const v4i_t *f = fa + (KS - 1) * 8 * 64 + r16;
        const long q20 = reinterpret_cast<const long *>(f + 64)[g & 1], q11 = reinterpret_cast<const long *>(f + 16)[g & 1];
        const long q21 = reinterpret_cast<const long *>(f + 64 + 16)[g & 1];
        const bool up = g >> 1;
        tf[TF_Z_Q20] = up ? q20 : 0;
        tf[TF_Z_Q11] = up ? q11 : 0;
        tf[TF_Q11_Q21] = up ? q21 : q11;
    }
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) asm volatile("" ::"v"(t20[ch]), "v"(t1[ch][0]), "v"(t1[ch][1]));
    asm volatile("" ::"v"(tf[0]), "v"(tf[1]), "v"(tf[2]));
    const int lane_off = r16 * PP + 16 * g;
    int lane_off_odd[2], vzero = 0;  // [lo_0 ; hi_0], [lo_1 ; hi_1]: an offset register each, as in ring_main_h16
    {
        const int at = r16 * PP + 32 * (KS - 1) + 8 * (g & 1) + ((g >> 1) ? 0 : 32 * PP);
        lane_off_odd[0] = at;
        lane_off_odd[1] = at + 16 * PP;
        asm volatile("" : "+v"(lane_off_odd[0]), "+v"(lane_off_odd[1]), "+v"(vzero));
    }
    // first tap row of this lane group's four slots of either half, + the data row + 1
    const int s0 = 4 * g, s1 = 16 + 4 * g;
    const int base0 = s0 - a.zrot + (s0 < a.zrot ? MF_Q : 0) + r16 + 1, base1 = s1 - a.zrot + (s1 < a.zrot ? MF_Q : 0) + r16 + 1;
    int *const win = c.s_acc + (c.rt >> 1) * RG_AS;
    const v4i_t zero4 = {0, 0, 0, 0};
    int slot = 0;
    for (int r = 0; r < c.rounds; ++r) {
        asm volatile("s_barrier" ::: "memory");
        const int t = 2 * r + c.cp;
        if (t < c.tiles) {
            const char *la = c.smem + (slot * 2 + c.cp) * SLOT + lane_off;
            const char *lb = c.smem + (slot * 2 + c.cp) * SLOT;
            v4i_t hh[NC ? NC : 1][2], ll[NC ? NC : 1][2];
            long df[2] = {};
            v4i_t z[2], a1[2], a2[2];  // per data-row half bj: S2 of tap-row half 0; S1, S2 of half 1
            auto fetch = [&](int ch) {  // `ch` is a compile-time constant at every call site
                if (ch < NC) {
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) {
                        hh[ch][bj] = *reinterpret_cast<const v4i_t *>(la + 16 * PP * bj + 64 * ch);
                        ll[ch][bj] = *reinterpret_cast<const v4i_t *>(la + 32 * PP + 16 * PP * bj + 64 * ch);
                    }
                } else {
                    df[0] = *reinterpret_cast<const long *>(lb + lane_off_odd[0]);
                    df[1] = *reinterpret_cast<const long *>(lb + lane_off_odd[1]);
                }
            };
            auto mf64 = [](v4i_t x, v4i_t y, v4i_t zz) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(x, y, zz, 0, 0, 0); };
            auto mf32 = [](long x, long y, v4i_t zz) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(x, y, zz, 0, 0, 0); };
            fetch(0);
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                if (ch + 1 < NC + ODD) fetch(ch + 1);
                const bool first = ch == 0;  // (an accumulator's uses lie at least two instructions apart)
                z[0] = mf64(t20[ch], hh[ch][0], first ? zero4 : z[0]);
                a1[0] = mf64(t1[ch][0], hh[ch][0], first ? zero4 : a1[0]);
                a2[0] = mf64(t1[ch][0], ll[ch][0], first ? zero4 : a2[0]);
                z[1] = mf64(t20[ch], hh[ch][1], first ? zero4 : z[1]);
                a1[1] = mf64(t1[ch][0], hh[ch][1], first ? zero4 : a1[1]);
                a2[1] = mf64(t1[ch][0], ll[ch][1], first ? zero4 : a2[1]);
                a2[0] = mf64(t1[ch][1], hh[ch][0], a2[0]);
                a2[1] = mf64(t1[ch][1], hh[ch][1], a2[1]);
            }
            if constexpr (ODD) {
#pragma unroll
                for (int bj = 0; bj < 2; ++bj) {
                    z[bj] = mf32(tf[TF_Z_Q20], df[bj], NC == 0 ? zero4 : z[bj]);
                    a1[bj] = mf32(tf[TF_Z_Q11], df[bj], NC == 0 ? zero4 : a1[bj]);
                    a2[bj] = mf32(tf[TF_Q11_Q21], df[bj], NC == 0 ? zero4 : a2[bj]);
                }
            }
            // diagonal scatter, ds_add_u32 in inline asm as in ring_main_h16: half 0 sends S2 alone
            const unsigned p0 = lds_addr(win + ((t * 32 + base0) & (RG_W - 1))), p1 = lds_addr(win + ((t * 32 + base1) & (RG_W - 1)));
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int comb = z[bj][q] + vzero;
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p0), "v"(comb), "n"(4 * (16 * bj + q)));
                }
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int comb = (a1[bj][q] << 8) + a2[bj][q];
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p1), "v"(comb), "n"(4 * (16 * bj + q)));
                }
        }
        slot ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One block = one contiguous range of outputs of any length (the host gives every CU one range): a persistent
// stream through the ring, sums in a 512-position sliding window, outputs emitted two rounds behind the matrix work.
// SKIPK (kernels of launches in which some lanes have high-byte-only taps, see ring_main's SKIP): lane pairs -- the pair's
// first lane (parity 0) skips the q2*hi product at compile time, the second never does (the host pairs a tap-row group's
// high-byte lane with its residue lane); one lane per workgroup -- every wave asks its lane's flag.
template <int KS, bool ACC64, bool ROWS, bool U8, bool PAIR = false, bool SKIPK = false, bool HALF = false, bool ONCE = false, bool ZEDGE = false>
__device__ __forceinline__ void ring_block(const MfmaArgs &a, long long range_idx)
{
    using G = RingGeo<KS, ROWS, U8, PAIR, HALF>;
    constexpr int R = G::R, SLOT = G::SLOT;
    constexpr bool LOADERS = G::LOADERS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    RingCtx c;
    c.lane = tid & 63;
    c.rt = wave & 3;
    c.cp = wave >= RG_WAVES ? (wave - RG_WAVES) & 1 : (wave >> 2) & 1;  // (loader waves: their parity, or the lane of a pair they emit)
    // ZEDGE: the multiplying waves of parity 1 take rt ^ 1, so that every SIMD hosts one light (even rt) and one heavy wave:
    // 8 + 12 instead of 12 + 12 matrix instructions per chunk on each.  Waves w and w + 4 share a SIMD -- read back from
    // HW_ID by probe/kstep_probe.hip `zedge` (SIMD_ID of waves 0..11: 2 1 3 0 2 1 3 0 2 1 3 0 on one box, 1 3 0 2 ... on another)
    if constexpr (ZEDGE)
        if (wave < RG_WAVES) c.rt ^= c.cp;
    c.col = c.lane & 31;
    c.h = c.lane >> 5;

    c.i0 = range_idx * a.range;
    c.cnt = static_cast<int>(min(static_cast<long long>(a.range), a.n_out - c.i0));
    c.m0 = a.m_lo + c.i0;
    c.tiles = (c.cnt + 63 + 31) >> 5;  // data columns b in [m0-64, m0+cnt-2], rounded up to tiles of 32
    c.rounds = PAIR ? c.tiles + a.pair_extra : (c.tiles + 1) >> 1;
    c.tshift = PAIR ? a.pair_shift : 0;  // (RG_PAIR_IDLE: the idle half of a pair without a second lane -- barriers only)
    c.smem = smem;
    c.s_acc = reinterpret_cast<int *>(smem + R * G::TPR * SLOT);
    for (int i = tid; i < G::ACCS * RG_ACC_BYTES / 4; i += G::THREADS) c.s_acc[i] = 0;
    if (PAIR) c.s_acc += c.cp * (RG_ACC_BYTES / 4);  // each lane of the pair sums into its own window

    // the stream: tile t starts at data row m0 - 64 - col_shift + 32 t, i.e. frame row*D + 1
    constexpr int FB = U8 ? 2 : 4;  // bytes per frame
    const long long row_bytes = static_cast<long long>(FB) * a.D;
    c.tile_bytes = 32 * row_bytes;
    const char *stream = reinterpret_cast<const char *>(a.raw) + FB * ((c.m0 - MF_Q - a.col_shift) * a.D + 1 - a.consumed) +
                         (ROWS ? G::KBYTES * a.k_first : 0);
    c.row_units = static_cast<int>(row_bytes >> 4);
    c.pitch_units = G::PADDED ? (c.row_units | 1) : c.row_units;  // odd: conflict-free fragment reads (see RingGeo)
    c.lane_off = G::SPLIT ? c.col * G::PLANE_PITCH + 16 * c.h : c.col * (ROWS ? G::PITCH : 16 * c.pitch_units) + (G::KBYTES / 2) * c.h;

    if constexpr (LOADERS) {
        if (wave >= RG_WAVES) {
            c.stream0 = stream;
            __syncthreads();
            if constexpr (G::SPLIT && PAIR) {
                switch (wave - RG_WAVES) {
                    case 0: ring_loader_split<KS, ACC64, ROWS, 0, true>(a, c); break;
                    case 1: ring_loader_split<KS, ACC64, ROWS, 1, true>(a, c); break;
                    case 2: ring_loader_split<KS, ACC64, ROWS, 2, true>(a, c); break;
                    default: ring_loader_split<KS, ACC64, ROWS, 3, true>(a, c); break;
                }
            } else if constexpr (G::SPLIT) {
                if ((wave - RG_WAVES) >> 1) ring_loader_split<KS, ACC64, ROWS, 1, false, HALF, ONCE>(a, c);
                else ring_loader_split<KS, ACC64, ROWS, 0, false, HALF, ONCE>(a, c);
            } else {
                ring_loader<KS, ACC64>(a, c);
            }
            return;
        }
    }
    // A row of 2 D values whose last k step holds at most 16 of them (D = 104: 208 = 6 x 32 + 16), up to 8 k steps (the
    // kernel variant HALF: the launcher picks it for rows of 32 (KS - 1) + 1 .. 16 values): 16x16x64 matrix tiles, which
    // gather their own tap operands
    if constexpr (HALF) {
        static_assert(!ROWS && !U8 && !PAIR && !ACC64 && !SKIPK, "16x16x64 tiles: single lanes over contiguous byte-plane slots, int32 sums");
        __syncthreads();
        c.stream0 = stream;
        ring_main_h16<KS, ZEDGE>(a, c);
    } else {
    // tap fragments of this wave's row tile: registers for the whole block
    v4i_t fq[KS][2];
    {
        const v4i_t *fa = a.afrag + c.rt * 128 + c.lane;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) fq[ks][pc] = fa[(ks * 8 + pc) * 64];
        // have them arrive here, before the first DMA: a later wait for them would drain the DMA queue with them
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" ::"v"(fq[ks][0]), "v"(fq[ks][1]));
    }
    __syncthreads();
    c.stream0 = stream;
    if constexpr (PAIR && G::SPLIT) {
        // loader waves feed the ring and emit: every multiplying wave only multiplies (parity 1 defers its adds)
        constexpr int SA = SKIPK ? 2 : 0, SB = 0;  // (parity 0 = the pair's first lane)
        if (c.cp) ring_main<KS, ACC64, ROWS, U8, false, false, true, true>(a, c, fq, std::integral_constant<int, SB>{});
        else ring_main<KS, ACC64, ROWS, U8, false, false, false, true>(a, c, fq, std::integral_constant<int, SA>{});
    } else if constexpr (PAIR) {
        // parity 0's first two waves feed the ring (one tile per round: the same KS + 1 instructions per issuing wave and
        // round as without pairs); one wave of either parity emits ITS lane's outputs; parity 1 defers its adds
        // (waves go to SIMDs cyclically: issuers on SIMDs 0 and 1, lane A's emitter -- wave 2 -- on SIMD 2, lane B's -- wave
        // 7 -- on SIMD 3)
        constexpr int SA = SKIPK ? 2 : 0, SB = 0;  // (parity 0 = the pair's first lane)
        if (c.cp == 0 && c.rt < 2) ring_main<KS, ACC64, ROWS, U8, true, false, false, true>(a, c, fq, std::integral_constant<int, SA>{});
        else if (c.cp == 0 && c.rt == 2) ring_main<KS, ACC64, ROWS, U8, false, true, false, true>(a, c, fq, std::integral_constant<int, SA>{});
        else if (c.cp == 1 && c.rt == 3) ring_main<KS, ACC64, ROWS, U8, false, true, false, true>(a, c, fq, std::integral_constant<int, SB>{});
        else if (c.cp) ring_main<KS, ACC64, ROWS, U8, false, false, true, true>(a, c, fq, std::integral_constant<int, SB>{});
        else ring_main<KS, ACC64, ROWS, U8, false, false, false, true>(a, c, fq, std::integral_constant<int, SA>{});
    } else if constexpr (LOADERS) {
        constexpr int S1 = SKIPK ? 1 : 0;
        if (c.cp) ring_main<KS, ACC64, ROWS, U8, false, false, true, false>(a, c, fq, std::integral_constant<int, S1>{});
        else ring_main<KS, ACC64, ROWS, U8, false, false, false, false>(a, c, fq, std::integral_constant<int, S1>{});
    } else {
        constexpr int S1 = SKIPK ? 1 : 0;
        // one issuing wave per SIMD (waves go to SIMDs in a cyclic order of period 4): rt 0,1 of parity 0, rt 2,3 of parity 1
        if ((c.rt >> 1) == c.cp) {
            if (c.cp) ring_main<KS, ACC64, ROWS, U8, true, false, true, false>(a, c, fq, std::integral_constant<int, S1>{});
            else ring_main<KS, ACC64, ROWS, U8, true, false, false, false>(a, c, fq, std::integral_constant<int, S1>{});
        } else if (wave == RG_EMIT_WAVE) ring_main<KS, ACC64, ROWS, U8, false, true, false, false>(a, c, fq, std::integral_constant<int, S1>{});
        else if (c.cp) ring_main<KS, ACC64, ROWS, U8, false, false, true, false>(a, c, fq, std::integral_constant<int, S1>{});
        else ring_main<KS, ACC64, ROWS, U8, false, false, false, false>(a, c, fq, std::integral_constant<int, S1>{});
    }
    }
}

// ---- several channels of ONE capture in one launch (shared ingest) ---------------------------------------------
//
// A lane = one (channel, tap-row group): its own tap fragments, output, scale, rotation.  All lanes of a launch share
// the capture, the decimation, the k-step range and the output range [m_lo, m_lo + n_out).  The reference runs a whole
// pipeline per --ft target over the same file (cli.py:683-710); here the lanes of one stretch of the capture run AT THE
// SAME TIME on the CUs of ONE XCD, so that stretch crosses the fabric once and the other lanes' LDS-DMAs hit in that
// XCD's L2: workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one -- a speed assumption only, nothing
// here depends on it for correctness), so workgroup b takes lane (b / 8) % n_lanes of output range
// ((b / 8) / n_lanes) * 8 + b % 8.  Every lane does the same work per tile, so the lanes of a range stay within a few
// rounds of each other without any synchronisation (4 MiB of L2 per XCD = dozens of rounds of slack).
constexpr int RG_MAX_LANES = 16;  // (<= 5 targets x <= 3 tap-row groups in the reference's CLI; the table travels as kernel arguments)

struct RingMultiArgs {
    MfmaArgs c;  // what the lanes share; the per-lane fields of `c` are overwritten per workgroup
    int n_lanes;
    MfmaLane lane[RG_MAX_LANES];
};

template <int KS, bool ROWS, bool U8, bool PAIR = false, bool ACC64 = false, bool SKIPK = false, bool HALF = false, bool ONCE = false, bool ZEDGE = false>
__device__ __forceinline__ void ring_multi_block(const RingMultiArgs &m)
{
    const int idx = blockIdx.x >> 3;
    // uniform: scalar loads from the kernel-argument segment.  PAIR: the table holds the pairs back to back, a workgroup
    // takes pair (idx mod n_pairs) and its waves of parity cp (waves 4..7: cp = 1) the pair's lane cp
    const int units = PAIR ? m.n_lanes >> 1 : m.n_lanes;
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    // (loader waves 8, 10 carry the first lane's arguments, 9, 11 the second's: waves 8 and 9 emit those lanes)
    const int li = PAIR ? 2 * (idx % units) + (wv >= RG_WAVES ? wv & 1 : (wv >> 2) & 1) : idx % units;
    const long long range_idx = static_cast<long long>(idx / units) * 8 + (blockIdx.x & 7);
    const MfmaLane &l = m.lane[li];
    MfmaArgs a = m.c;
    a.pair_shift = a.pair_extra = 0;
    a.afrag = l.afrag;
    a.out = l.out;
    a.partial_in = l.partial_in;
    a.partial_out = l.partial_out;
    a.unit = l.unit;
    a.c_re = l.c_re;
    a.c_im = l.c_im;
    a.rot_step = l.rot_step;
    a.rot_base = l.rot_base;
    a.rot64_re = l.rot64_re;
    a.rot64_im = l.rot64_im;
    a.sc_re = l.sc_re;
    a.sc_im = l.sc_im;
    a.col_shift = l.col_shift;
    a.finalize = l.finalize;
    a.conj_sum = l.conj_sum;
    a.rotate = l.rotate;
    a.raw_partials = l.raw_partials;
    a.high_taps_only = l.high_taps_only;
    a.zrot = l.zrot;
    if constexpr (PAIR) {
        // the pair's first lane has the larger (or the same) tap-row group: ITS stream is staged, the second lane's own
        // tiles arrive 2 rounds per group of difference later; a pair without a second lane (afrag NULL) idles that half
        const MfmaLane &la = m.lane[li & ~1], &lb = m.lane[li | 1];
        const bool idle_b = lb.afrag == nullptr;
        // (rounds the second lane works behind the first: two tiles, one round each, per tap-row group of difference)
        a.pair_extra = idle_b ? 0 : (la.col_shift - lb.col_shift) >> 5;
        a.col_shift = la.col_shift;
        if (li & 1) {
            a.pair_shift = idle_b ? RG_PAIR_IDLE : a.pair_extra;
            if (idle_b) a.afrag = la.afrag;  // (anything readable: the fragments are loaded, never used)
        }
        a.pace_units = units;
        a.pace_slot = static_cast<int>(range_idx) * units + idx % units;
    }
    if (range_idx * a.range >= a.n_out) return;  // (the last ranges of a short launch)
    ring_block<KS, ACC64, ROWS, U8, PAIR, SKIPK, HALF, ONCE, ZEDGE>(a, range_idx);
}

// ACC64: one int64 (S1 << 32) + S2 per output component instead of one int32 256*S1 + S2 -- 16-bit taps without the int32
// bound, what the "full" precision's lanes (taps + their residue, dsp_plan.plan_mfma(residual=True)) need; contiguous slots only.
// ONCE (launches of a single lane, loader waves): the loaders stream the capture with nt loads (ring_load16).
template <int KS, bool ACC64 = false, bool SKIPK = false, bool ONCE = false>
__global__ __launch_bounds__((RingGeo<KS, false>::THREADS), (RingGeo<KS, false>::LOADERS ? 3 : 2)) void k_channelize_mfma_s16_ring_multi(RingMultiArgs m)
{
    static_assert(!ONCE || (RingGeo<KS, false>::SPLIT && !ACC64 && !SKIPK), "nt variant: byte-plane kernels, int32 sums, no skipped product");
    ring_multi_block<KS, false, false, false, ACC64, SKIPK, false, ONCE>(m);
}

// ... for rows whose last k step is at most half full (rows of 32 (KS - 1) + 1 .. 16 values: D = 104 -> 208 = 6 x 32 + 16),
// on 16x16x64 matrix tiles (ring_main_h16).  ZEDGE (single-lane launches whose lane carries zrot != 0): the all-zero high
// tap bytes of the filter's edge rows are not multiplied (ring_main_h16_light).
template <int KS, bool ONCE = false, bool ZEDGE = false>
__global__ __launch_bounds__((RingGeo<KS, false, false, false, true>::THREADS), 3) void k_channelize_mfma_s16_ring_multi_half(RingMultiArgs m)
{
    static_assert(RingGeo<KS, false, false, false, true>::SPLIT, "byte-plane kernels only");
    static_assert(!ZEDGE || ONCE, "rotated fragments: single-lane launches");
    ring_multi_block<KS, false, false, false, false, false, true, ONCE, ZEDGE>(m);
}

// Two lanes per workgroup (RingGeo PAIR): the lanes of the table in pairs of equal tap-row group.
template <int KS, bool ACC64 = false, bool SKIPK = false>
__global__ __launch_bounds__((RingGeo<KS, false, false, true>::THREADS), (RingGeo<KS, false, false, true>::LOADERS ? 3 : 2)) void k_channelize_mfma_s16_ring_pairs(RingMultiArgs m)
{
    ring_multi_block<KS, false, false, true, ACC64, SKIPK>(m);
}

template <int KS, bool SKIPK = false>
__global__ __launch_bounds__((RingGeo<KS, true>::THREADS), 3) void k_channelize_mfma_s16_ring_rows_multi(RingMultiArgs m)
{
    ring_multi_block<KS, true, false, false, false, SKIPK>(m);
}

template <int KS>
__global__ __launch_bounds__((RingGeo<KS, true, true>::THREADS), 3) void k_channelize_mfma_u8_ring_rows_multi(RingMultiArgs m)
{
    ring_multi_block<KS, true, true>(m);
}

// The 160 KiB dynamic-LDS limit is a per-device attribute of a kernel: `done` remembers (one bit per device id)
// where it has been raised.  Two threads that race here both set it -- harmless, the call is idempotent.
template <typename K, typename A>
static int ring_launch_kernel(K kernel, const char *name, int threads, const A &a, unsigned blocks, size_t lds, hipStream_t stream,
                              std::atomic<unsigned long long> &done)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) {
            set_error("%s: cannot raise the dynamic LDS limit on device %d: %s", name, dev, hipGetErrorString(e));
            return IQA_EHIP;
        }
        done.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, stream, a);
    return check_launch(name);
}

// the kernel family the calling thread's last multi-lane launch took (mfma_ring_last_kernel: tests ask which body ran)
static thread_local const char *g_ring_last_kernel = "";

template <int KS>
static int ring_launch_multi(const RingMultiArgs &m, unsigned blocks, size_t lds, hipStream_t stream, bool rows, bool u8, bool acc64, bool skipk)
{
    g_ring_last_kernel = "another ring kernel";
    static std::atomic<unsigned long long> done[11] = {{0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}, {0}};
    // a single lane: one workgroup streams each range, nobody fetches a byte of the capture twice -- the variants whose
    // loaders stream it with nt loads (traces show them as <KS, false, false, true> and ..._multi_half<KS, true>)
    const bool once = m.n_lanes == 1;
    (void)once;  // (14 - 16 k steps have no such variant)
    if (acc64) {
        if constexpr (KS < RG_MAX_KS) {  // (64-bit sums at 16 k steps do not fit the registers)
            if (!rows && !u8) {
                if (skipk)
                    return ring_launch_kernel(k_channelize_mfma_s16_ring_multi<KS, true, true>, "k_channelize_mfma_s16_ring_multi64", RingGeo<KS, false>::THREADS, m, blocks, lds, stream, done[4]);
                return ring_launch_kernel(k_channelize_mfma_s16_ring_multi<KS, true>, "k_channelize_mfma_s16_ring_multi64", RingGeo<KS, false>::THREADS, m, blocks, lds, stream, done[3]);
            }
        }
        set_error("multi-lane launches with 64-bit sums: contiguous int16 slots, at most %d k steps (got %d)", RG_MAX_KS - 1, KS);
        return IQA_EINVAL;
    }
    if constexpr (KS <= RG_ROWS_MAX_KS_C) {
        if (u8) return ring_launch_kernel(k_channelize_mfma_u8_ring_rows_multi<KS>, "k_channelize_mfma_u8_ring_rows_multi", RingGeo<KS, true, true>::THREADS, m, blocks, lds, stream, done[2]);
        if (rows && skipk) return ring_launch_kernel(k_channelize_mfma_s16_ring_rows_multi<KS, true>, "k_channelize_mfma_s16_ring_rows_multi", RingGeo<KS, true>::THREADS, m, blocks, lds, stream, done[5]);
        if (rows) return ring_launch_kernel(k_channelize_mfma_s16_ring_rows_multi<KS>, "k_channelize_mfma_s16_ring_rows_multi", RingGeo<KS, true>::THREADS, m, blocks, lds, stream, done[1]);
    } else {
        if (u8 || rows) {
            set_error("row-staged ring kernels take at most %d k steps per pass (got %d)", RG_ROWS_MAX_KS_C, KS);
            return IQA_EINVAL;
        }
    }
    if (skipk) return ring_launch_kernel(k_channelize_mfma_s16_ring_multi<KS, false, true>, "k_channelize_mfma_s16_ring_multi", RingGeo<KS, false>::THREADS, m, blocks, lds, stream, done[6]);
    if constexpr (KS <= 8) {
        const int rem = (2 * m.c.D) & 31;  // values in the row's last k step
        if (rem != 0 && rem <= 16) {  // (planes at a pitch of their own: this family's LDS, not the caller's figure)
            using GH = RingGeo<KS, false, false, false, true>;
            // rotated fragments (mfma_ring_zedge_supported): the variant that skips the zero high tap bytes of slots 0..15
            if (once && m.lane[0].zrot) {
                g_ring_last_kernel = "k_channelize_mfma_s16_ring_multi_half<KS, ONCE, ZEDGE>";
                return ring_launch_kernel(k_channelize_mfma_s16_ring_multi_half<KS, true, true>, "k_channelize_mfma_s16_ring_multi", GH::THREADS, m, blocks, GH::LDS_BYTES, stream, done[10]);
            }
            g_ring_last_kernel = once ? "k_channelize_mfma_s16_ring_multi_half<KS, ONCE>" : "k_channelize_mfma_s16_ring_multi_half<KS>";
            if (once) return ring_launch_kernel(k_channelize_mfma_s16_ring_multi_half<KS, true>, "k_channelize_mfma_s16_ring_multi", GH::THREADS, m, blocks, GH::LDS_BYTES, stream, done[9]);
            return ring_launch_kernel(k_channelize_mfma_s16_ring_multi_half<KS>, "k_channelize_mfma_s16_ring_multi", GH::THREADS, m, blocks, GH::LDS_BYTES, stream, done[7]);
        }
    }
    if constexpr (KS <= RG_LOADERS_MAX_KS) {
        if (once) return ring_launch_kernel(k_channelize_mfma_s16_ring_multi<KS, false, false, true>, "k_channelize_mfma_s16_ring_multi", RingGeo<KS, false>::THREADS, m, blocks, lds, stream, done[8]);
    }
    return ring_launch_kernel(k_channelize_mfma_s16_ring_multi<KS>, "k_channelize_mfma_s16_ring_multi", RingGeo<KS, false>::THREADS, m, blocks, lds, stream, done[0]);
}

constexpr int RG_PAIR_MIN_KS = 9;  // lane pairs from 9 k steps on (below, a range's single-lane workgroups share the capture through L2 by themselves)

template <int KS>
static int ring_launch_pairs(const RingMultiArgs &m, unsigned blocks, hipStream_t stream, bool acc64, bool skipk)
{
    static std::atomic<unsigned long long> done{0}, done64{0}, done_s{0}, done64_s{0};
    if constexpr (KS >= RG_PAIR_MIN_KS && KS != 15) {  // (15: see mfma_ring_pairs_supported)
        using G = RingGeo<KS, false, false, true>;
        if (acc64) {
            if constexpr (KS <= 14) {
                if (skipk)
                    return ring_launch_kernel(k_channelize_mfma_s16_ring_pairs<KS, true, true>, "k_channelize_mfma_s16_ring_pairs64", G::THREADS, m, blocks, G::LDS_BYTES, stream, done64_s);
                return ring_launch_kernel(k_channelize_mfma_s16_ring_pairs<KS, true>, "k_channelize_mfma_s16_ring_pairs64", G::THREADS, m, blocks, G::LDS_BYTES, stream, done64);
            }
            set_error("lane pairs with 64-bit sums: 9..14 k steps (got %d)", KS);
            return IQA_EINVAL;
        }
        if (skipk) return ring_launch_kernel(k_channelize_mfma_s16_ring_pairs<KS, false, true>, "k_channelize_mfma_s16_ring_pairs", G::THREADS, m, blocks, G::LDS_BYTES, stream, done_s);
        return ring_launch_kernel(k_channelize_mfma_s16_ring_pairs<KS>, "k_channelize_mfma_s16_ring_pairs", G::THREADS, m, blocks, G::LDS_BYTES, stream, done);
    } else {
        set_error("lane pairs: %d k steps not instantiated (%d..14, 16)", KS, RG_PAIR_MIN_KS);
        return IQA_EINVAL;
    }
}

// The pacing words of the lane-pair launches: RG_PACE_WORDS x 4 bytes per device, library state (see the header's
// conventions), never freed.  Allocated and cleared -- synchronously -- at the first pair launch on a device that is
// NOT inside a stream capture (an allocation would invalidate the capture: such a launch runs unpaced, which is correct,
// only its workgroups may drift apart); every launch takes its own slice of the buffer, handed out round-robin, so two
// pair launches in flight on one device do not share words, and entries carry the launch's token, so nothing is reset
// between launches.
static unsigned int *ring_pace_buffer(unsigned int &token, int words, hipStream_t stream)
{
    static std::mutex mu;
    static unsigned int *buf[64] = {};
    static int next_off[64] = {};
    static unsigned int next_token = 1;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    token = next_token = (next_token % 0xFFFFFu) + 1;
    unsigned int *&b = buf[dev & 63];
    if (b == nullptr) {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return nullptr;
        }
        void *p = nullptr;
        if (hipMalloc(&p, RG_PACE_WORDS * sizeof(unsigned int)) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (hipMemset(p, 0, RG_PACE_WORDS * sizeof(unsigned int)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p);
            return nullptr;
        }
        b = static_cast<unsigned int *>(p);
    }
    if (words > RG_PACE_WORDS) return nullptr;
    int &off = next_off[dev & 63];
    if (off + words > RG_PACE_WORDS) off = 0;
    unsigned int *mine = b + off;
    off += (words + 63) & ~63;
    return mine;
}

bool mfma_ring_pairs_supported(int decimation, int k_first, int k_count, bool u8, bool acc64)
{
    // (15 k steps: the pair kernel would need 20 registers more than a wave has -- a spill's scratch loads would join
    // the counted vmcnt sequence of the issuing waves; 64-bit sums cost ~20 registers more: up to 14 k steps)
    return mfma_ring_mode(decimation, k_first, k_count, acc64, u8) == 1 && k_count >= RG_PAIR_MIN_KS && k_count != 15 && (!acc64 || k_count <= 14);
}

constexpr int RG_ROWS_MAX_KS = RG_ROWS_MAX_KS_C;  // 8*KS tap registers + the rest must stay within 168 (three waves on two SIMDs)

// 0: the ring kernels do not apply; 1: contiguous slots; 2: row-staged slots (int32 sums only)
int mfma_ring_mode(int decimation, int k_first, int k_count, bool acc64, bool u8)
{
    const int ks_all = (2 * decimation + 31) / 32;
    // (64-bit sums at 16 k steps do not fit 256 registers: a spill's scratch loads would join the counted vmcnt sequence)
    if (!u8 && decimation >= 4 && (decimation & 3) == 0 && ks_all <= (acc64 ? RG_MAX_KS - 1 : RG_MAX_KS) && k_first == 0 && k_count == ks_all) return 1;
    if (!acc64 && decimation >= 1 && k_count >= 1 && k_count <= RG_ROWS_MAX_KS && k_first >= 0 && k_first + k_count <= ks_all) return 2;
    return 0;
}

bool mfma_ring_supported(int decimation)
{
    const int ks = (2 * decimation + 31) / 32;
    return decimation >= 4 && (decimation & 3) == 0 && ks <= RG_MAX_KS;
}

// f(std::integral_constant<int, K>{}) for the K in LO..HI that equals ks: where a run-time k-step count becomes the
// template argument of a kernel.  ks must lie in LO..HI (the callers check it); `if constexpr` inside f decides which
// kernels exist for a K.
template <int LO, int HI, class F>
static auto with_ks(int ks, F &&f)
{
    if constexpr (LO < HI) {
        if (ks > LO) return with_ks<LO + 1, HI>(ks, f);
    }
    return f(std::integral_constant<int, LO>{});
}

template <int KS>
static constexpr size_t ring_bytes_of(bool rows, bool u8)
{
    return u8     ? static_cast<size_t>(RingGeo<KS, true, true>::R) * 2 * RingGeo<KS, true, true>::SLOT + RG_ACC_BYTES
           : rows ? static_cast<size_t>(RingGeo<KS, true>::R) * 2 * RingGeo<KS, true>::SLOT + RG_ACC_BYTES
                  : static_cast<size_t>(RingGeo<KS, false>::R) * 2 * RingGeo<KS, false>::SLOT + RG_ACC_BYTES;
}

size_t mfma_ring_lds_bytes(int ksteps, bool rows, bool u8)
{
    if (ksteps < 1 || ksteps > (rows ? RG_ROWS_MAX_KS : RG_MAX_KS)) return 0;
    return with_ks<1, RG_MAX_KS>(ksteps, [&](auto k) { return ring_bytes_of<decltype(k)::value>(rows, u8); });
}

// Every ring pass: 1..16 lanes (channels x tap-row groups) of one capture in one launch.  `lanes` holds n_lanes entries,
// the per-lane part of MfmaArgs; `a` carries what they share.
int mfma_ring_launch_multi(const MfmaArgs &a, const MfmaLane *lanes, int n_lanes, size_t lds, hipStream_t stream, bool rows, bool u8,
                           bool pairs, bool acc64)
{
    if (n_lanes < 1 || n_lanes > RG_MAX_LANES) {
        set_error("a multi-lane launch takes 1..%d lanes (got %d)", RG_MAX_LANES, n_lanes);
        return IQA_EINVAL;
    }
    if (pairs) {
        if (rows || u8 || (n_lanes & 1)) {
            set_error("lane pairs: contiguous int16 slots and an even number of lanes");
            return IQA_EINVAL;
        }
        for (int i = 0; i < n_lanes; i += 2)
            if (lanes[i].afrag == nullptr || (lanes[i + 1].afrag != nullptr && lanes[i].col_shift < lanes[i + 1].col_shift)) {
                set_error("lane pairs: lane %d must exist and have the larger (or the same) tap-row group of its pair", i);
                return IQA_EINVAL;
            }
    }
    RingMultiArgs m;
    m.c = a;
    m.n_lanes = n_lanes;
    for (int i = 0; i < n_lanes; ++i) m.lane[i] = lanes[i];
    for (int i = n_lanes; i < RG_MAX_LANES; ++i) m.lane[i] = m.lane[0];
    // Which lanes may skip the q2*hi product.  Pairs: the kernel variant skips it for every pair's FIRST lane at compile time,
    // so it is taken only when every first lane is high-byte-only and no second lane is (what the host's pairing of a
    // tap-row group's two lanes gives); otherwise nothing is skipped.  One lane per workgroup: the variant that asks the
    // lane's flag, when any lane has it.
    // rotated fragments are for the one kernel that knows the rotation; any other would multiply the wrong rows
    for (int i = 0; i < n_lanes; ++i)
        if (lanes[i].zrot != 0 && !(n_lanes == 1 && !pairs && !lanes[i].high_taps_only && (lanes[i].zrot & 3) == 0 && lanes[i].zrot <= 32 &&
                                    mfma_ring_zedge_supported(a.D, a.k_first, a.ksteps, rows, u8, acc64))) {
            set_error("lane %d: rotated tap fragments (rot %d) need a single-lane launch of the half-step kernels (iqa_mfma_ring_zero_rows) and a rot of 4, 8 .. 32", i, lanes[i].zrot);
            return IQA_EINVAL;
        }
    bool skipk = false;
    if (!u8) {
        if (pairs) {
            skipk = true;
            for (int i = 0; i < n_lanes; i += 2)
                if (!lanes[i].high_taps_only || (lanes[i + 1].afrag != nullptr && lanes[i + 1].high_taps_only)) skipk = false;
        } else {
            for (int i = 0; i < n_lanes; ++i) skipk = skipk || lanes[i].high_taps_only != 0;
        }
    }
    if (!skipk)
        for (int i = 0; i < RG_MAX_LANES; ++i) m.lane[i].high_taps_only = 0;
    const long long ranges = (a.n_out + a.range - 1) / a.range;
    const long long groups = (ranges + 7) / 8;  // ranges are dealt to the 8 XCD classes: workgroup b -> class b % 8
    const unsigned blocks = static_cast<unsigned>(groups * (pairs ? n_lanes / 2 : n_lanes) * 8);
    if (a.ksteps < 1 || a.ksteps > RG_MAX_KS) {
        set_error("ring kernel: %d k steps not instantiated (1..%d)", a.ksteps, RG_MAX_KS);
        return IQA_EINVAL;
    }
    if (pairs) {
        m.c.pace = nullptr;
        m.c.pace = ring_pace_buffer(m.c.pace_token, static_cast<int>(std::min<long long>(groups * 8 * (n_lanes / 2), RG_PACE_WORDS + 1)), stream);
        return with_ks<1, RG_MAX_KS>(a.ksteps, [&](auto k) { return ring_launch_pairs<decltype(k)::value>(m, blocks, stream, acc64, skipk); });
    }
    return with_ks<1, RG_MAX_KS>(a.ksteps, [&](auto k) {
        return ring_launch_multi<decltype(k)::value>(m, blocks, lds, stream, rows, u8, acc64, skipk);
    });
}

const char *mfma_ring_last_kernel() { return g_ring_last_kernel; }

// A single-lane launch over these k steps takes k_channelize_mfma_s16_ring_multi_half (whose ZEDGE variant reads rotated fragments)
bool mfma_ring_zedge_supported(int decimation, int k_first, int k_count, bool rows, bool u8, bool acc64)
{
    const int rem = (2 * decimation) & 31;
    return !rows && !u8 && !acc64 && mfma_ring_mode(decimation, k_first, k_count, acc64, u8) == 1 && k_count <= 8 && rem != 0 && rem <= 16;
}

}  // namespace iqa
