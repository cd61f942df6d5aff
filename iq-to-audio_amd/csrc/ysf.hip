// ysf.hip -- the frames of YSF (System Fusion) channels behind their frame sync (--find-ysf), for gfx950:
// the levels and the 960 sliced bits of every kept sync hit, the frame information channel (FICH) of every sliced frame, and
// the data channels (DCH) behind it.
//
// Specification (plane the integrator plane v of section 25 at 4800 symbols/s, n samples; a hit (m, s): m where sync symbol 0
// ends, s the sign of its correlation, a negative hit being the same word with the spectrum inverted; o[i] = rint(i sps),
// i = 0 .. 479; s_i the level of sync symbol i, in -3 -1 1 3):
//   k_ysf_slice, per hit:
//     valid = 0 if m + o[0] < 0, else the number of i with m + o[i] < n (a prefix); valid < 20: all bits 0, A = Dc = 0
//     x_i = v[m + o[i]], i = 0 .. 19; P = sum x_i, Q = sum s_i x_i; Dc = 31 P - 3 Q, A = s (15 Q - 9 P)   (int64; the least
//     squares fit of x_i to DC + L s s_i with sum s_i = 12 and sum s_i^2 = 124: the determinant 20 * 124 - 12^2 = 2336 less its
//     factor 4, so Dc is 584 times the DC and A 584 times the outer level 3 L)
//     symbol i < valid: d = s (584 v[m + o[i]] - Dc); its first bit (d < 0), its second (3 |d| >= 2 A); i >= valid: 0, 0
//     bits: u32[30], symbol i the frame bits 2 i, 2 i + 1, the first sent bit the MSB of word 0; levels: A, Dc, valid
//   the code: rate 1/2, K = 5; input bit d with the memory d1 .. d4 sends g1 = d ^ d3 ^ d4, then g2 = d ^ d1 ^ d2 ^ d4; a
//     block ends in four zero bits.  The state is d1 << 3 | d2 << 2 | d3 << 1 | d4, so state t has the predecessors
//     (t & 7) << 1 and (t & 7) << 1 | 1 on the input t >> 3.  Viterbi on the Hamming distance of the dibits, from state 0 (every
//     other state starts 1000 away) to state 0; on equal metrics the predecessor with the smaller state index survives
//   k_ysf_fich, per frame: coded dibit i = 0 .. 99 is the channel dibit 20 (i mod 5) + i / 5 of the frame bits 40 .. 239; the
//     96 decoded bits are four Golay(24,12,8) words (protocol.h's pl_golay(d, 12)): the nearest of the 4096 codewords, the
//     smaller data on equal distance, corrected at a distance of 3 or less, else refused with its raw top 12 bits kept
//     fich: u32[2]: the 48 data bits, the top 16 of word 1 the CRC; rec: int32[5] = status (0 clean, 1 corrected, 2 a word
//     refused), the Viterbi metric, the words corrected, the words refused, the bits changed in the corrected words
//   k_ysf_decode, per frame and class; payload block p is the frame bits 240 + 144 p .. + 143:
//     1: DCH-a the first 72 bits of every block, DCH-b the 72 behind them; 180 dibits each, coded dibit i the channel dibit
//     20 (i mod 9) + i / 9; 176 decoded bits each       2: DCH-a alone
//     3: the first 40 bits of every block, 100 dibits, coded dibit i the channel dibit 20 (i mod 5) + i / 5; 96 decoded bits
//     0 and over 3: zeros
//     info: u32[12]: DCH-a in words 0 .. 5, DCH-b in 6 .. 11, the block's first bit the MSB of its first word; rec: int32[4] =
//     the class, the metric of DCH-a, of DCH-b, 0
//
// k_ysf_slice is protocol.h's pl_slice_frame on YsfSlice, one wave per hit: eight strided rounds, 30 lanes pack the words.  The
// code, its decoder of one trellis in sixteen lanes (pl_viterbi16, without erasures; four survivor words for 100 steps, six for
// 180) and the rule for a frame past K (pl_frame) are protocol.h's as well.  k_ysf_fich is a wave for four frames, k_ysf_decode a
// wave for the two blocks of two frames; no lane leaves before the barrier.  The Golay search is sixteen lanes by 256 codewords,
// the minimum over (distance, data) by shuffles.  LDS holds only the frames' words, written before the one barrier and read after
// it.  Plain C++ stores, no inline assembly, no atomics, no mutable statics.
#include "protocol.h"

namespace iqa {

constexpr int Y_WAVE = 64;
constexpr int Y_OFFSETS = IQA_YSF_OFFSETS;  // 480
constexpr int Y_WORDS = IQA_YSF_WORDS;      // 30 words of 32 bits
constexpr int Y_ROUNDS = (Y_OFFSETS + Y_WAVE - 1) / Y_WAVE;  // 8
constexpr int Y_FICH_REC = IQA_YSF_FICH_RECORD;  // 5
constexpr int Y_INFO = IQA_YSF_INFO;        // 12
constexpr int Y_REC = IQA_YSF_RECORD;       // 4
constexpr int Y_SYNC_SYMBOLS = 20;
constexpr unsigned long long Y_SYNC = 0xD471C9634Dull;
constexpr int Y_FICH_STEPS = 100, Y_DCH_STEPS = 180, Y_DCH2_STEPS = 100;
constexpr int Y_FICH_FIRST = 40, Y_PAYLOAD_FIRST = 240, Y_PAYLOAD_BLOCK = 144;

static_assert(2 * Y_OFFSETS == 32 * Y_WORDS && Y_ROUNDS == 8, "480 symbols: eight rounds of a wave, 30 words");
static_assert(Y_INFO == 12 && 32 * 6 >= Y_DCH_STEPS && 32 * 4 >= Y_FICH_STEPS, "six words to a DCH block, four to the FICH");

struct YsfOffsets {
    int o[Y_OFFSETS];
};

// protocol.h's slicer on the levels of the sync word: Dc = 31 P - 3 Q, A = s (15 Q - 9 P) at the scale 584
struct YsfSlice {
    static constexpr int OFFSETS = Y_OFFSETS, WORDS = Y_WORDS, SYNC_SYMBOLS = Y_SYNC_SYMBOLS, OUTER = 3;
    static constexpr long long SCALE = 584, A_Q = 15, A_P = -9, D_P = 31, D_Q = -3;
    __host__ __device__ static constexpr int weight(int i) { return pl_sync_level(Y_SYNC, Y_SYNC_SYMBOLS, i); }
    __device__ static constexpr unsigned flip(int) { return 0u; }
};

constexpr int y_sync_sum(bool squares)
{
    int sum = 0;
    for (int i = 0; i < Y_SYNC_SYMBOLS; ++i) sum += squares ? YsfSlice::weight(i) * YsfSlice::weight(i) : YsfSlice::weight(i);
    return sum;
}
static_assert(y_sync_sum(false) == 12 && y_sync_sum(true) == 124, "sum s_i = 12 and sum s_i^2 = 124: Dc = 31 P - 3 Q, A = s (15 Q - 9 P)");
static_assert(20 * 124 - 12 * 12 == 4 * YsfSlice::SCALE && 124 == 4 * YsfSlice::D_P && 12 == -4 * YsfSlice::D_Q && 20 * 3 == 4 * YsfSlice::A_Q &&
              12 * 3 == -4 * YsfSlice::A_P, "the fit, less its factor 4");
static_assert((YsfSlice::A_Q * 124 - YsfSlice::A_P * 20) * PL_V_MAX * 3 < (1LL << 50) && YsfSlice::SCALE * PL_V_MAX * 2 * 3 < (1LL << 50),
              "15 Q - 9 P, 584 y - Dc and 3 |d| stay far inside int64");

// ---- Golay(24,12,8) ---------------------------------------------------------------------------------------------------------------

// the codeword of the 12-bit value d is hi[d >> 4] ^ lo[d & 15]
struct YGolay {
    unsigned hi[256], lo[16];
    constexpr unsigned word(unsigned d) const { return hi[d >> 4] ^ lo[d & 15u]; }
};

constexpr YGolay y_golay_tables()
{
    YGolay t{};
    for (unsigned d = 0; d < 256; ++d) t.hi[d] = pl_golay(d << 4, 12);
    for (unsigned d = 0; d < 16; ++d) t.lo[d] = pl_golay(d, 12);
    return t;
}

constexpr YGolay Y_GOLAY_HOST = y_golay_tables();
static_assert(Y_GOLAY_HOST.word(1) == 0x0018EBu, "the word of data 1");
static_assert(pl_golay_distance(Y_GOLAY_HOST, 4096) == 8, "the 4096 codewords lie 8 apart at the least: a word within 3 of one is within 3 of no other");
__device__ const YGolay Y_GOLAY = y_golay_tables();

// ---- the convolutional code ---------------------------------------------------------------------------------------------------------

// the channel dibit of a block of 20 R dibits that is dibit i of the coded stream
__host__ __device__ constexpr int y_deinterleave(int i, int rows) { return 20 * (i % rows) + i / rows; }

constexpr bool y_permutes(int rows)
{
    bool seen[180] = {};
    for (int i = 0; i < 20 * rows; ++i) {
        const int at = y_deinterleave(i, rows);
        if (at < 0 || at >= 20 * rows || seen[at]) return false;
        seen[at] = true;
    }
    return true;
}
static_assert(y_permutes(5) && y_permutes(9), "the de-interleaver is a permutation of 0 .. 99 and of 0 .. 179");

// the dibit at the frame bits b, b + 1 (b even) of a frame's words
__device__ __forceinline__ unsigned y_dibit(const unsigned *w, int b) { return (w[b >> 5] >> (30 - (b & 31))) & 3u; }

__global__ __launch_bounds__(Y_WAVE) void k_ysf_slice(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                                      YsfOffsets off, unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    pl_slice_frame<YsfSlice>(plane, n, hits, off.o, bits_out, levels_out);
}

// four frames to a wave, one to every sixteen lanes
__global__ __launch_bounds__(Y_WAVE) void k_ysf_fich(const unsigned *__restrict__ bits, long long count, unsigned *__restrict__ fich_out,
                                                     int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[Y_WAVE / PL_GROUP][Y_WORDS + 2];
    const int lane = threadIdx.x, group = lane / PL_GROUP, sub = lane % PL_GROUP;
    const auto [mine, id] = pl_frame(4LL * blockIdx.x + group, count);
    s_w[group][sub] = bits[Y_WORDS * id + sub];
    s_w[group][sub + PL_GROUP] = sub + PL_GROUP < Y_WORDS ? bits[Y_WORDS * id + sub + PL_GROUP] : 0u;
    __syncthreads();
    const unsigned *w = s_w[group];
    unsigned out[4];
    const int metric = pl_viterbi16<4, false>(Y_FICH_STEPS, [w](int t) { return y_dibit(w, Y_FICH_FIRST + 2 * y_deinterleave(t, 5)); }, out);
    const unsigned words[4] = {out[0] >> 8, (out[0] & 0xFFu) << 16 | out[1] >> 16, (out[1] & 0xFFFFu) << 8 | out[2] >> 24, out[2] & 0xFFFFFFu};
    unsigned data[4];
    int corrected = 0, refused = 0, changed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned best = 0xFFFFFFFFu;
#pragma unroll 1
        for (int h = 0; h < 16; ++h) {
            const unsigned top = static_cast<unsigned>(16 * sub + h), near = words[j] ^ Y_GOLAY.hi[top];
            for (int k = 0; k < 16; ++k) {
                const unsigned key = pl_popcount(near ^ Y_GOLAY.lo[k]) << 12 | top << 4 | static_cast<unsigned>(k);
                best = key < best ? key : best;
            }
        }
        const unsigned key = pl_group_min16(best);
        const int distance = static_cast<int>(key >> 12);
        data[j] = key & 0xFFFu;
        if (distance > 3) {
            ++refused;
            data[j] = words[j] >> 12;
        } else if (distance > 0) {
            ++corrected;
            changed += distance;
        }
    }
    if (mine && sub == 0) {
        fich_out[2 * id] = data[0] << 20 | data[1] << 8 | data[2] >> 4;
        fich_out[2 * id + 1] = ((data[2] & 15u) << 12 | data[3]) << 16;
        int *e = rec_out + Y_FICH_REC * id;
        e[0] = refused > 0 ? 2 : (metric > 0 || corrected > 0) ? 1 : 0;
        e[1] = metric;
        e[2] = corrected;
        e[3] = refused;
        e[4] = changed;
    }
}

// two frames to a wave: the lanes 0 .. 15 and 16 .. 31 take DCH-a and DCH-b of the first, the lanes 32 .. 63 those of the second
__global__ __launch_bounds__(Y_WAVE) void k_ysf_decode(const unsigned *__restrict__ bits, const unsigned char *__restrict__ classes, long long count,
                                                       unsigned *__restrict__ info_out, int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[2][2 * PL_GROUP];
    const int lane = threadIdx.x, slot = lane / (2 * PL_GROUP), block = (lane / PL_GROUP) & 1, sub = lane % PL_GROUP;
    const auto [mine, id] = pl_frame(2LL * blockIdx.x + slot, count);
    const int at = lane % (2 * PL_GROUP);
    s_w[slot][at] = at < Y_WORDS ? bits[Y_WORDS * id + at] : 0u;
    __syncthreads();
    const unsigned *w = s_w[slot];
    const int given = classes[id];
    const int cls = given <= 3 ? given : 0;
    const int steps = cls == 1 || (cls == 2 && block == 0) ? Y_DCH_STEPS : cls == 3 && block == 0 ? Y_DCH2_STEPS : 0;
    const int rows = cls == 3 ? 5 : 9, part = cls == 3 ? 40 : 72, first = Y_PAYLOAD_FIRST + 72 * block;
    unsigned out[6];
    const int metric = pl_viterbi16<6, false>(steps, [=](int t) {
        const int b = 2 * y_deinterleave(t, rows);  // the bit of the data channel; it lies in payload block b / part
        return y_dibit(w, first + Y_PAYLOAD_BLOCK * (b / part) + b % part);
    }, out);
    const int metric_a = __shfl(metric, 0, 2 * PL_GROUP), metric_b = __shfl(metric, PL_GROUP, 2 * PL_GROUP);
    if (mine) {
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) word = sub == k ? out[k] : word;
        if (sub < 6) info_out[Y_INFO * id + 6 * block + sub] = word;
        if (block == 0 && sub == 0) {
            int *e = rec_out + Y_REC * id;
            e[0] = cls;
            e[1] = metric_a;
            e[2] = metric_b;
            e[3] = 0;
        }
    }
}

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_ysf_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_YSF_OFFSETS],
                             void *bits_dev, void *levels_dev, void *stream)
{
    YsfOffsets off;
    if (const int rc = pl_check_lengths(n, K)) return rc;
    if (const int rc = pl_copy_offsets(offsets, Y_OFFSETS, 0, "offsets", off.o)) return rc;
    if (n == 0 || K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!plane_dev || !hits_dev || !bits_dev || !levels_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_ysf_slice, dim3(static_cast<unsigned>(K)), dim3(Y_WAVE), 0, as_stream(stream), static_cast<const int *>(plane_dev),
                       (long long)n, static_cast<const long long *>(hits_dev), off, static_cast<unsigned *>(bits_dev),
                       static_cast<long long *>(levels_dev));
    return check_launch("k_ysf_slice");
}

extern "C" int iqa_ysf_fich(const void *bits_dev, int64_t K, void *fich_dev, void *rec_dev, void *stream)
{
    if (const int rc = pl_check_lengths(0, K)) return rc;
    if (K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!bits_dev || !fich_dev || !rec_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_ysf_fich, dim3(static_cast<unsigned>((K + 3) / 4)), dim3(Y_WAVE), 0, as_stream(stream),
                       static_cast<const unsigned *>(bits_dev), (long long)K, static_cast<unsigned *>(fich_dev), static_cast<int *>(rec_dev));
    return check_launch("k_ysf_fich");
}

extern "C" int iqa_ysf_decode(const void *bits_dev, const void *classes_dev, int64_t K, void *info_dev, void *rec_dev, void *stream)
{
    if (const int rc = pl_check_lengths(0, K)) return rc;
    if (K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!bits_dev || !classes_dev || !info_dev || !rec_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_ysf_decode, dim3(static_cast<unsigned>((K + 1) / 2)), dim3(Y_WAVE), 0, as_stream(stream),
                       static_cast<const unsigned *>(bits_dev), static_cast<const unsigned char *>(classes_dev), (long long)K,
                       static_cast<unsigned *>(info_dev), static_cast<int *>(rec_dev));
    return check_launch("k_ysf_decode");
}
