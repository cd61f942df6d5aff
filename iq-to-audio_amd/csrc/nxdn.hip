// nxdn.hip -- the frames of NXDN channels behind their frame sync (--find-nxdn), for gfx950: the levels and
// the 384 descrambled bits of every kept sync hit, and the SACCH, the two FACCH1s or the outbound CAC behind the LICH.
//
// Specification (plane the integrator plane v of section 25 at 4800 or 2400 symbols/s, n samples; a hit (m, s): m where sync
// symbol 0 ends, s the sign of its correlation, a negative hit being the same word with the spectrum inverted; o[i] = rint(i sps),
// i = 0 .. 191; s_i the level of sync symbol i, in -3 -1 1 3):
//   k_nxdn_slice, per hit:
//     valid = 0 if m + o[0] < 0, else the number of i with m + o[i] < n (a prefix); valid < 10: all bits 0, A = Dc = 0
//     x_i = v[m + o[i]], i = 0 .. 9; P = sum x_i, Q = sum s_i x_i; Dc = 37 P, A = s 15 Q   (int64; the least squares fit of x_i
//     to DC + L s s_i with sum s_i = 0 and sum s_i^2 = 74: DC = P / 10 and L = s Q / 74, at the common scale 370 = 37 * 10 =
//     5 * 74, so Dc is 370 times the DC and A 370 times the outer level 3 L)
//     symbol i < valid: d = s (370 v[m + o[i]] - Dc); its first bit (d < 0), its second (3 |d| >= 2 A); i >= valid: 0, 0
//     the scrambler: one bit per symbol from symbol 10 on, 0 0 1 0 0 1 1 1 0 and then b[k] = b[k - 5] ^ b[k - 9]; where it is 1
//     the first bit of symbol 10 + k < valid is inverted (the symbol's sign), so ``bits`` is descrambled
//     bits: u32[12], symbol i the frame bits 2 i, 2 i + 1, the first sent bit the MSB of word 0; levels: A, Dc, valid
//   the code: section 32's (ysf.hip): rate 1/2, K = 5, g1 = d ^ d3 ^ d4, then g2 = d ^ d1 ^ d2 ^ d4, four zero tail bits, the
//     state d1 << 3 | d2 << 2 | d3 << 1 | d4.  New here: the coded bits c[j] (g1 of step t at 2 t, g2 at 2 t + 1) are punctured
//     and interleaved bit by bit: the p-th coded bit that is sent is channel bit C (p mod D) + p / D of its block.  Viterbi on
//     the Hamming distance, a punctured bit adding 0 to both branches, from state 0 (every other state starts 1000 away) to state
//     0; on equal metrics the predecessor with the smaller state index survives
//   k_nxdn_decode, per frame and class mask:
//     1 SACCH: frame bits 36 .. 95, 36 steps, punctured j mod 6 = 5, D = 12, C = 5
//     2 FACCH1-a: 96 .. 239; 4 FACCH1-b: 240 .. 383; 96 steps each, punctured j mod 4 = 1, D = 9, C = 16
//     8 CAC (alone): 36 .. 335, 175 steps, punctured j mod 14 = 3 and 11, D = 12, C = 25
//     a mask over 15, or 8 with another bit: nothing is read, the recorded mask is 0
//     info: u32[14]: SACCH words 0 .. 1, FACCH1-a 2 .. 4, FACCH1-b 5 .. 7, CAC 8 .. 13, a block's first bit the MSB of its first
//     word, zeros elsewhere; rec: int32[4] = the mask, the metric of the SACCH or the CAC, of FACCH1-a, of FACCH1-b
//
// k_nxdn_slice is protocol.h's pl_slice_frame on NxdnSlice, one wave per hit: three whole rounds, the scrambler bit of a symbol
// from a constexpr table, 12 lanes pack the words.  The code, its decoder of one trellis in sixteen lanes (pl_viterbi16, with
// erasures: nx_fetch says which bits of a step were sent) and the rule for a frame past K (pl_frame) are protocol.h's as well.
// k_nxdn_decode is a wave to a frame: the lanes 0 .. 15 run the SACCH or the CAC, 16 .. 31 and 32 .. 47 the two FACCH1s,
// 48 .. 63 nothing (0 steps).  The mask is the same in the whole wave, so the wave takes one of three sizes of the decoder: six
// survivor words with a CAC, three with a FACCH1, two for a SACCH alone.  No lane leaves before the barrier.  LDS holds only the
// frame's words, written before the one barrier and read after it.  Plain C++ stores, no inline assembly, no atomics, no mutable
// statics.
#include "protocol.h"

namespace iqa {

constexpr int NX_WAVE = 64;
constexpr int NX_OFFSETS = IQA_NXDN_OFFSETS;  // 192
constexpr int NX_WORDS = IQA_NXDN_WORDS;      // 12 words of 32 bits
constexpr int NX_ROUNDS = NX_OFFSETS / NX_WAVE;  // 3
constexpr int NX_INFO = IQA_NXDN_INFO;        // 14
constexpr int NX_REC = IQA_NXDN_RECORD;       // 4
constexpr int NX_SYNC_SYMBOLS = 10;
constexpr unsigned NX_SYNC = 0xCDF59u;
constexpr int NX_SCRAMBLED = NX_OFFSETS - NX_SYNC_SYMBOLS;  // 182 scrambler bits

static_assert(NX_ROUNDS * NX_WAVE == NX_OFFSETS && 2 * NX_OFFSETS == 32 * NX_WORDS, "192 symbols: three rounds of a wave, 12 words");
static_assert(NX_INFO == 2 + 3 + 3 + 6 && NX_REC == 4, "two words to the SACCH, three to a FACCH1, six to the CAC");

struct NxdnOffsets {
    int o[NX_OFFSETS];
};

// ---- the scrambler ------------------------------------------------------------------------------------------------------------------

// bit i mod 32 of sym[i / 32]: whether the sign of symbol i is inverted; mask: the same as an XOR over the frame's words
struct NxScramble {
    unsigned sym[NX_OFFSETS / 32], mask[NX_WORDS];
};

constexpr NxScramble nx_scramble()
{
    NxScramble t{};
    bool b[NX_SCRAMBLED] = {false, false, true, false, false, true, true, true, false};
    for (int k = 9; k < NX_SCRAMBLED; ++k) b[k] = b[k - 5] != b[k - 9];
    for (int k = 0; k < NX_SCRAMBLED; ++k) {
        if (!b[k]) continue;
        const int i = NX_SYNC_SYMBOLS + k;
        t.sym[i >> 5] |= 1u << (i & 31);
        t.mask[(2 * i) >> 5] |= 1u << (31 - ((2 * i) & 31));
    }
    return t;
}

constexpr int nx_scramble_ones(const NxScramble &t)
{
    int ones = 0;
    for (int w = 0; w < NX_WORDS; ++w) ones += static_cast<int>(pl_popcount(t.mask[w]));
    return ones;
}

constexpr NxScramble NX_SCRAMBLE_HOST = nx_scramble();
static_assert(nx_scramble_ones(NX_SCRAMBLE_HOST) == 92, "the scrambler inverts 92 of the 182 symbols");
static_assert(NX_SCRAMBLE_HOST.mask[0] == 0x00000082u && NX_SCRAMBLE_HOST.mask[1] == 0xA0888A00u && NX_SCRAMBLE_HOST.mask[2] == 0xA2A8828Au &&
              NX_SCRAMBLE_HOST.mask[3] == 0x82022008u && NX_SCRAMBLE_HOST.mask[4] == 0x8A20AAA2u && NX_SCRAMBLE_HOST.mask[5] == 0x8208228Au &&
              NX_SCRAMBLE_HOST.mask[6] == 0xAA082888u && NX_SCRAMBLE_HOST.mask[7] == 0x2828000Au && NX_SCRAMBLE_HOST.mask[8] == 0x02822028u &&
              NX_SCRAMBLE_HOST.mask[9] == 0x822AAA20u && NX_SCRAMBLE_HOST.mask[10] == 0x2280A88Au && NX_SCRAMBLE_HOST.mask[11] == 0x08A0AA02u,
              "the scrambler as a mask over the 48 bytes of a frame");
__device__ const NxScramble NX_SCRAMBLE = nx_scramble();

// ---- the slicer -----------------------------------------------------------------------------------------------------------------------

// protocol.h's slicer on the levels of the sync word: Dc = 37 P, A = s 15 Q at the scale 370; the scrambler inverts a symbol's sign
struct NxdnSlice {
    static constexpr int OFFSETS = NX_OFFSETS, WORDS = NX_WORDS, SYNC_SYMBOLS = NX_SYNC_SYMBOLS, OUTER = 3;
    static constexpr long long SCALE = 370, A_Q = 15, A_P = 0, D_P = 37, D_Q = 0;
    __host__ __device__ static constexpr int weight(int i) { return pl_sync_level(NX_SYNC, NX_SYNC_SYMBOLS, i); }
    __device__ static unsigned flip(int i) { return ((NX_SCRAMBLE.sym[i >> 5] >> (i & 31)) & 1u) << 1; }
};

constexpr int nx_sync_sum(int power)
{
    int sum = 0;
    for (int i = 0; i < NX_SYNC_SYMBOLS; ++i) {
        const int s = NxdnSlice::weight(i);
        sum += power == 2 ? s * s : power == 1 ? s : s < 0 ? -s : s;
    }
    return sum;
}
static_assert(nx_sync_sum(1) == 0 && nx_sync_sum(2) == 74, "sum s_i = 0 and sum s_i^2 = 74: the fit is DC = P / 10, L = s Q / 74");
static_assert(NxdnSlice::SCALE == NxdnSlice::D_P * NX_SYNC_SYMBOLS && NxdnSlice::SCALE * 3 == NxdnSlice::A_Q * 74, "at the scale 370: Dc = 37 P, A = s 15 Q");
static_assert(NxdnSlice::A_Q * nx_sync_sum(0) * PL_V_MAX * 3 < (1LL << 50) && NxdnSlice::SCALE * PL_V_MAX * 2 * 3 < (1LL << 50),
              "15 Q, 370 x - Dc and 3 |d| stay far inside int64");

// ---- the convolutional code, its puncturing and its interleave -------------------------------------------------------------------------

// A block's coder: STEPS trellis steps; of every PERIOD coded bits those at Q0 and Q1 are not sent (Q1 = PERIOD: one alone);
// the p-th sent bit is channel bit C (p mod D) + p / D of the D C bits from frame bit FIRST on.
template <int STEPS_, int PERIOD_, int Q0_, int Q1_, int D_, int C_>
struct NxCode {
    static constexpr int STEPS = STEPS_, PERIOD = PERIOD_, Q0 = Q0_, Q1 = Q1_, D = D_, C = C_;
    static constexpr int CUT = Q1_ < PERIOD_ ? 2 : 1;  // punctured bits to a period
    __host__ __device__ static constexpr bool punctured(int j) { return j % PERIOD == Q0 || j % PERIOD == Q1; }
    // the sent bits in front of coded bit j
    __host__ __device__ static constexpr int sent_before(int j)
    {
        const int r = j % PERIOD;
        return j - CUT * (j / PERIOD) - (r > Q0 ? 1 : 0) - (r > Q1 ? 1 : 0);
    }
    __host__ __device__ static constexpr int channel_bit(int p) { return C * (p % D) + p / D; }
    static constexpr int SENT = sent_before(2 * STEPS_);
};

using NxSacch = NxCode<36, 6, 5, 6, 12, 5>;
using NxFacch1 = NxCode<96, 4, 1, 4, 9, 16>;
using NxCac = NxCode<175, 14, 3, 11, 12, 25>;
constexpr int NX_SACCH_FIRST = 36, NX_FACCH1_A_FIRST = 96, NX_FACCH1_B_FIRST = 240, NX_CAC_FIRST = 36;

template <class Code>
constexpr bool nx_permutes()
{
    bool seen[Code::D * Code::C] = {};
    int sent = 0;
    for (int j = 0; j < 2 * Code::STEPS; ++j) {
        if (Code::punctured(j)) continue;
        if (Code::sent_before(j) != sent) return false;
        const int at = Code::channel_bit(sent++);
        if (at < 0 || at >= Code::D * Code::C || seen[at]) return false;
        seen[at] = true;
    }
    return sent == Code::D * Code::C && sent == Code::SENT;
}
static_assert(NxSacch::SENT == 60 && NxFacch1::SENT == 144 && NxCac::SENT == 300, "72 - 12, 192 - 48 and 350 - 50 coded bits are sent");
static_assert(nx_permutes<NxSacch>() && nx_permutes<NxFacch1>() && nx_permutes<NxCac>(), "the three interleavers are permutations of their blocks");
static_assert(NX_SACCH_FIRST + NxSacch::SENT == NX_FACCH1_A_FIRST && NX_FACCH1_A_FIRST + NxFacch1::SENT == NX_FACCH1_B_FIRST &&
              NX_FACCH1_B_FIRST + NxFacch1::SENT == 32 * NX_WORDS && NX_CAC_FIRST + NxCac::SENT <= 32 * NX_WORDS, "the blocks lie inside the frame's words");

// step t of a block: its received dibit in the bits 1 .. 0, and in the bits 3 .. 2 which of the two were sent
template <class Code>
__device__ __forceinline__ unsigned nx_fetch(const unsigned *w, int first, int t)
{
    unsigned out = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int j = 2 * t + k;
        const bool sent = !Code::punctured(j);
        const int at = first + Code::channel_bit(sent ? Code::sent_before(j) : 0);
        out |= sent ? (4u | pl_bit(w, at)) << (1 - k) : 0u;
    }
    return out;
}

__global__ __launch_bounds__(NX_WAVE) void k_nxdn_slice(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                                        NxdnOffsets off, unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    pl_slice_frame<NxdnSlice>(plane, n, hits, off.o, bits_out, levels_out);
}

// a frame to a wave: the lanes 0 .. 15 take the SACCH or the CAC, 16 .. 31 FACCH1-a, 32 .. 47 FACCH1-b, 48 .. 63 nothing
__global__ __launch_bounds__(NX_WAVE) void k_nxdn_decode(const unsigned *__restrict__ bits, const unsigned char *__restrict__ classes, long long count,
                                                         unsigned *__restrict__ info_out, int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[PL_GROUP];
    const int lane = threadIdx.x, group = lane / PL_GROUP, sub = lane % PL_GROUP;
    const auto [mine, id] = pl_frame(blockIdx.x, count);
    if (lane < PL_GROUP) s_w[lane] = lane < NX_WORDS ? bits[NX_WORDS * id + lane] : 0u;
    __syncthreads();
    const unsigned *w = s_w;
    const int given = classes[id];
    const int cls = (given > 15 || ((given & IQA_NXDN_CAC) != 0 && given != IQA_NXDN_CAC)) ? 0 : given;  // (the same in the whole wave)
    const bool cac = cls == IQA_NXDN_CAC;
    unsigned out[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    int metric;
    if (cac) {
        metric = pl_viterbi16<6, true>(group == 0 ? NxCac::STEPS : 0, [w](int t) { return nx_fetch<NxCac>(w, NX_CAC_FIRST, t); }, out);
    } else {
        const int steps = group == 0 ? (cls & IQA_NXDN_SACCH ? NxSacch::STEPS : 0)
                                     : group == 1 ? (cls & IQA_NXDN_FACCH1_A ? NxFacch1::STEPS : 0)
                                                  : group == 2 ? (cls & IQA_NXDN_FACCH1_B ? NxFacch1::STEPS : 0) : 0;
        const int first = group == 2 ? NX_FACCH1_B_FIRST : NX_FACCH1_A_FIRST;
        if (cls & (IQA_NXDN_FACCH1_A | IQA_NXDN_FACCH1_B)) {
            unsigned three[3];
            metric = pl_viterbi16<3, true>(steps, [=](int t) {
                const unsigned sacch = nx_fetch<NxSacch>(w, NX_SACCH_FIRST, t < NxSacch::STEPS ? t : 0);
                const unsigned facch = nx_fetch<NxFacch1>(w, first, t);
                return group == 0 ? sacch : facch;
            }, three);
            out[0] = three[0], out[1] = three[1], out[2] = three[2];
        } else {
            unsigned two[2];
            metric = pl_viterbi16<2, true>(steps, [w](int t) { return nx_fetch<NxSacch>(w, NX_SACCH_FIRST, t); }, two);
            out[0] = two[0], out[1] = two[1];
        }
    }
    const int metric_0 = __shfl(metric, 0), metric_a = __shfl(metric, PL_GROUP), metric_b = __shfl(metric, 2 * PL_GROUP);
    if (mine) {
        unsigned *e = info_out + NX_INFO * id;
        if (group == 0 && sub < 8) {
            // the words 0 .. 1 (SACCH) from the lanes 0 .. 1, the words 8 .. 13 (CAC) from the lanes 2 .. 7
            const int k = sub < 2 ? sub : sub - 2;
            unsigned word = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) word = k == q ? out[q] : word;
            e[sub < 2 ? sub : sub + 6] = (sub < 2) == cac ? 0u : word;
        } else if ((group == 1 || group == 2) && sub < 3) {
            unsigned word = 0;
#pragma unroll
            for (int q = 0; q < 3; ++q) word = sub == q ? out[q] : word;
            e[2 + 3 * (group - 1) + sub] = word;
        }
        if (lane == 0) {
            int *r = rec_out + NX_REC * id;
            r[0] = cls;
            r[1] = metric_0;
            r[2] = metric_a;
            r[3] = metric_b;
        }
    }
}

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_nxdn_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_NXDN_OFFSETS],
                              void *bits_dev, void *levels_dev, void *stream)
{
    NxdnOffsets off;
    if (const int rc = pl_check_lengths(n, K)) return rc;
    if (const int rc = pl_copy_offsets(offsets, NX_OFFSETS, 0, "offsets", off.o)) return rc;
    if (n == 0 || K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!plane_dev || !hits_dev || !bits_dev || !levels_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_nxdn_slice, dim3(static_cast<unsigned>(K)), dim3(NX_WAVE), 0, as_stream(stream), static_cast<const int *>(plane_dev),
                       (long long)n, static_cast<const long long *>(hits_dev), off, static_cast<unsigned *>(bits_dev),
                       static_cast<long long *>(levels_dev));
    return check_launch("k_nxdn_slice");
}

extern "C" int iqa_nxdn_decode(const void *bits_dev, const void *classes_dev, int64_t K, void *info_dev, void *rec_dev, void *stream)
{
    if (const int rc = pl_check_lengths(0, K)) return rc;
    if (K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!bits_dev || !classes_dev || !info_dev || !rec_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_nxdn_decode, dim3(static_cast<unsigned>(K)), dim3(NX_WAVE), 0, as_stream(stream),
                       static_cast<const unsigned *>(bits_dev), static_cast<const unsigned char *>(classes_dev), (long long)K,
                       static_cast<unsigned *>(info_dev), static_cast<int *>(rec_dev));
    return check_launch("k_nxdn_decode");
}
