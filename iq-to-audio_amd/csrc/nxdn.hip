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
// k_nxdn_slice is one wave per hit: its lanes gather the 192 instants in three strided rounds, each checked against [0, n) before
// it is read; P, Q and valid are wave reductions; 12 lanes pack the words from LDS.  The decoder (n_viterbi) is ysf.hip's
// layout with an erasure mask: one trellis in sixteen lanes, a state to a lane, add-compare-select reading the two
// predecessors' metrics by a shuffle inside the sixteen, a step's survivor bit bit t mod 32 of register t / 32 of its lane, the
// traceback reading the bit of the state it stands in by the same shuffle.  k_nxdn_decode is a wave to a frame: the lanes
// 0 .. 15 run the SACCH or the CAC, 16 .. 31 and 32 .. 47 the two FACCH1s, 48 .. 63 nothing (0 steps).  The mask is the same in
// the whole wave, so the wave takes one of three sizes of the decoder: six survivor words with a CAC, three with a FACCH1, two
// for a SACCH alone.  Every shuffle stands outside the conditions on lanes, and no lane leaves before the barrier.  LDS holds
// only the frame's words, written before the one barrier and read after it.  Plain C++ stores, no inline assembly, no atomics,
// no mutable statics.
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
constexpr long long NX_SCALE = 370;
constexpr int NX_GROUP = 16;  // lanes of a trellis: its states
constexpr int NX_FAR = 1000;  // the metric of a state that cannot be reached yet: above every real one (300 at the most)
constexpr int NX_SCRAMBLED = NX_OFFSETS - NX_SYNC_SYMBOLS;  // 182 scrambler bits

static_assert(NX_ROUNDS * NX_WAVE == NX_OFFSETS && 2 * NX_OFFSETS == 32 * NX_WORDS, "192 symbols: three rounds of a wave, 12 words");
static_assert(NX_INFO == 2 + 3 + 3 + 6 && NX_REC == 4, "two words to the SACCH, three to a FACCH1, six to the CAC");

struct NxdnOffsets {
    int o[NX_OFFSETS];
};

// the level of sync symbol i: the dibits 01 +3, 00 +1, 10 -1, 11 -3
__host__ __device__ constexpr int nx_sync_level(int i)
{
    const unsigned two = (NX_SYNC >> (2 * (NX_SYNC_SYMBOLS - 1 - i))) & 3u;
    return two == 1u ? 3 : two == 0u ? 1 : two == 2u ? -1 : -3;
}

constexpr int nx_sync_sum(int power)
{
    int sum = 0;
    for (int i = 0; i < NX_SYNC_SYMBOLS; ++i) {
        const int s = nx_sync_level(i);
        sum += power == 2 ? s * s : power == 1 ? s : s < 0 ? -s : s;
    }
    return sum;
}
static_assert(nx_sync_sum(1) == 0 && nx_sync_sum(2) == 74, "sum s_i = 0 and sum s_i^2 = 74: the fit is DC = P / 10, L = s Q / 74");
static_assert(NX_SCALE == 37 * NX_SYNC_SYMBOLS && NX_SCALE * 3 == 15 * 74, "at the scale 370: Dc = 37 P, A = s 15 Q");
static_assert(15LL * nx_sync_sum(0) * PL_V_MAX * 3 < (1LL << 50) && NX_SCALE * PL_V_MAX * 2 * 3 < (1LL << 50), "15 Q, 370 x - Dc and 3 |d| stay far inside int64");

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

// ---- the convolutional code, its puncturing and its interleave -------------------------------------------------------------------------

// the dibit g1 << 1 | g2 that the input d sends from the state d1 << 3 | d2 << 2 | d3 << 1 | d4
__host__ __device__ constexpr unsigned nx_branch(unsigned state, unsigned d)
{
    const unsigned d1 = (state >> 3) & 1u, d2 = (state >> 2) & 1u, d3 = (state >> 1) & 1u, d4 = state & 1u;
    return (d ^ d3 ^ d4) << 1 | (d ^ d1 ^ d2 ^ d4);
}

// the ten sent bits of the input 1, 0, 0, 0, 0
constexpr unsigned nx_impulse()
{
    unsigned state = 0, sent = 0;
    for (int t = 0; t < 5; ++t) {
        const unsigned d = t == 0 ? 1u : 0u;
        sent = sent << 2 | nx_branch(state, d);
        state = d << 3 | state >> 1;
    }
    return sent;
}
static_assert(nx_impulse() == 0x35Bu, "the input 1 0 0 0 0 sends 11 01 01 10 11");

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

// The decoder of one block in the sixteen lanes that the caller's lane belongs to: ``steps`` trellis steps (the same in all
// sixteen; 0: nothing is read), step t from ``fetch(t)`` (nx_fetch's form).  out: decoded bit t is bit 31 - t mod 32 of word
// t / 32 (the four tail bits are 0: the path ends in state 0), zeros behind.  Returns the metric of the surviving path.  Every
// lane of the wave calls it.
template <int NW, class Fetch>
__device__ __forceinline__ int n_viterbi(int steps, Fetch fetch, unsigned (&out)[NW])
{
    const unsigned state = threadIdx.x & (NX_GROUP - 1), input = state >> 3;
    const int from = static_cast<int>((state & 7u) << 1);  // the smaller predecessor; the other is from + 1
    const unsigned sent0 = nx_branch(from, input), sent1 = nx_branch(from + 1, input);
    int metric = state == 0 ? 0 : NX_FAR;
    unsigned surv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        unsigned word = 0;
#pragma unroll 1
        for (int b = 0; b < 32; ++b) {
            const int t = 32 * w + b;
            const bool live = t < steps;
            const unsigned got = live ? fetch(t) : 0u;
            const unsigned rx = got & 3u, keep = got >> 2;  // (a punctured bit adds 0 to both branches)
            const int m0 = __shfl(metric, from, NX_GROUP) + static_cast<int>(pl_popcount((rx ^ sent0) & keep));
            const int m1 = __shfl(metric, from + 1, NX_GROUP) + static_cast<int>(pl_popcount((rx ^ sent1) & keep));
            const bool second = m1 < m0;  // (equal: the smaller state index survives)
            metric = live ? (second ? m1 : m0) : metric;
            word |= (live && second ? 1u : 0u) << b;
        }
        surv[w] = word;
    }
    const int total = __shfl(metric, 0, NX_GROUP);
    unsigned at = 0;  // the state the path stands in behind step t: the same in all sixteen lanes
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) {
        unsigned word = 0;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const bool live = 32 * w + b < steps;
            const unsigned bit = (static_cast<unsigned>(__shfl(static_cast<int>(surv[w]), static_cast<int>(at), NX_GROUP)) >> b) & 1u;
            word |= (live ? at >> 3 : 0u) << (31 - b);
            at = live ? ((at & 7u) << 1 | bit) : at;
        }
        out[w] = word;
    }
    return steps > 0 ? total : 0;
}

__global__ __launch_bounds__(NX_WAVE) void k_nxdn_slice(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                                        NxdnOffsets off, unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    __shared__ unsigned char s_two[NX_OFFSETS];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;
    const PlHit hit = pl_hit(hits + 2 * id);
    const long long reach = hit.m >= 0 ? n : 0;  // o[0] = 0 and o ascends: a hit in front of the plane reads nothing, one inside it a prefix
    // the gather: every instant is checked against [0, n) before it is read
    int y[NX_ROUNDS];
    int count = 0;
#pragma unroll
    for (int p = 0; p < NX_ROUNDS; ++p) {
        bool inside;
        y[p] = pl_read(plane, reach, hit.m + off.o[p * NX_WAVE + lane], inside);
        count += inside ? 1 : 0;
    }
    long long sum = lane < NX_SYNC_SYMBOLS ? y[0] : 0;
    long long weighted = lane < NX_SYNC_SYMBOLS ? static_cast<long long>(nx_sync_level(lane)) * y[0] : 0;
    sum = wave_sum(sum);
    weighted = wave_sum(weighted);
    const int valid = wave_sum(count);
    const bool read = valid >= NX_SYNC_SYMBOLS;
    const long long amp = read ? hit.s * 15 * weighted : 0, dc = read ? 37 * sum : 0;
#pragma unroll
    for (int p = 0; p < NX_ROUNDS; ++p) {
        const int idx = p * NX_WAVE + lane;
        unsigned two = pl_dibit(hit.s * (NX_SCALE * y[p] - dc), amp);
        two ^= ((NX_SCRAMBLE.sym[idx >> 5] >> (idx & 31)) & 1u) << 1;  // (the scrambler inverts the symbol's sign)
        if (!read || idx >= valid) two = 0;
        s_two[idx] = static_cast<unsigned char>(two);
    }
    __syncthreads();
    if (lane < NX_WORDS) bits_out[NX_WORDS * id + lane] = pl_pack_dibits(s_two, lane);
    if (lane == 0) {
        long long *e = levels_out + 3 * id;
        e[0] = amp;
        e[1] = dc;
        e[2] = valid;
    }
}

// a frame to a wave: the lanes 0 .. 15 take the SACCH or the CAC, 16 .. 31 FACCH1-a, 32 .. 47 FACCH1-b, 48 .. 63 nothing
__global__ __launch_bounds__(NX_WAVE) void k_nxdn_decode(const unsigned *__restrict__ bits, const unsigned char *__restrict__ classes, long long count,
                                                         unsigned *__restrict__ info_out, int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[NX_GROUP];
    const int lane = threadIdx.x, group = lane / NX_GROUP, sub = lane % NX_GROUP;
    const long long want = blockIdx.x;
    const bool mine = want < count;
    const long long id = mine ? want : count - 1;  // (a frame past the last reads the last and writes nothing)
    if (lane < NX_GROUP) s_w[lane] = lane < NX_WORDS ? bits[NX_WORDS * id + lane] : 0u;
    __syncthreads();
    const unsigned *w = s_w;
    const int given = classes[id];
    const int cls = (given > 15 || ((given & IQA_NXDN_CAC) != 0 && given != IQA_NXDN_CAC)) ? 0 : given;  // (the same in the whole wave)
    const bool cac = cls == IQA_NXDN_CAC;
    unsigned out[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    int metric;
    if (cac) {
        metric = n_viterbi<6>(group == 0 ? NxCac::STEPS : 0, [w](int t) { return nx_fetch<NxCac>(w, NX_CAC_FIRST, t); }, out);
    } else {
        const int steps = group == 0 ? (cls & IQA_NXDN_SACCH ? NxSacch::STEPS : 0)
                                     : group == 1 ? (cls & IQA_NXDN_FACCH1_A ? NxFacch1::STEPS : 0)
                                                  : group == 2 ? (cls & IQA_NXDN_FACCH1_B ? NxFacch1::STEPS : 0) : 0;
        const int first = group == 2 ? NX_FACCH1_B_FIRST : NX_FACCH1_A_FIRST;
        if (cls & (IQA_NXDN_FACCH1_A | IQA_NXDN_FACCH1_B)) {
            unsigned three[3];
            metric = n_viterbi<3>(steps, [=](int t) {
                const unsigned sacch = nx_fetch<NxSacch>(w, NX_SACCH_FIRST, t < NxSacch::STEPS ? t : 0);
                const unsigned facch = nx_fetch<NxFacch1>(w, first, t);
                return group == 0 ? sacch : facch;
            }, three);
            out[0] = three[0], out[1] = three[1], out[2] = three[2];
        } else {
            unsigned two[2];
            metric = n_viterbi<2>(steps, [w](int t) { return nx_fetch<NxSacch>(w, NX_SACCH_FIRST, t); }, two);
            out[0] = two[0], out[1] = two[1];
        }
    }
    const int metric_0 = __shfl(metric, 0), metric_a = __shfl(metric, NX_GROUP), metric_b = __shfl(metric, 2 * NX_GROUP);
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
