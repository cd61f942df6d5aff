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
// k_ysf_slice is one wave per hit: its lanes gather the 480 instants in eight strided rounds, each checked against [0, n)
// before it is read; P, Q and valid are wave reductions; 30 lanes pack the words from LDS.  The decoder (y_viterbi) holds one
// trellis in sixteen lanes, a state to a lane, so a wave holds four: add-compare-select reads the two predecessors' metrics by
// a shuffle inside the sixteen, a step's survivor bit is bit t mod 32 of register t / 32 of its lane (six registers for 180
// steps), and the traceback reads the bit of the state it stands in by the same shuffle.  Lanes of one trellis share their step
// count, and every shuffle stands outside the conditions, so no lane reads from one that is switched off.  k_ysf_fich is a wave
// for four frames, k_ysf_decode a wave for the two blocks of two frames; a frame past K reads frame K - 1 and writes nothing,
// and no lane leaves before the barrier.  The Golay search is sixteen lanes by 256 codewords, the minimum over (distance, data)
// by shuffles.  LDS holds only the frames' words, written before the one barrier and read after it.  Plain C++ stores, no inline
// assembly, no atomics, no mutable statics.
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
constexpr long long Y_SCALE = 584;
constexpr int Y_GROUP = 16;   // lanes of a trellis: its states
constexpr int Y_FAR = 1000;   // the metric of a state that cannot be reached yet: above every real one (360 at the most)
constexpr int Y_FICH_STEPS = 100, Y_DCH_STEPS = 180, Y_DCH2_STEPS = 100;
constexpr int Y_FICH_FIRST = 40, Y_PAYLOAD_FIRST = 240, Y_PAYLOAD_BLOCK = 144;

static_assert(2 * Y_OFFSETS == 32 * Y_WORDS && Y_ROUNDS == 8, "480 symbols: eight rounds of a wave, 30 words");
static_assert(Y_INFO == 12 && 32 * 6 >= Y_DCH_STEPS && 32 * 4 >= Y_FICH_STEPS, "six words to a DCH block, four to the FICH");

struct YsfOffsets {
    int o[Y_OFFSETS];
};

// the level of sync symbol i: the dibits 01 +3, 00 +1, 10 -1, 11 -3
__host__ __device__ constexpr int y_sync_level(int i)
{
    const unsigned two = static_cast<unsigned>(Y_SYNC >> (2 * (Y_SYNC_SYMBOLS - 1 - i))) & 3u;
    return two == 1u ? 3 : two == 0u ? 1 : two == 2u ? -1 : -3;
}

constexpr int y_sync_sum(bool squares)
{
    int sum = 0;
    for (int i = 0; i < Y_SYNC_SYMBOLS; ++i) sum += squares ? y_sync_level(i) * y_sync_level(i) : y_sync_level(i);
    return sum;
}
static_assert(y_sync_sum(false) == 12 && y_sync_sum(true) == 124, "sum s_i = 12 and sum s_i^2 = 124: Dc = 31 P - 3 Q, A = s (15 Q - 9 P)");
static_assert(20 * 124 - 12 * 12 == 4 * Y_SCALE && 124 == 4 * 31 && 12 == 4 * 3 && 20 * 3 == 4 * 15 && 12 * 3 == 4 * 9, "the fit, less its factor 4");
static_assert((15 * 124 + 9 * 20) * PL_V_MAX * 3 < (1LL << 50) && Y_SCALE * PL_V_MAX * 2 * 3 < (1LL << 50), "15 Q - 9 P, 584 y - Dc and 3 |d| stay far inside int64");

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

// the dibit g1 << 1 | g2 that the input d sends from the state d1 << 3 | d2 << 2 | d3 << 1 | d4
__host__ __device__ constexpr unsigned y_branch(unsigned state, unsigned d)
{
    const unsigned d1 = (state >> 3) & 1u, d2 = (state >> 2) & 1u, d3 = (state >> 1) & 1u, d4 = state & 1u;
    return (d ^ d3 ^ d4) << 1 | (d ^ d1 ^ d2 ^ d4);
}

// the ten sent bits of the input 1, 0, 0, 0, 0
constexpr unsigned y_impulse()
{
    unsigned state = 0, sent = 0;
    for (int t = 0; t < 5; ++t) {
        const unsigned d = t == 0 ? 1u : 0u;
        sent = sent << 2 | y_branch(state, d);
        state = d << 3 | state >> 1;
    }
    return sent;
}
static_assert(y_impulse() == 0x35Bu, "the input 1 0 0 0 0 sends 11 01 01 10 11");

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

// The decoder of one block in the sixteen lanes that the caller's lane belongs to: ``steps`` dibits (the same in all sixteen;
// 0: nothing is read), dibit t from ``fetch(t)``.  out: decoded bit t is bit 31 - t mod 32 of word t / 32 (the four tail bits
// are 0: the path ends in state 0), zeros behind.  Returns the metric of the surviving path.  Every lane of the wave calls it.
template <int NW, class Fetch>
__device__ __forceinline__ int y_viterbi(int steps, Fetch fetch, unsigned (&out)[NW])
{
    const unsigned state = threadIdx.x & (Y_GROUP - 1), input = state >> 3;
    const int from = static_cast<int>((state & 7u) << 1);  // the smaller predecessor; the other is from + 1
    const unsigned sent0 = y_branch(from, input), sent1 = y_branch(from + 1, input);
    int metric = state == 0 ? 0 : Y_FAR;
    unsigned surv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        unsigned word = 0;
#pragma unroll 1
        for (int b = 0; b < 32; ++b) {
            const int t = 32 * w + b;
            const bool live = t < steps;
            const unsigned rx = live ? fetch(t) : 0u;
            const int m0 = __shfl(metric, from, Y_GROUP) + static_cast<int>(pl_popcount(rx ^ sent0));
            const int m1 = __shfl(metric, from + 1, Y_GROUP) + static_cast<int>(pl_popcount(rx ^ sent1));
            const bool second = m1 < m0;  // (equal: the smaller state index survives)
            metric = live ? (second ? m1 : m0) : metric;
            word |= (live && second ? 1u : 0u) << b;
        }
        surv[w] = word;
    }
    const int total = __shfl(metric, 0, Y_GROUP);
    unsigned at = 0;  // the state the path stands in behind step t: the same in all sixteen lanes
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) {
        unsigned word = 0;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const bool live = 32 * w + b < steps;
            const unsigned bit = (static_cast<unsigned>(__shfl(static_cast<int>(surv[w]), static_cast<int>(at), Y_GROUP)) >> b) & 1u;
            word |= (live ? at >> 3 : 0u) << (31 - b);
            at = live ? ((at & 7u) << 1 | bit) : at;
        }
        out[w] = word;
    }
    return steps > 0 ? total : 0;
}

// the minimum of key over the sixteen lanes of a trellis
__device__ __forceinline__ unsigned y_group_min(unsigned key)
{
#pragma unroll
    for (int w = Y_GROUP / 2; w >= 1; w >>= 1) {
        const unsigned other = static_cast<unsigned>(__shfl_xor(static_cast<int>(key), w, Y_GROUP));
        key = other < key ? other : key;
    }
    return key;
}

// the dibit at the frame bits b, b + 1 (b even) of a frame's words
__device__ __forceinline__ unsigned y_dibit(const unsigned *w, int b) { return (w[b >> 5] >> (30 - (b & 31))) & 3u; }

__global__ __launch_bounds__(Y_WAVE) void k_ysf_slice(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                                      YsfOffsets off, unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    __shared__ unsigned char s_two[Y_ROUNDS * Y_WAVE];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;
    const PlHit hit = pl_hit(hits + 2 * id);
    const long long reach = hit.m >= 0 ? n : 0;  // o[0] = 0 and o ascends: a hit in front of the plane reads nothing, one inside it a prefix
    // the gather: every instant is checked against [0, n) before it is read
    int y[Y_ROUNDS];
    int count = 0;
#pragma unroll
    for (int p = 0; p < Y_ROUNDS; ++p) {
        const int idx = p * Y_WAVE + lane;
        y[p] = 0;
        if (idx < Y_OFFSETS) {
            bool inside;
            y[p] = pl_read(plane, reach, hit.m + off.o[idx], inside);
            count += inside ? 1 : 0;
        }
    }
    long long sum = lane < Y_SYNC_SYMBOLS ? y[0] : 0;
    long long weighted = lane < Y_SYNC_SYMBOLS ? static_cast<long long>(y_sync_level(lane)) * y[0] : 0;
    sum = wave_sum(sum);
    weighted = wave_sum(weighted);
    const int valid = wave_sum(count);
    const bool read = valid >= Y_SYNC_SYMBOLS;
    const long long amp = read ? hit.s * (15 * weighted - 9 * sum) : 0, dc = read ? 31 * sum - 3 * weighted : 0;
#pragma unroll
    for (int p = 0; p < Y_ROUNDS; ++p) {
        const int idx = p * Y_WAVE + lane;
        unsigned two = pl_dibit(hit.s * (Y_SCALE * y[p] - dc), amp);
        if (!read || idx >= valid) two = 0;
        s_two[idx] = static_cast<unsigned char>(two);
    }
    __syncthreads();
    if (lane < Y_WORDS) bits_out[Y_WORDS * id + lane] = pl_pack_dibits(s_two, lane);
    if (lane == 0) {
        long long *e = levels_out + 3 * id;
        e[0] = amp;
        e[1] = dc;
        e[2] = valid;
    }
}

// four frames to a wave, one to every sixteen lanes
__global__ __launch_bounds__(Y_WAVE) void k_ysf_fich(const unsigned *__restrict__ bits, long long count, unsigned *__restrict__ fich_out,
                                                     int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[Y_WAVE / Y_GROUP][Y_WORDS + 2];
    const int lane = threadIdx.x, group = lane / Y_GROUP, sub = lane % Y_GROUP;
    const long long want = 4LL * blockIdx.x + group;
    const bool mine = want < count;
    const long long id = mine ? want : count - 1;  // (a frame past the last reads the last and writes nothing)
    s_w[group][sub] = bits[Y_WORDS * id + sub];
    s_w[group][sub + Y_GROUP] = sub + Y_GROUP < Y_WORDS ? bits[Y_WORDS * id + sub + Y_GROUP] : 0u;
    __syncthreads();
    const unsigned *w = s_w[group];
    unsigned out[4];
    const int metric = y_viterbi<4>(Y_FICH_STEPS, [w](int t) { return y_dibit(w, Y_FICH_FIRST + 2 * y_deinterleave(t, 5)); }, out);
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
        const unsigned key = y_group_min(best);
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
    __shared__ unsigned s_w[2][2 * Y_GROUP];
    const int lane = threadIdx.x, slot = lane / (2 * Y_GROUP), block = (lane / Y_GROUP) & 1, sub = lane % Y_GROUP;
    const long long want = 2LL * blockIdx.x + slot;
    const bool mine = want < count;
    const long long id = mine ? want : count - 1;  // (a frame past the last reads the last and writes nothing)
    const int at = lane % (2 * Y_GROUP);
    s_w[slot][at] = at < Y_WORDS ? bits[Y_WORDS * id + at] : 0u;
    __syncthreads();
    const unsigned *w = s_w[slot];
    const int given = classes[id];
    const int cls = given <= 3 ? given : 0;
    const int steps = cls == 1 || (cls == 2 && block == 0) ? Y_DCH_STEPS : cls == 3 && block == 0 ? Y_DCH2_STEPS : 0;
    const int rows = cls == 3 ? 5 : 9, part = cls == 3 ? 40 : 72, first = Y_PAYLOAD_FIRST + 72 * block;
    unsigned out[6];
    const int metric = y_viterbi<6>(steps, [=](int t) {
        const int b = 2 * y_deinterleave(t, rows);  // the bit of the data channel; it lies in payload block b / part
        return y_dibit(w, first + Y_PAYLOAD_BLOCK * (b / part) + b % part);
    }, out);
    const int metric_a = __shfl(metric, 0, 2 * Y_GROUP), metric_b = __shfl(metric, Y_GROUP, 2 * Y_GROUP);
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
