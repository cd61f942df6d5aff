// protocol.h -- what the kernels of the second pass's protocol layers share (ident.hip, flex.hip, dmr.hip, p25.hip, ysf.hip, nxdn.hip;
// DESIGN.md section 27), for gfx950: the bits of a word record, the sync word's levels, the Golay code over 0xC75, the workgroup minimum,
// the slicing of a four-level symbol against the levels of its sync word, the slice kernel of a whole frame behind its sync word,
// the K = 5, rate 1/2 convolutional code with its sixteen-lane Viterbi decoder, and the host checks of the entry points.
//
// Words and codes.  A record is u32 words with the first sent bit the MSB of word 0 (pl_bit).  A 24-symbol sync word is 48 bits,
// symbol 0 on top, a dibit 01 = +3, 11 = -3: pl_sync_positive names a symbol's sign, pl_sync_ups counts the +3 (the balance that
// turns the sums over the sync symbols into the DC and the outer level).  pl_golay is the systematic encoder of the (23,12) code
// over 0xC75 with an even parity bit, shortened to data_bits; pl_golay_distance holds a table of its codewords to the code's
// distance at compile time.
//
// Workgroup.  pl_block_min: the minimum over keys (distance << k | value) that every thread has put into LDS.
//
// Slicing.  A hit row begins (m, s): m where sync symbol 0 ends on the integrator plane of section 25, s the sign of its
// correlation (pl_hit).  An instant m + o[i] is read only where it lies in [0, n) (pl_read).  pl_dibit slices d, a symbol less
// the DC, against the outer level amp, both at the layer's common scale; pl_pack_dibits packs sixteen of them into a word.
// pl_slice_frame<Spec> is the slice kernel of P25, YSF and NXDN: a spec names the frame's size, its sync symbols' weights
// (pl_sync_positive's sign, or pl_sync_level where the word holds inner levels), the two linear forms that give A and Dc, their
// scale and a scrambler; DMR's two sync kinds and FLEX's bit convention keep their own kernels.
//
// The code.  pl_conv_branch is the K = 5, rate 1/2 code of YSF and NXDN, pl_viterbi16 its decoder (with or without erasures for
// punctured bits), pl_group_min16 the minimum over a trellis's lanes, pl_frame the rule for a frame slot past the last.
//
// Host.  pl_check_lengths and pl_copy_offsets are the prologue of the entry points: the limits of one stored stream and of one
// call, and the offset table o[i] = rint(i sps) that is passed by value to the kernels.
#pragma once

#include "common.h"

namespace iqa {

constexpr int64_t PL_MAX_N = 1LL << 30;       // samples of one stored stream: positions stay far inside int64, rows inside 2^31
constexpr int64_t PL_MAX_K = 1LL << 20;       // hits, frames or bursts of one call: at most 55 workgroups each inside the grid's 2^31
constexpr long long PL_V_MAX = 64LL * 65534;  // |v| of the integrator plane
constexpr unsigned PL_GOLAY_POLY = 0xC75u;
constexpr int PL_WAVE = 64;
constexpr int PL_GROUP = 16;   // lanes of a trellis of the K = 5 code: its states
constexpr int PL_FAR = 1000;   // the metric of a state that cannot be reached yet: above every real one (two a step, 360 for YSF's 180 steps)

// ---- words and codes ----------------------------------------------------------------------------------------------------------

// bit b of a record, the first sent bit the MSB of word 0
__device__ inline unsigned pl_bit(const unsigned *w, int b) { return (w[b >> 5] >> (31 - (b & 31))) & 1u; }

__host__ __device__ constexpr unsigned pl_popcount(unsigned x)
{
    unsigned c = 0;
    for (; x; x &= x - 1) ++c;
    return c;
}

__host__ __device__ constexpr unsigned pl_parity(unsigned x)
{
    x ^= x >> 16;
    x ^= x >> 8;
    x ^= x >> 4;
    x ^= x >> 2;
    x ^= x >> 1;
    return x & 1u;
}

// whether symbol i (0 .. 23) of a sync word is a positive level: the dibits 01 (+3) and 00 (+1) have a clear first bit
__host__ __device__ constexpr bool pl_sync_positive(unsigned long long word, int i) { return ((word >> (2 * (23 - i) + 1)) & 1ull) == 0; }

// the level of symbol i of a sync word of ``symbols`` dibits, symbol 0 on top: the dibits 01 +3, 00 +1, 10 -1, 11 -3
__host__ __device__ constexpr int pl_sync_level(unsigned long long word, int symbols, int i)
{
    const unsigned two = static_cast<unsigned>(word >> (2 * (symbols - 1 - i))) & 3u;
    return two == 1u ? 3 : two == 0u ? 1 : two == 2u ? -1 : -3;
}

// the +3 symbols of a sync word, or -1 where it holds an inner level (only 01 and 11 may occur)
constexpr int pl_sync_ups(unsigned long long word)
{
    int up = 0;
    for (int i = 0; i < 24; ++i) {
        if (((word >> (2 * (23 - i))) & 1ull) == 0) return -1;
        up += pl_sync_positive(word, i) ? 1 : 0;
    }
    return up;
}

// the codeword of a data_bits-bit value (at most 12): data << 12 | (data x^11 mod 0xC75) << 1 | even parity
__host__ __device__ constexpr unsigned pl_golay(unsigned data, int data_bits)
{
    unsigned r = data << 11;
    for (int i = data_bits + 10; i >= 11; --i)
        if ((r >> i) & 1u) r ^= PL_GOLAY_POLY << (i - 11);
    const unsigned cw = (data << 12) | ((r & 0x7FFu) << 1);
    return cw | pl_parity(cw);
}
static_assert(pl_golay(0x29, 8) == pl_golay(0x29, 12), "a shortened value has the codeword of the full code");

// The smallest weight of a nonzero codeword of a table (t.word(d), d < count), or 0 where the table is not linear.  Every word is
// held to the sum of the word of its lowest set bit and the word of the rest, so the table is linear, a difference of two
// codewords is a codeword, and the smallest nonzero weight is the smallest distance between two of them.
template <class Table>
constexpr unsigned pl_golay_distance(const Table &t, unsigned count)
{
    unsigned best = 32;
    for (unsigned d = 1; d < count; ++d) {
        if (t.word(d) != (t.word(d & (d - 1)) ^ t.word(d & (0u - d)))) return 0;
        const unsigned w = pl_popcount(t.word(d));
        if (w < best) best = w;
    }
    return t.word(0) == 0 ? best : 0;
}

// ---- workgroup ----------------------------------------------------------------------------------------------------------------

// the minimum of s_key[0 .. threads) over the workgroup (threads a power of two); every thread has written its entry
__device__ inline unsigned pl_block_min(unsigned *s_key, int tid, int threads)
{
    __syncthreads();
    for (int w = threads / 2; w >= 1; w >>= 1) {
        if (tid < w && s_key[tid + w] < s_key[tid]) s_key[tid] = s_key[tid + w];
        __syncthreads();
    }
    const unsigned key = s_key[0];
    __syncthreads();  // (the next round overwrites s_key only behind every read of it)
    return key;
}

// ---- slicing ------------------------------------------------------------------------------------------------------------------

struct PlHit {
    long long m, s;  // where sync symbol 0 ends; +-1
};
__device__ __forceinline__ PlHit pl_hit(const long long *row) { return {row[0], row[1] < 0 ? -1LL : 1LL}; }

// plane[at] where the instant lies in [0, n), else 0: nothing outside the plane is read
__device__ __forceinline__ int pl_read(const int *__restrict__ plane, long long n, long long at, bool &inside)
{
    inside = at >= 0 && at < n;
    return inside ? plane[at] : 0;
}

// the dibit of a symbol at d from the DC with the outer level amp: its first bit (d < 0), its second (3 |d| >= 2 amp)
__device__ __forceinline__ unsigned pl_dibit(long long d, long long amp)
{
    const long long mag = d < 0 ? -d : d;
    return (d < 0 ? 2u : 0u) | (3 * mag >= 2 * amp ? 1u : 0u);
}

// word ``lane`` of the dibits in s_two, sixteen to a word, the first the top two bits
__device__ __forceinline__ unsigned pl_pack_dibits(const unsigned char *s_two, int lane)
{
    unsigned word = 0;
    for (int k = 0; k < 16; ++k) word |= static_cast<unsigned>(s_two[16 * lane + k]) << (30 - 2 * k);
    return word;
}

// whether a spec's A and Dc are its SCALE times the outer level and the DC of the least squares fit of x_i to DC + L w_i over
// its sync symbols (w_i = weight(i), an outer symbol weighing OUTER): with N symbols, S1 = sum w_i, S2 = sum w_i^2 and
// det = N S2 - S1^2 the fit is DC = (S2 P - S1 Q) / det, L = (N Q - S1 P) / det
template <class Spec>
constexpr bool pl_slice_fits()
{
    long long s1 = 0, s2 = 0;
    for (int i = 0; i < Spec::SYNC_SYMBOLS; ++i) {
        s1 += Spec::weight(i);
        s2 += Spec::weight(i) * Spec::weight(i);
    }
    const long long det = Spec::SYNC_SYMBOLS * s2 - s1 * s1;
    return Spec::A_Q * det == Spec::OUTER * Spec::SYNC_SYMBOLS * Spec::SCALE && Spec::A_P * det == -Spec::OUTER * s1 * Spec::SCALE &&
           Spec::D_P * det == s2 * Spec::SCALE && Spec::D_Q * det == -s1 * Spec::SCALE;
}

// The body of a frame's slice kernel (k_p25_slice, k_ysf_slice, k_nxdn_slice), one wave per hit.  Spec names the frame: OFFSETS
// symbols in WORDS words; SYNC_SYMBOLS at its head with the weights weight(i); P = sum x_i and Q = sum weight(i) x_i over them
// give A = s (A_Q Q + A_P P) and Dc = D_P P + D_Q Q, both SCALE times the outer level and the DC; flip(i) is XORed onto the dibit
// of symbol i (0 but for a scrambler).  valid = 0 if m + o[0] < 0, else the number of i with m + o[i] < n: o[0] = 0 and o
// ascends, so a reach of 0 for a hit in front of the plane makes it a prefix count.  valid < SYNC_SYMBOLS: all bits 0,
// A = Dc = 0.  The lanes gather the instants in strided rounds, each checked against [0, n) before it is read; P, Q and valid
// are wave reductions; WORDS lanes pack the words from LDS.  bits: u32[WORDS] per hit, levels: A, Dc, valid.
template <class Spec>
__device__ __forceinline__ void pl_slice_frame(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                               const int (&o)[Spec::OFFSETS], unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    constexpr int ROUNDS = (Spec::OFFSETS + PL_WAVE - 1) / PL_WAVE;
    static_assert(2 * Spec::OFFSETS == 32 * Spec::WORDS && Spec::WORDS <= PL_WAVE, "sixteen symbols to a word, a word to a lane");
    static_assert(pl_slice_fits<Spec>(), "A and Dc are the least squares fit over the sync symbols at the scale");
    __shared__ unsigned char s_two[ROUNDS * PL_WAVE];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;
    const PlHit hit = pl_hit(hits + 2 * id);
    const long long reach = hit.m >= 0 ? n : 0;
    int y[ROUNDS];
    int count = 0;
#pragma unroll
    for (int p = 0; p < ROUNDS; ++p) {
        const int idx = p * PL_WAVE + lane;
        y[p] = 0;
        if (Spec::OFFSETS % PL_WAVE == 0 || idx < Spec::OFFSETS) {  // (only a last, partial round keeps the test)
            bool inside;
            y[p] = pl_read(plane, reach, hit.m + o[idx], inside);
            count += inside ? 1 : 0;
        }
    }
    long long sum = lane < Spec::SYNC_SYMBOLS ? y[0] : 0;
    long long weighted = lane < Spec::SYNC_SYMBOLS ? static_cast<long long>(Spec::weight(lane)) * y[0] : 0;
    sum = wave_sum(sum);
    weighted = wave_sum(weighted);
    const int valid = wave_sum(count);
    const bool read = valid >= Spec::SYNC_SYMBOLS;
    const long long amp = read ? hit.s * (Spec::A_Q * weighted + Spec::A_P * sum) : 0, dc = read ? Spec::D_P * sum + Spec::D_Q * weighted : 0;
#pragma unroll
    for (int p = 0; p < ROUNDS; ++p) {
        const int idx = p * PL_WAVE + lane;
        unsigned two = pl_dibit(hit.s * (Spec::SCALE * y[p] - dc), amp) ^ Spec::flip(idx);
        if (!read || idx >= valid) two = 0;
        s_two[idx] = static_cast<unsigned char>(two);
    }
    __syncthreads();
    if (lane < Spec::WORDS) bits_out[Spec::WORDS * id + lane] = pl_pack_dibits(s_two, lane);
    if (lane == 0) {
        long long *e = levels_out + 3 * id;
        e[0] = amp;
        e[1] = dc;
        e[2] = valid;
    }
}

// ---- the K = 5, rate 1/2 convolutional code ---------------------------------------------------------------------------------------

// the dibit g1 << 1 | g2 that the input d sends from the state d1 << 3 | d2 << 2 | d3 << 1 | d4: g1 = d ^ d3 ^ d4, g2 = d ^ d1 ^ d2 ^ d4
__host__ __device__ constexpr unsigned pl_conv_branch(unsigned state, unsigned d)
{
    const unsigned d1 = (state >> 3) & 1u, d2 = (state >> 2) & 1u, d3 = (state >> 1) & 1u, d4 = state & 1u;
    return (d ^ d3 ^ d4) << 1 | (d ^ d1 ^ d2 ^ d4);
}

// the ten sent bits of the input 1, 0, 0, 0, 0
constexpr unsigned pl_conv_impulse()
{
    unsigned state = 0, sent = 0;
    for (int t = 0; t < 5; ++t) {
        const unsigned d = t == 0 ? 1u : 0u;
        sent = sent << 2 | pl_conv_branch(state, d);
        state = d << 3 | state >> 1;
    }
    return sent;
}
static_assert(pl_conv_impulse() == 0x35Bu, "the input 1 0 0 0 0 sends 11 01 01 10 11");

// a frame past the last reads the last and writes nothing: (whether frame ``want`` is one of the ``count``, the frame to read)
struct PlFrame {
    bool mine;
    long long id;
};
__device__ __forceinline__ PlFrame pl_frame(long long want, long long count) { return {want < count, want < count ? want : count - 1}; }

// the minimum of key over the sixteen lanes of a trellis
__device__ __forceinline__ unsigned pl_group_min16(unsigned key)
{
#pragma unroll
    for (int w = PL_GROUP / 2; w >= 1; w >>= 1) {
        const unsigned other = static_cast<unsigned>(__shfl_xor(static_cast<int>(key), w, PL_GROUP));
        key = other < key ? other : key;
    }
    return key;
}

// The Viterbi decoder of one block of the code, on the Hamming distance, from state 0 (every other state starts PL_FAR away) to
// state 0; on equal metrics the predecessor with the smaller state index survives.  It runs in the sixteen lanes that the
// caller's lane belongs to: ``steps`` trellis steps (the same in all sixteen; 0: nothing is read), step t from ``fetch(t)``: the
// received dibit, and with ERASURES in the bits 3 .. 2 which of its two bits were sent (a punctured bit adds 0 to both branches;
// without ERASURES no mask is applied).  out: decoded bit t is bit 31 - t mod 32 of word t / 32 (the four tail bits are 0: the
// path ends in state 0), zeros behind.  Returns the metric of the surviving path.  Every lane of the wave calls it.
//
// A state to a lane, so a wave holds four trellises.  State t has the predecessors (t & 7) << 1 and (t & 7) << 1 | 1 on the input
// t >> 3: add-compare-select reads their metrics by a shuffle inside the sixteen; a step's survivor bit is bit t mod 32 of
// register t / 32 of its lane (NW registers for up to 32 NW steps), and the traceback reads the bit of the state it stands in by
// the same shuffle.  Lanes of one trellis share their step count and a step past it is predicated off (``live``), so every
// shuffle stands outside the conditions and no lane reads from one that is switched off.  The survivor words are indexed by the
// unrolled outer loops only, so nothing goes to scratch; the two 32-step loops stay loops (#pragma unroll 1): unrolled, YSF's
// two kernels took 211 and 188 registers.
template <int NW, bool ERASURES, class Fetch>
__device__ __forceinline__ int pl_viterbi16(int steps, Fetch fetch, unsigned (&out)[NW])
{
    const unsigned state = threadIdx.x & (PL_GROUP - 1), input = state >> 3;
    const int from = static_cast<int>((state & 7u) << 1);  // the smaller predecessor; the other is from + 1
    const unsigned sent0 = pl_conv_branch(from, input), sent1 = pl_conv_branch(from + 1, input);
    int metric = state == 0 ? 0 : PL_FAR;
    unsigned surv[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        unsigned word = 0;
#pragma unroll 1
        for (int b = 0; b < 32; ++b) {
            const int t = 32 * w + b;
            const bool live = t < steps;
            const unsigned got = live ? fetch(t) : 0u;
            const unsigned d0 = got ^ sent0, d1 = got ^ sent1;  // (the bits 1 .. 0; with ERASURES the mask in the bits 3 .. 2 picks from them)
            const int m0 = __shfl(metric, from, PL_GROUP) + static_cast<int>(pl_popcount(ERASURES ? d0 & (got >> 2) : d0));
            const int m1 = __shfl(metric, from + 1, PL_GROUP) + static_cast<int>(pl_popcount(ERASURES ? d1 & (got >> 2) : d1));
            const bool second = m1 < m0;  // (equal: the smaller state index survives)
            metric = live ? (second ? m1 : m0) : metric;
            word |= (live && second ? 1u : 0u) << b;
        }
        surv[w] = word;
    }
    const int total = __shfl(metric, 0, PL_GROUP);
    unsigned at = 0;  // the state the path stands in behind step t: the same in all sixteen lanes
#pragma unroll
    for (int w = NW - 1; w >= 0; --w) {
        unsigned word = 0;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const bool live = 32 * w + b < steps;
            const unsigned bit = (static_cast<unsigned>(__shfl(static_cast<int>(surv[w]), static_cast<int>(at), PL_GROUP)) >> b) & 1u;
            word |= (live ? at >> 3 : 0u) << (31 - b);
            at = live ? ((at & 7u) << 1 | bit) : at;
        }
        out[w] = word;
    }
    return steps > 0 ? total : 0;
}

// ---- host side of the entry points --------------------------------------------------------------------------------------------

// The lengths of a call: n samples of the plane and K items (``count`` the letter of the argument); 0 for the one that an entry
// point does not take.
inline int pl_check_lengths(int64_t n, int64_t K, char count = 'K')
{
    if (n < 0 || K < 0) return fail_inval("negative length");
    if (n > PL_MAX_N) return fail_inval("n must not exceed 2^30");
    if (K > PL_MAX_K) {
        set_error("invalid argument: %c must not exceed 2^20", count);
        return IQA_EINVAL;
    }
    return IQA_OK;
}

// dst = the table ``name`` of N offsets with o[0] at index ``lead``: o[0] = 0, strictly ascending, no step above the longest
// symbol plus the one sample that rounding adds.
inline int pl_copy_offsets(const int32_t *offsets, int N, int lead, const char *name, int *dst)
{
    if (!offsets) return fail_inval("NULL offsets");
    if (offsets[lead] != 0) {
        set_error("invalid argument: %s[%d] (o[0]) must be 0", name, lead);
        return IQA_EINVAL;
    }
    for (int i = 0; i < N; ++i) {
        const char *must = nullptr;
        if (i && offsets[i] <= offsets[i - 1]) must = "ascend";
        else if (i && offsets[i] - offsets[i - 1] > IQA_IDENT_MAX_SPS + 1) must = "not step by more than IQA_IDENT_MAX_SPS + 1";
        if (must) {
            set_error("invalid argument: %s must %s", name, must);
            return IQA_EINVAL;
        }
        dst[i] = offsets[i];
    }
    return IQA_OK;
}

}  // namespace iqa
