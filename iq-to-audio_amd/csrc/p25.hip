// p25.hip -- the frames of P25 phase 1 channels behind their frame sync (--find-p25), for gfx950: the
// levels and the 1728 sliced bits of every kept sync hit, the network identifier (NID) of every sliced frame, and the link
// control or the trunking blocks behind it.
//
// Specification (plane the integrator plane v of section 25 at 4800 symbols/s, n samples; a hit (m, s): m where sync symbol 0
// ends, s the sign of its correlation, a negative hit being the same word with the spectrum inverted; o[i] = rint(i sps),
// i = 0 .. 863; sgn_i the sign of sync symbol i; data dibit q is frame symbol q + q / 35, the symbols i mod 36 = 35 being status
// symbols; data bit b is bit b mod 2 of data dibit b / 2):
//   k_p25_slice, per hit:
//     valid = 0 if m + o[0] < 0, else the number of i with m + o[i] < n (a prefix); valid < 24: all bits 0, A = Dc = 0
//     x_i = v[m + o[i]], i = 0 .. 23; P = sum x_i, Q = sum sgn_i x_i; A = s (12 Q + P), Dc = 12 P + Q   (int64; the sync word
//     holds eleven +3 and thirteen -3, so A is 286 times the outer level and Dc 286 times the DC)
//     symbol i < valid: d = s (286 v[m + o[i]] - Dc); its first bit (d < 0), its second (3 |d| >= 2 A); i >= valid: 0, 0
//     bits: u32[54], symbol i the frame bits 2 i, 2 i + 1, the first sent bit the MSB of word 0; levels: A, Dc, valid
//   k_p25_nid, per frame: the 64 data bits 48 .. 111; the first 63 against the 65 536 codewords data x^47 + (data x^47 mod g) of
//     BCH(63,16,23), g the product of the minimal polynomials of alpha^1 .. alpha^22 over GF(64) / x^6 + x + 1; the minimum over
//     distance << 16 | data; status 0 clean, 1 corrected (distance 1 .. 11), 2 refused (the raw top 16 bits kept); parity_ok:
//     the 64 bits have even weight
//   k_p25_decode, per frame and DUID:
//     0xF (class 2): data bits 112 + 24 w .. + 23, w = 0 .. 11, Golay(24,12,8): data << 12 | (data x^11 mod 0xC75) << 1 | even
//     parity; the nearest of the 4096 codewords at a distance of 3 or less, else the word is refused and its raw top 12 bits kept
//     0x5 (class 1): data bits 400 + 184 g + 10 k .. + 9, g = 0 .. 5, k = 0 .. 3, Hamming(10,6,3): d0 .. d5 p0 .. p3, the parity
//     parts of the data columns 1110 1101 1011 0111 0011 1100; a syndrome that is one of the ten columns flips that bit, the
//     five others leave the word alone (unmatched)
//     0x7 (class 3): blocks b = 0 .. 2 of 98 data dibits from data dibit 56 + 98 b on, de-interleaved, 49 pairs through the
//     4-state trellis (state = the previous input dibit, start 0, 48 information dibits and a flush dibit 0), Viterbi on the
//     Hamming distance of the four bits, the smaller predecessor on equal metric, the path that ends in state 0
//     any other DUID (class 0): zeros
//   info: u32[9]: classes 1, 2 the 144 bits in words 0 .. 4; class 3 the 96 bits of block b in words 3 b .. 3 b + 2
//   rec: int32[8] = class, then (corrected words, refused or unmatched words, bits changed) or the three block metrics; 0s
//
// k_p25_slice is protocol.h's pl_slice_frame on P25Slice, one wave per hit: fourteen strided rounds, 54 lanes pack the words.
// k_p25_nid and k_p25_decode are a workgroup of 256 per frame: 256 codewords of the BCH code to a thread (T_hi[t] ^ T_lo[j]: the
// code is linear), 16 of the Golay code, with a minimum over (distance, data) through LDS; a thread per Hamming word; a thread
// per trellis block with its survivors in LDS.  The sync word's signs, the Golay encoder, the minimum and the host prologue are
// protocol.h's too.  Plain C++ stores, no inline assembly, no atomics, no mutable statics.
#include "protocol.h"

namespace iqa {

constexpr int P5_WAVE = 64;
constexpr int P5_THREADS = 256;
constexpr int P5_OFFSETS = IQA_P25_OFFSETS;  // 864: o[0] .. o[863], one LDU
constexpr int P5_WORDS = IQA_P25_WORDS;      // 54 words of 32 bits
constexpr int P5_ROUNDS = (P5_OFFSETS + P5_WAVE - 1) / P5_WAVE;  // 14
constexpr int P5_INFO = IQA_P25_INFO;        // 9
constexpr int P5_REC = IQA_P25_RECORD;       // 8
constexpr int P5_SYNC_SYMBOLS = 24;
constexpr unsigned long long P5_SYNC = 0x5575F5FF77FFull;

struct P25Offsets {
    int o[P5_OFFSETS];
};

// protocol.h's slicer on the signs of the all-outer sync word: A = s (12 Q + P), Dc = 12 P + Q at the scale 286
struct P25Slice {
    static constexpr int OFFSETS = P5_OFFSETS, WORDS = P5_WORDS, SYNC_SYMBOLS = P5_SYNC_SYMBOLS, OUTER = 1;
    static constexpr long long SCALE = 286, A_Q = 12, A_P = 1, D_P = 12, D_Q = 1;
    __host__ __device__ static constexpr int weight(int i) { return pl_sync_positive(P5_SYNC, i) ? 1 : -1; }
    __device__ static constexpr unsigned flip(int) { return 0u; }
};

static_assert(2 * P5_OFFSETS == 32 * P5_WORDS && P5_ROUNDS == 14, "864 symbols: fourteen rounds of a wave, 54 words");
static_assert(P25Slice::SCALE * PL_V_MAX * 2 * P5_SYNC_SYMBOLS * 3 < (1LL << 50), "286 y - Dc and 3 |d| stay far inside int64");
static_assert(pl_sync_ups(P5_SYNC) == 11, "the sync word holds eleven +3 and thirteen -3: 12 Q + P = 286 s L and 12 P + Q = 286 DC");

// ---- BCH(63,16,23) over GF(64) / x^6 + x + 1 ------------------------------------------------------------------------------------

struct P5Gf {
    unsigned char exp[126], log[64];
};

constexpr P5Gf p5_gf()
{
    P5Gf t{};
    unsigned x = 1;
    for (int i = 0; i < 63; ++i) {
        t.exp[i] = static_cast<unsigned char>(x);
        t.log[x] = static_cast<unsigned char>(i);
        x <<= 1;
        if (x & 0x40u) x ^= 0x43u;
    }
    for (int i = 63; i < 126; ++i) t.exp[i] = t.exp[i - 63];
    return t;
}

// the product of (x + alpha^e) over the conjugates of alpha^1 .. alpha^22; bit k the coefficient of x^k; 0 where a coefficient
// falls outside GF(2)
constexpr unsigned long long p5_bch_generator()
{
    const P5Gf gf = p5_gf();
    bool root[63] = {};
    for (int r = 1; r <= 22; ++r)
        for (int e = r, k = 0; k < 6; ++k, e = (2 * e) % 63) root[e] = true;
    unsigned char g[64] = {1};
    int deg = 0;
    for (int e = 0; e < 63; ++e) {
        if (!root[e]) continue;
        for (int k = deg + 1; k >= 0; --k) {
            const unsigned low = k > 0 ? g[k - 1] : 0u;
            const unsigned scaled = (k <= deg && g[k]) ? gf.exp[gf.log[g[k]] + e] : 0u;
            g[k] = static_cast<unsigned char>(low ^ scaled);
        }
        ++deg;
    }
    unsigned long long out = 0;
    for (int k = 0; k <= deg; ++k) {
        if (g[k] > 1) return 0;
        out |= static_cast<unsigned long long>(g[k]) << k;
    }
    return out;
}

constexpr unsigned long long P5_BCH_G = p5_bch_generator();
static_assert(P5_BCH_G == 06331141367235453ull, "the generator of degree 47, as the standard prints it in octal");

// value mod g, value of degree at most 63
constexpr unsigned long long p5_bch_rem(unsigned long long value)
{
    for (int i = 63; i >= 47; --i)
        if ((value >> i) & 1ull) value ^= P5_BCH_G << (i - 47);
    return value;
}
static_assert(p5_bch_rem((1ull << 63) | 1ull) == 0, "g divides x^63 + 1");

// the 63-bit codeword of a 16-bit value
constexpr unsigned long long p5_bch(unsigned data)
{
    const unsigned long long top = static_cast<unsigned long long>(data) << 47;
    return top | p5_bch_rem(top);
}

struct P5Bch {
    unsigned long long hi[256], lo[256];
};

constexpr P5Bch p5_bch_tables()
{
    P5Bch t{};
    for (unsigned d = 0; d < 256; ++d) {
        t.hi[d] = p5_bch(d << 8);
        t.lo[d] = p5_bch(d);
    }
    return t;
}

constexpr P5Bch P5_BCH_HOST = p5_bch_tables();
static_assert((P5_BCH_HOST.hi[0x29] ^ P5_BCH_HOST.lo[0x35]) == p5_bch(0x2935), "the code is linear: a codeword is T_hi ^ T_lo");
__device__ const P5Bch P5_BCH = p5_bch_tables();

// ---- Golay(24,12,8) ---------------------------------------------------------------------------------------------------------------

// the codeword of the 12-bit value d is hi[d >> 4] ^ lo[d & 15]
struct P5Golay {
    unsigned hi[256], lo[16];
    constexpr unsigned word(unsigned d) const { return hi[d >> 4] ^ lo[d & 15u]; }
};

constexpr P5Golay p5_golay_tables()
{
    P5Golay t{};
    for (unsigned d = 0; d < 256; ++d) t.hi[d] = pl_golay(d << 4, 12);
    for (unsigned d = 0; d < 16; ++d) t.lo[d] = pl_golay(d, 12);
    return t;
}

constexpr P5Golay P5_GOLAY_HOST = p5_golay_tables();
static_assert((P5_GOLAY_HOST.hi[0xAB] ^ P5_GOLAY_HOST.lo[0xC]) == pl_golay(0xABC, 12), "the code is linear: a codeword is G_hi ^ G_lo");
static_assert(pl_golay_distance(P5_GOLAY_HOST, 4096) == 8, "the 4096 codewords lie 8 apart at the least: a word within 3 of one is within 3 of no other");
__device__ const P5Golay P5_GOLAY = p5_golay_tables();

// ---- Hamming(10,6,3) --------------------------------------------------------------------------------------------------------------

// the column of H of word bit j (0 .. 5 data, 6 .. 9 parity) as p0 p1 p2 p3, p0 the top bit
__host__ __device__ constexpr unsigned p5_hamming_column(int j)
{
    constexpr unsigned packed = 0xEDB73Cu;  // 1110 1101 1011 0111 0011 1100
    return j < 6 ? (packed >> (4 * (5 - j))) & 15u : 8u >> (j - 6);
}

// the word bit whose column is syn, or -1 where no column is
__host__ __device__ constexpr int p5_hamming_position(unsigned syn)
{
    for (int j = 0; j < 10; ++j)
        if (p5_hamming_column(j) == syn) return j;
    return -1;
}

constexpr int p5_hamming_named()
{
    int named = 0;
    for (unsigned syn = 1; syn < 16; ++syn) named += p5_hamming_position(syn) >= 0 ? 1 : 0;
    return named;
}
static_assert(p5_hamming_named() == 10, "ten distinct nonzero columns: five syndromes name no bit");

// ---- the trellis ------------------------------------------------------------------------------------------------------------------

// the four channel bits (first dibit << 2 | second) of the branch from state i on input j: the pair of point[i][j]
constexpr unsigned long long p5_branches()
{
    constexpr unsigned pair[16] = {0x2, 0xA, 0x7, 0xF, 0xE, 0x6, 0xB, 0x3, 0xD, 0x5, 0x8, 0x0, 0x1, 0x9, 0x4, 0xC};
    constexpr unsigned point[16] = {0, 15, 12, 3, 4, 11, 8, 7, 13, 2, 1, 14, 9, 6, 5, 10};
    unsigned long long out = 0;
    for (int k = 0; k < 16; ++k) out |= static_cast<unsigned long long>(pair[point[k]]) << (4 * k);
    return out;
}
constexpr unsigned long long P5_BRANCHES = p5_branches();
__host__ __device__ constexpr unsigned p5_branch(int state, int input) { return static_cast<unsigned>(P5_BRANCHES >> (4 * (4 * state + input))) & 15u; }

// the dibit of a block (0 .. 97, as sent) that is dibit n of the coded stream
__host__ __device__ constexpr int p5_deinterleave(int n)
{
    if (n < 26) return 8 * (n >> 1) + (n & 1);
    const int k = n - 26, r = 1 + k / 24;
    return 8 * ((k % 24) >> 1) + 2 * r + (n & 1);
}

constexpr bool p5_permutes()
{
    bool seen[98] = {};
    for (int n = 0; n < 98; ++n) {
        const int at = p5_deinterleave(n);
        if (at < 0 || at >= 98 || seen[at]) return false;
        seen[at] = true;
    }
    return true;
}
static_assert(p5_permutes(), "the de-interleaver is a permutation of 0 .. 97");

constexpr int P5_TRELLIS_STEPS = 49;
constexpr int P5_FAR = 1000;  // the metric of a state that cannot be reached yet: above every real one (196 at the most)

// ---- the bits of a frame ------------------------------------------------------------------------------------------------------------

// data bit b of a frame's record: the status symbols skipped
__device__ inline unsigned p5_data_bit(const unsigned *w, int b)
{
    const int q = b >> 1;
    return pl_bit(w, 2 * (q + q / 35) + (b & 1));
}
static_assert(2 * (679 + 679 / 35) + 1 < 32 * P5_WORDS, "data bit 1359, the last that a decoder reads, lies inside the record");

__global__ __launch_bounds__(P5_WAVE) void k_p25_slice(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                                       P25Offsets off, unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    pl_slice_frame<P25Slice>(plane, n, hits, off.o, bits_out, levels_out);
}

__global__ __launch_bounds__(P5_THREADS) void k_p25_nid(const unsigned *__restrict__ bits, int *__restrict__ nid_out)
{
    __shared__ unsigned s_w[4];
    __shared__ unsigned s_key[P5_THREADS];
    const int tid = threadIdx.x;
    const long long id = blockIdx.x;
    if (tid < 4) s_w[tid] = bits[P5_WORDS * id + tid];  // data bits 48 .. 111 are frame bits 48 .. 113
    __syncthreads();
    unsigned long long word = 0;
    for (int b = 0; b < 64; ++b) word = word << 1 | p5_data_bit(s_w, 48 + b);
    const unsigned long long r = word >> 1, mine = r ^ P5_BCH.hi[tid];
    unsigned best = 0xFFFFFFFFu;
    for (int j = 0; j < 256; ++j) {
        const unsigned key = static_cast<unsigned>(__popcll(mine ^ P5_BCH.lo[j])) << 16 | static_cast<unsigned>(tid) << 8 | static_cast<unsigned>(j);
        best = key < best ? key : best;
    }
    s_key[tid] = best;
    const unsigned key = pl_block_min(s_key, tid, P5_THREADS);
    if (tid == 0) {
        const int distance = static_cast<int>(key >> 16);
        const int status = distance == 0 ? 0 : distance <= 11 ? 1 : 2;
        int *e = nid_out + 4 * id;
        e[0] = status;
        e[1] = distance;
        e[2] = status == 2 ? static_cast<int>(r >> 47) : static_cast<int>(key & 0xFFFFu);
        e[3] = (__popcll(word) & 1) == 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(P5_THREADS) void k_p25_decode(const unsigned *__restrict__ bits, const unsigned char *__restrict__ duids,
                                                           unsigned *__restrict__ info_out, int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[P5_WORDS];
    __shared__ unsigned s_key[P5_THREADS];
    __shared__ unsigned char s_bits[32 * P5_INFO];
    __shared__ unsigned char s_flag[24];
    __shared__ unsigned char s_surv[3][P5_TRELLIS_STEPS];
    __shared__ int s_metric[3];
    const int tid = threadIdx.x;
    const long long id = blockIdx.x;
    const int duid = duids[id] & 15;  // (block-uniform)
    if (tid < P5_WORDS) s_w[tid] = bits[P5_WORDS * id + tid];
    for (int k = tid; k < 32 * P5_INFO; k += P5_THREADS) s_bits[k] = 0;
    __syncthreads();
    int cls = 0, a = 0, b = 0, c = 0;
    if (duid == 0xF) {  // twelve Golay words
        cls = 2;
        for (int w = 0; w < 12; ++w) {
            unsigned word = 0;
            for (int k = 0; k < 24; ++k) word = word << 1 | p5_data_bit(s_w, 112 + 24 * w + k);
            const unsigned mine = word ^ P5_GOLAY.hi[tid];
            unsigned best = 0xFFFFFFFFu;
            for (int j = 0; j < 16; ++j) {
                const unsigned key = pl_popcount(mine ^ P5_GOLAY.lo[j]) << 12 | static_cast<unsigned>(tid) << 4 | static_cast<unsigned>(j);
                best = key < best ? key : best;
            }
            s_key[tid] = best;
            const unsigned key = pl_block_min(s_key, tid, P5_THREADS);
            const int distance = static_cast<int>(key >> 12);
            unsigned data = key & 0xFFFu;
            if (distance > 3) {
                ++b;
                data = word >> 12;
            } else if (distance > 0) {
                ++a;
                c += distance;
            }
            if (tid < 12) s_bits[12 * w + tid] = static_cast<unsigned char>((data >> (11 - tid)) & 1u);
        }
    } else if (duid == 0x5) {  // 24 Hamming words
        cls = 1;
        if (tid < 24) {
            const int first = 400 + 184 * (tid >> 2) + 10 * (tid & 3);
            unsigned word = 0, syn = 0;
            for (int j = 0; j < 10; ++j) {
                const unsigned bit = p5_data_bit(s_w, first + j);
                word |= bit << j;
                if (bit) syn ^= p5_hamming_column(j);
            }
            const int pos = syn ? p5_hamming_position(syn) : -1;
            if (pos >= 0) word ^= 1u << pos;
            s_flag[tid] = static_cast<unsigned char>(syn == 0 ? 0 : pos >= 0 ? 1 : 2);
            for (int j = 0; j < 6; ++j) s_bits[6 * tid + j] = static_cast<unsigned char>((word >> j) & 1u);
        }
        __syncthreads();
        for (int j = 0; j < 24; ++j) {
            a += s_flag[j] == 1 ? 1 : 0;
            b += s_flag[j] == 2 ? 1 : 0;
        }
        c = a;
    } else if (duid == 0x7) {  // three trellis blocks
        cls = 3;
        if (tid < 3) {
            const int first = 2 * (56 + 98 * tid);  // the block's first data bit
            int m0 = 0, m1 = P5_FAR, m2 = P5_FAR, m3 = P5_FAR;
            for (int t = 0; t < P5_TRELLIS_STEPS; ++t) {
                const int d0 = first + 2 * p5_deinterleave(2 * t), d1 = first + 2 * p5_deinterleave(2 * t + 1);
                const unsigned rx = p5_data_bit(s_w, d0) << 3 | p5_data_bit(s_w, d0 + 1) << 2 | p5_data_bit(s_w, d1) << 1 | p5_data_bit(s_w, d1 + 1);
                int next[4];
                unsigned surv = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int best = m0 + static_cast<int>(pl_popcount(rx ^ p5_branch(0, j))), arg = 0;
                    const int c1 = m1 + static_cast<int>(pl_popcount(rx ^ p5_branch(1, j)));
                    const int c2 = m2 + static_cast<int>(pl_popcount(rx ^ p5_branch(2, j)));
                    const int c3 = m3 + static_cast<int>(pl_popcount(rx ^ p5_branch(3, j)));
                    if (c1 < best) best = c1, arg = 1;
                    if (c2 < best) best = c2, arg = 2;
                    if (c3 < best) best = c3, arg = 3;
                    next[j] = best;
                    surv |= static_cast<unsigned>(arg) << (2 * j);
                }
                m0 = next[0], m1 = next[1], m2 = next[2], m3 = next[3];
                s_surv[tid][t] = static_cast<unsigned char>(surv);
            }
            int state = 0;  // the flush dibit
            for (int t = P5_TRELLIS_STEPS - 1; t >= 0; --t) {
                if (t < P5_TRELLIS_STEPS - 1) {
                    s_bits[96 * tid + 2 * t] = static_cast<unsigned char>(state >> 1);
                    s_bits[96 * tid + 2 * t + 1] = static_cast<unsigned char>(state & 1);
                }
                state = (s_surv[tid][t] >> (2 * state)) & 3;
            }
            s_metric[tid] = m0;
        }
        __syncthreads();
        a = s_metric[0], b = s_metric[1], c = s_metric[2];
    }
    __syncthreads();
    if (tid < P5_INFO) {
        unsigned word = 0;
        for (int k = 0; k < 32; ++k) word |= static_cast<unsigned>(s_bits[32 * tid + k]) << (31 - k);
        info_out[P5_INFO * id + tid] = word;
    }
    if (tid == 0) {
        int *e = rec_out + P5_REC * id;
        e[0] = cls;
        e[1] = a;
        e[2] = b;
        e[3] = c;
        e[4] = e[5] = e[6] = e[7] = 0;
    }
}

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_p25_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_P25_OFFSETS],
                             void *bits_dev, void *levels_dev, void *stream)
{
    P25Offsets off;
    if (const int rc = pl_check_lengths(n, K)) return rc;
    if (const int rc = pl_copy_offsets(offsets, P5_OFFSETS, 0, "offsets", off.o)) return rc;
    if (n == 0 || K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!plane_dev || !hits_dev || !bits_dev || !levels_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_p25_slice, dim3(static_cast<unsigned>(K)), dim3(P5_WAVE), 0, as_stream(stream), static_cast<const int *>(plane_dev),
                       (long long)n, static_cast<const long long *>(hits_dev), off, static_cast<unsigned *>(bits_dev),
                       static_cast<long long *>(levels_dev));
    return check_launch("k_p25_slice");
}

extern "C" int iqa_p25_nid(const void *bits_dev, int64_t K, void *nid_dev, void *stream)
{
    if (const int rc = pl_check_lengths(0, K)) return rc;
    if (K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!bits_dev || !nid_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_p25_nid, dim3(static_cast<unsigned>(K)), dim3(P5_THREADS), 0, as_stream(stream), static_cast<const unsigned *>(bits_dev),
                       static_cast<int *>(nid_dev));
    return check_launch("k_p25_nid");
}

extern "C" int iqa_p25_decode(const void *bits_dev, const void *duids_dev, int64_t K, void *info_dev, void *rec_dev, void *stream)
{
    if (const int rc = pl_check_lengths(0, K)) return rc;
    if (K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!bits_dev || !duids_dev || !info_dev || !rec_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_p25_decode, dim3(static_cast<unsigned>(K)), dim3(P5_THREADS), 0, as_stream(stream),
                       static_cast<const unsigned *>(bits_dev), static_cast<const unsigned char *>(duids_dev), static_cast<unsigned *>(info_dev),
                       static_cast<int *>(rec_dev));
    return check_launch("k_p25_decode");
}
