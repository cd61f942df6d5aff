// flex.hip -- the words of FLEX frames behind their first sync word (--find-flex), for gfx950: the levels
// and the frame information word of every kept sync-1 hit, and the 2- or 4-level slicing, phase split, block de-interleave and
// BCH(31,21) check of a frame's eleven data blocks at five timing shifts.
//
// Specification (plane the integrator plane v of section 25, n samples; a hit (m, s): m where bit 0 of the marker ends, s the
// sign of its correlation; o16[i] = rint(i sps), i = -16 .. 95, at index 16 + i; p_i the marker 0xA6C6AAAA as +-1, MSB first):
//   k_flex_frames, per hit:
//     x_i = s plane[m + o16[i]], i = 0 .. 31; Sigma = sum x_i, A = sum p_i x_i                     (int64; valid iff all inside)
//     FIW bit j = (32 s plane[m + o16[64 + j]] - Sigma > 0), j = 0 .. 31, the first sent bit 0 of W   (status 3 where outside)
//   k_flex_words, per frame (m, s, Sigma, A), shift index e = 0 .. 4 (d = (e - 2) step), block b = 0 .. 10, with per = 256 u:
//     symbol q = b per + r, r = k u + pair, at the instant m + off[q] + d: y = s plane[instant], dd = 32 y - Sigma
//     bit_a = (dd > 0), bit_b = (3 |dd| < 2 A)                                                     (bit_b at 4 levels only)
//     pair 0 feeds phase A (bit_a) and B (bit_b), pair 1 phase C (bit_a) and D (bit_b)
//     bit k of a block and phase is bit k / 8 of word 8 b + k % 8
//   a word W: rev32(W) is a section 12 codeword (the upper 31 bits modulo g = 0x769, even parity over 32): status 0 clean, 1
//   one bit restored, 2 refused (fixed = raw), 3 an instant outside [0, n) (raw = fixed = 0), 4 a phase that the mode does
//   not send (raw = fixed = 0).
//
// k_flex_words is a workgroup per (frame, shift, block): 256 threads gather the block's 256 u plane values (one strided read
// each, u = 1 or 2), slice them to a byte of four phase bits and two validity bits in LDS; 32 threads (8 words x 4 phases)
// then assemble and check their words from LDS.  The hit's head, the checked read, the parity and the host prologue are
// protocol.h's; the bit convention is FLEX's own.  Plain C++ stores, no inline assembly, no atomics.
#include "protocol.h"

namespace iqa {

constexpr int FX_THREADS = 256;
constexpr int FX_FRAME_THREADS = 64;
constexpr int FX_HEAD = IQA_FLEX_HEADER_OFFSETS;  // 112: o16[-16] .. o16[95]
constexpr int FX_LEAD = 16;                       // o16[i] sits at index 16 + i
constexpr int FX_BLOCKS = IQA_FLEX_BLOCKS;        // 11
constexpr int FX_SHIFTS = IQA_FLEX_SHIFTS;        // 5
constexpr int FX_PHASES = IQA_FLEX_PHASES;        // 4
constexpr int FX_WORDS = IQA_FLEX_WORDS;          // 88 words of a phase
constexpr int FX_SYMBOLS = IQA_FLEX_SYMBOLS;      // 2816 data symbols of a frame at u = 1
constexpr unsigned FX_POLY = 0x769u;              // x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
constexpr unsigned FX_MARKER = 0xA6C6AAAAu;

static_assert(FX_THREADS * 11 == FX_SYMBOLS && FX_BLOCKS * 8 == FX_WORDS, "eleven blocks of 256 bits, eight words each");
static_assert(32 * PL_V_MAX * 33 < (1LL << 40), "32 y - Sigma and 3 |dd| stay far inside int64");

struct FlexHeader {
    int o[FX_HEAD];
};

__host__ __device__ constexpr unsigned fx_rev32(unsigned x)
{
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    return (x >> 16) | (x << 16);
}

// remainder of the upper 31 bits of a codeword (first sent bit as MSB) modulo g (10 bits)
__host__ __device__ constexpr unsigned fx_syndrome(unsigned cw)
{
    unsigned r = cw >> 1;
    for (int i = 30; i >= 10; --i)
        if ((r >> i) & 1u) r ^= FX_POLY << (i - 10);
    return r & 0x3FFu;
}

constexpr bool fx_singles_distinct()
{
    for (int a = 1; a < 32; ++a)
        for (int b = a + 1; b < 32; ++b)
            if (fx_syndrome(1u << a) == fx_syndrome(1u << b)) return false;
    for (int a = 1; a < 32; ++a)
        if (fx_syndrome(1u << a) == 0) return false;
    return true;
}

// 0x1BA84B3E is 0x7CD215D8 (section 12's sync word, a codeword of g) with its first sent bit as bit 0
static_assert(fx_rev32(0x1BA84B3Eu) == 0x7CD215D8u && fx_syndrome(fx_rev32(0x1BA84B3Eu)) == 0 && pl_parity(0x1BA84B3Eu) == 0,
              "rev32 of a known codeword has a zero syndrome and even parity");
static_assert(fx_singles_distinct(), "the 31 single-bit syndromes are distinct and not zero");

// section 12's rule on a word whose first sent bit is bit 0: the fixed word; status 0, 1 or 2
__host__ __device__ constexpr unsigned fx_correct(unsigned raw, unsigned char &status)
{
    const unsigned cw = fx_rev32(raw), syn = fx_syndrome(cw), odd = pl_parity(cw);
    status = 2;
    if (syn == 0) {
        status = odd ? 1 : 0;
        return fx_rev32(cw ^ odd);  // (an odd word with a clean syndrome: the parity bit itself)
    }
    if (odd)
        for (int pos = 1; pos < 32; ++pos)
            if (fx_syndrome(1u << pos) == syn) {
                status = 1;
                return fx_rev32(cw ^ (1u << pos));
            }
    return raw;
}

__global__ __launch_bounds__(FX_FRAME_THREADS) void k_flex_frames(const int *__restrict__ plane, long long n,
                                                                 const long long *__restrict__ hits, long long K, FlexHeader hd,
                                                                 long long *__restrict__ out)
{
    const long long id = static_cast<long long>(blockIdx.x) * FX_FRAME_THREADS + threadIdx.x;
    if (id >= K) return;
    const PlHit hit = pl_hit(hits + 2 * id);
    long long sigma = 0, amp = 0, valid = 1;
    for (int i = 0; i < 32; ++i) {
        bool inside;
        const long long x = hit.s * pl_read(plane, n, hit.m + hd.o[FX_LEAD + i], inside);
        if (!inside) {
            valid = 0;
            break;
        }
        sigma += x;
        amp += ((FX_MARKER >> (31 - i)) & 1u) ? x : -x;
    }
    unsigned raw = 0, fixed = 0;
    unsigned char status = 3;
    if (!valid) {
        sigma = amp = 0;
    } else {
        bool inside = true;
        for (int j = 0; j < 32 && inside; ++j)
            if (32 * hit.s * pl_read(plane, n, hit.m + hd.o[FX_LEAD + 64 + j], inside) - sigma > 0) raw |= 1u << j;
        if (inside)
            fixed = fx_correct(raw, status);
        else
            raw = 0;
    }
    long long *e = out + 6 * id;
    e[0] = sigma;
    e[1] = amp;
    e[2] = raw;
    e[3] = fixed;
    e[4] = status;
    e[5] = valid;
}

__global__ __launch_bounds__(FX_THREADS) void k_flex_words(const int *__restrict__ plane, long long n, const long long *__restrict__ frames,
                                                           int levels, int u, int step, const int *__restrict__ offs,
                                                           unsigned *__restrict__ fixed_out, unsigned *__restrict__ raw_out,
                                                           unsigned char *__restrict__ status_out)
{
    // per bit k of the block: bits 0 .. 3 the bits of phases A .. D, bit 4 + pair set where the pair's instant lies outside
    __shared__ unsigned char s_bits[FX_THREADS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x % FX_BLOCKS, e = (blockIdx.x / FX_BLOCKS) % FX_SHIFTS;
    const long long f = blockIdx.x / (FX_BLOCKS * FX_SHIFTS);
    const PlHit hit = pl_hit(frames + 4 * f);
    const long long sigma = frames[4 * f + 2], amp = frames[4 * f + 3];
    const long long d = static_cast<long long>(e - 2) * step;
    unsigned bits = 0;
    for (int pair = 0; pair < u; ++pair) {
        const int q = b * FX_THREADS * u + tid * u + pair;  // (< 2816 u: inside offs)
        bool inside;
        const long long dd = 32 * hit.s * pl_read(plane, n, hit.m + offs[q] + d, inside) - sigma;
        if (!inside) {
            bits |= 16u << pair;
            continue;
        }
        if (dd > 0) bits |= 1u << (2 * pair);
        if (levels == 4 && 3 * (dd < 0 ? -dd : dd) < 2 * amp) bits |= 2u << (2 * pair);
    }
    s_bits[tid] = static_cast<unsigned char>(bits);
    __syncthreads();
    if (tid >= 8 * FX_PHASES) return;
    const int ph = tid >> 3, col = tid & 7, pair = ph >> 1;
    const bool active = ((ph & 1) == 0 || levels == 4) && (pair == 0 || u == 2);
    unsigned raw = 0, fixed = 0;
    unsigned char status = 4;
    if (active) {
        unsigned outside = 0;
        for (int j = 0; j < 32; ++j) {
            const unsigned v = s_bits[8 * j + col];
            outside |= (v >> (4 + pair)) & 1u;
            raw |= ((v >> ph) & 1u) << j;
        }
        if (outside) {
            raw = 0;
            status = 3;
        } else {
            fixed = fx_correct(raw, status);
        }
    }
    const long long at = ((f * FX_SHIFTS + e) * FX_PHASES + ph) * FX_WORDS + 8 * b + col;
    fixed_out[at] = fixed;
    raw_out[at] = raw;
    status_out[at] = status;
}

}  // namespace iqa

using namespace iqa;

static_assert(PL_MAX_K * FX_SHIFTS * FX_BLOCKS < (1LL << 31), "55 workgroups to a frame stay inside the grid");

extern "C" int iqa_flex_frames(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K,
                               const int32_t offsets16[IQA_FLEX_HEADER_OFFSETS], void *out_dev, void *stream)
{
    FlexHeader hd;
    if (const int rc = pl_check_lengths(n, K)) return rc;
    if (const int rc = pl_copy_offsets(offsets16, FX_HEAD, FX_LEAD, "offsets16", hd.o)) return rc;
    if (n == 0 || K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!plane_dev || !hits_dev || !out_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_flex_frames, grid1d(K, FX_FRAME_THREADS), dim3(FX_FRAME_THREADS), 0, as_stream(stream),
                       static_cast<const int *>(plane_dev), (long long)n, static_cast<const long long *>(hits_dev), (long long)K, hd,
                       static_cast<long long *>(out_dev));
    return check_launch("k_flex_frames");
}

extern "C" int iqa_flex_words(const void *plane_dev, int64_t n, const void *frames_dev, int64_t F, int32_t levels, int32_t u,
                              int32_t step, const void *offsets_dev, void *fixed_dev, void *raw_dev, void *status_dev, void *stream)
{
    if (const int rc = pl_check_lengths(n, F, 'F')) return rc;
    if (levels != 2 && levels != 4) return fail_inval("levels must be 2 or 4");
    if (u != 1 && u != 2) return fail_inval("u must be 1 or 2");
    if (step < 1 || step > IQA_FLEX_MAX_STEP) return fail_inval("step must be 1 .. IQA_FLEX_MAX_STEP");
    if (n == 0 || F == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!plane_dev || !frames_dev || !offsets_dev || !fixed_dev || !raw_dev || !status_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_flex_words, dim3(static_cast<unsigned>(F * FX_SHIFTS * FX_BLOCKS)), dim3(FX_THREADS), 0, as_stream(stream),
                       static_cast<const int *>(plane_dev), (long long)n, static_cast<const long long *>(frames_dev), (int)levels, (int)u,
                       (int)step, static_cast<const int *>(offsets_dev), static_cast<unsigned *>(fixed_dev),
                       static_cast<unsigned *>(raw_dev), static_cast<unsigned char *>(status_dev));
    return check_launch("k_flex_words");
}
