// ais.hip -- AIS (9600 bit/s GMSK, HDLC) beside the NFM demodulator, for gfx950.
//
// Specification (fs the channel rate, theta the discriminator output, all indices absolute, everything zero in front of
// the stream; sps = fs / 9600, L = rint(sps), W = 3 L - 1, h[k] the int16 pulse taps of dsp_plan.plan_ais, 0 <= h <= 256):
//   t[n]    = rint(theta[n] 4096)                                   (int32, half-even; integers from here on)
//   S[n]    = sum_{k<W} h[k] t[n-k]                                 (int32: 12 868 . sum |h| < 2^31)
//   phase p, symbol i: instant n_i = W - 1 + rint((8 i + p) (sps / 8)) (one float64 product, one rint);  v_p[i] = S[n_i]
//   position s >= 24 of phase p: level sum = v[s-24] + .. + v[s-9] (int64); m_i = (16 v_i > sum); b_i = (m_i == m_{i-1});
//   s opens a candidate iff b[s-8 .. s-1] = 0111 1110 and b[s-22 .. s-9] alternate; from s bytes LSB first, a zero after
//   five ones dropped, a sixth one ends the walk (a closing flag iff the next bit is 0 and 6 bits of the current byte are
//   collected), more than 128 bytes abort; kept iff >= 11 bytes and the CRC-16/X.25 of all but the last two equals them.
//
// k_ais_filter has k_afsk_correlate's layout (afsk.hip): a workgroup owns 2048 consecutive samples, quantises them and the
// H = W - 1 rounded up to 8 values in front of them into LDS, the image padded by one word per 8 (lanes are 8 samples apart,
// so a fixed tap of consecutive lanes is 9 words apart), and every thread makes 8 consecutive outputs from a register
// window.  Tap 0 reads the thread's own 8 values; taps 1 .. W - 1 go in groups of 8, zero-padded to H, each group reading
// the 8 values in front of the window: every staged value is used and nothing in front of the image is touched.  Taps
// are read from LDS at a wave-uniform address, four per read.  One accumulator per output, 24-bit multiply-add.
// k_ais_symbols and k_ais_frames run once per run and read global memory directly.
#include "common.h"

namespace iqa {

constexpr int AI_THREADS = 256;
constexpr int AI_RUN = 8;                       // consecutive outputs of a thread of k_ais_filter, and its tap group
constexpr int AI_TILE = AI_THREADS * AI_RUN;    // 2048
constexpr int AI_MAX_TAPS = 3 * IQA_AIS_MAX_SPS - 1;  // 299
constexpr float AI_THETA_SCALE = 4096.0f;
constexpr int AI_MIN_FRAME = 11, AI_MAX_FRAME = IQA_AIS_SLOT_BYTES;
constexpr int AI_LEVEL_FIRST = 24, AI_LEVEL_COUNT = 16;  // the level of s: v[s-24 .. s-9]
constexpr unsigned AI_CRC_POLY = 0x8408u;

__host__ __device__ constexpr int ai_pad(int i) { return i + (i >> 3); }
__host__ __device__ constexpr int ai_front(int W) { return (W - 1 + AI_RUN - 1) / AI_RUN * AI_RUN; }  // H
__host__ __device__ constexpr int ai_lds_words(int W) { return ai_front(W) + ai_pad(ai_front(W) + AI_TILE) + 1; }

// acc += a b for |a|, |b| < 2^23 (see af_mad24 in afsk.hip: written out so that the compiler keeps one instruction per
// multiply-add).
__device__ __forceinline__ void ai_mad24(int &acc, int a, int b)
{
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

struct AisFilterArgs {
    const float *theta;   // [n]
    const int *hist;      // [W - 1]: t in front of theta[0]; NULL = zeros
    const short *taps;    // [W]
    int *t_out;           // [n] or NULL
    int *s_out;           // [n]
    long long n;
    int W;
};

__global__ __launch_bounds__(AI_THREADS) void k_ais_filter(AisFilterArgs g)
{
    extern __shared__ int4 s_ai[];
    const int tid = threadIdx.x, W = g.W, H = ai_front(W);
    int *s_taps = reinterpret_cast<int *>(s_ai);  // [H]: s_taps[j] = h[1 + j], zero for 1 + j >= W
    int *s_t = s_taps + H;                        // s_t[ai_pad(i)] = t at block index A - H + i, i = 0 .. H + AI_TILE - 1
    const long long A = static_cast<long long>(blockIdx.x) * AI_TILE;
    for (int j = tid; j < H; j += AI_THREADS) s_taps[j] = (1 + j < W) ? g.taps[1 + j] : 0;
    for (int i = tid; i < H + AI_TILE; i += AI_THREADS) {
        const long long a = A - H + i;
        int v = 0;
        if (a < 0) {
            if (g.hist && a >= -(W - 1)) v = g.hist[(W - 1) + a];  // (the index is 0 .. W-2; further back only zero taps reach)
        } else if (a < g.n) {
            v = __float2int_rn(g.theta[a] * AI_THETA_SCALE);
            if (i >= H && g.t_out) g.t_out[a] = v;
        }
        s_t[ai_pad(i)] = v;
    }
    __syncthreads();
    const long long a0 = A + tid * AI_RUN;
    if (a0 >= g.n) return;
    const int first = H + tid * AI_RUN;  // LDS index (unpadded) of this thread's first output
    // w[j] = t at LDS index first - kb - 8 + j, j = 0 .. 15: output r, tap 1 + kb + kk reads index first + r - 1 - kb - kk = w[7 + r - kk]
    int w[2 * AI_RUN], acc[AI_RUN];
    const int h0 = g.taps[0];
#pragma unroll
    for (int j = 0; j < AI_RUN; ++j) {
        w[AI_RUN + j] = s_t[ai_pad(first + j)];
        acc[j] = 0;
        ai_mad24(acc[j], h0, w[AI_RUN + j]);
    }
    for (int kb = 0; kb < H; kb += AI_RUN) {
#pragma unroll
        for (int j = 0; j < AI_RUN; ++j) w[j] = s_t[ai_pad(first - kb - AI_RUN + j)];  // (first - kb - 8 >= H - (H - 8) - 8 = 0)
        const int4 ta = s_ai[kb >> 2], tb = s_ai[(kb >> 2) + 1];
        const int tp[AI_RUN] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
#pragma unroll
        for (int kk = 0; kk < AI_RUN; ++kk)
#pragma unroll
            for (int r = 0; r < AI_RUN; ++r) ai_mad24(acc[r], tp[kk], w[AI_RUN - 1 + r - kk]);
#pragma unroll
        for (int j = 0; j < AI_RUN; ++j) w[AI_RUN + j] = w[j];
    }
    if (a0 + AI_RUN <= g.n && (reinterpret_cast<uintptr_t>(g.s_out) & 15u) == 0) {  // (a0 is a multiple of 8: 32 bytes)
        int4 *dst = reinterpret_cast<int4 *>(g.s_out + a0);
        dst[0] = make_int4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_int4(acc[4], acc[5], acc[6], acc[7]);
        return;
    }
#pragma unroll
    for (int r = 0; r < AI_RUN; ++r)
        if (a0 + r < g.n) g.s_out[a0 + r] = acc[r];
}

__device__ __forceinline__ long long ai_instant(int W, double step, long long i, int p)
{
    return W - 1 + static_cast<long long>(rint(static_cast<double>(8 * i + p) * step));
}

struct AisSymbolArgs {
    const int *s;      // [n]
    int *v;            // [8][nsym]
    long long n, nsym;
    double step;       // sps / 8
    int W;
};

__global__ __launch_bounds__(AI_THREADS) void k_ais_symbols(AisSymbolArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * AI_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (i >= g.nsym) return;
    const long long at = ai_instant(g.W, g.step, i, p);
    g.v[p * g.nsym + i] = at < g.n ? g.s[at] : 0;  // (a symbol whose instant lies beyond the stream does not exist: never read)
}

struct AisFrameArgs {
    const int *v;               // [8][nsym]
    long long nsym;
    long long count_of[IQA_AIS_PHASES];  // symbols of phase p that exist
    long long *list;            // [capacity][4]: phase, s, start instant, nbytes
    unsigned char *slots;       // [capacity][IQA_AIS_SLOT_BYTES]
    long long capacity;
    unsigned long long *counts; // [2]: kept frames; closed candidates of >= 11 bytes
    double step;
    int W;
};

__device__ __forceinline__ unsigned ai_crc_byte(unsigned reg, unsigned byte)
{
    reg ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) reg = (reg & 1u) ? (reg >> 1) ^ AI_CRC_POLY : reg >> 1;
    return reg;
}

__device__ __forceinline__ unsigned ai_level(int v, long long total) { return 16LL * v > total ? 1u : 0u; }

// The walk from s under the level sum ``total``: -1 for an abort / an over-long frame / the end of the stream, else the
// byte count.  crc_ok: the CRC-16/X.25 of all but the last two bytes equals them (low byte first); three registers one
// byte apart, as af_walk keeps them.  out != NULL also stores the bytes.
__device__ int ai_walk(const int *__restrict__ v, long long s, long long nb, long long total, unsigned char *out, bool &crc_ok)
{
    unsigned cur = 0, c0 = 0xFFFFu, c1 = 0xFFFFu, c2 = 0xFFFFu, last = 0, last2 = 0;  // c0: over all bytes; c2: all but two
    int have = 0, ones = 0, nbytes = 0;
    crc_ok = false;
    unsigned m_prev = ai_level(v[s - 1], total);
    for (long long j = s; j < nb; ++j) {
        const unsigned m = ai_level(v[j], total), bit = m == m_prev ? 1u : 0u;
        m_prev = m;
        if (bit) {
            if (++ones == 6) {
                if (!(j + 1 < nb && ai_level(v[j + 1], total) != m && have == 6)) return -1;
                crc_ok = nbytes >= 2 && ((c2 ^ 0xFFFFu) & 0xFFFFu) == (last2 | (last << 8));
                return nbytes;
            }
        } else {
            const bool stuffed = ones == 5;
            ones = 0;
            if (stuffed) continue;
        }
        cur |= bit << have;
        if (++have == 8) {
            if (nbytes == AI_MAX_FRAME) return -1;
            if (out) out[nbytes] = static_cast<unsigned char>(cur);
            ++nbytes;
            c2 = c1, c1 = c0, c0 = ai_crc_byte(c0, cur);
            last2 = last, last = cur;
            cur = 0, have = 0;
        }
    }
    return -1;
}

__global__ __launch_bounds__(AI_THREADS) void k_ais_frames(AisFrameArgs g)
{
    const long long s = static_cast<long long>(blockIdx.x) * AI_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    const long long nb = g.count_of[p];
    if (s < AI_LEVEL_FIRST || s > nb) return;
    const int *v = g.v + p * g.nsym;
    long long total = 0;
    for (int k = 0; k < AI_LEVEL_COUNT; ++k) total += v[s - AI_LEVEL_FIRST + k];
    unsigned word = 0, m_prev = ai_level(v[s - 23], total);  // b[s-22 .. s-1], first bit most significant
    for (int k = 0; k < 22; ++k) {
        const unsigned m = ai_level(v[s - 22 + k], total);
        word = (word << 1) | (m == m_prev ? 1u : 0u);
        m_prev = m;
    }
    if ((word & 0xFFu) != 0x7Eu) return;
    if ((word >> 8) != 0x1555u && (word >> 8) != 0x2AAAu) return;
    bool crc_ok;
    const int nbytes = ai_walk(v, s, nb, total, nullptr, crc_ok);
    if (nbytes < AI_MIN_FRAME) return;
    atomicAdd(g.counts + 1, 1ULL);
    if (!crc_ok) return;
    const unsigned long long at = atomicAdd(g.counts, 1ULL);
    if (at >= static_cast<unsigned long long>(g.capacity)) return;
    long long *e4 = g.list + 4 * at;
    e4[0] = p;
    e4[1] = s;
    e4[2] = ai_instant(g.W, g.step, s, p);
    e4[3] = nbytes;
    unsigned char *slot = g.slots + at * IQA_AIS_SLOT_BYTES;
    ai_walk(v, s, nb, total, slot, crc_ok);
    for (int k = nbytes; k < IQA_AIS_SLOT_BYTES; ++k) slot[k] = 0;
}

static_assert(ai_lds_words(AI_MAX_TAPS) * 4 <= 64 * 1024, "the filter window must fit the default LDS allowance");
static_assert(ai_front(AI_MAX_TAPS) % 8 == 0 && ai_front(1) == 0, "taps are read two int4 per group");
static_assert(12868LL * 256 * AI_MAX_TAPS < (1LL << 31), "the filter sums stay inside int32 for any taps of |h| <= 256");

static bool ai_window_ok(int window) { return window >= 1 && window <= AI_MAX_TAPS; }
static bool ai_step_ok(double step) { return step >= 5.0 / 8.0 && step <= IQA_AIS_MAX_SPS / 8.0; }

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_ais_filter(const void *theta_dev, int64_t n, const void *hist_dev, int32_t window, const void *taps_dev, void *t_out_dev,
                              void *s_out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (!ai_window_ok(window)) return fail_inval("window must be 1 .. 3 IQA_AIS_MAX_SPS - 1");
    if (n == 0) return IQA_OK;
    if (!theta_dev || !taps_dev || !s_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    AisFilterArgs g;
    g.theta = static_cast<const float *>(theta_dev);
    g.hist = static_cast<const int *>(hist_dev);
    g.taps = static_cast<const short *>(taps_dev);
    g.t_out = static_cast<int *>(t_out_dev);
    g.s_out = static_cast<int *>(s_out_dev);
    g.n = n;
    g.W = window;
    const size_t lds = static_cast<size_t>(ai_lds_words(window)) * sizeof(int);
    hipLaunchKernelGGL(k_ais_filter, grid1d(n, AI_TILE), dim3(AI_THREADS), lds, as_stream(stream), g);
    return check_launch("k_ais_filter");
}

extern "C" int iqa_ais_symbols(const void *s_dev, int64_t n, int32_t window, double step, int64_t nsym, void *v_out_dev, void *stream)
{
    if (n < 0 || nsym < 0) return fail_inval("negative length");
    if (!ai_window_ok(window)) return fail_inval("window must be 1 .. 3 IQA_AIS_MAX_SPS - 1");
    if (!ai_step_ok(step)) return fail_inval("step must be sps / 8 with 5 <= sps <= IQA_AIS_MAX_SPS");
    if (nsym == 0) return IQA_OK;
    if (!s_dev || !v_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40) || nsym > (1LL << 37)) return fail_inval("length out of range");
    AisSymbolArgs g;
    g.s = static_cast<const int *>(s_dev);
    g.v = static_cast<int *>(v_out_dev);
    g.n = n;
    g.nsym = nsym;
    g.step = step;
    g.W = window;
    dim3 grid = grid1d(nsym, AI_THREADS);
    grid.y = IQA_AIS_PHASES;
    hipLaunchKernelGGL(k_ais_symbols, grid, dim3(AI_THREADS), 0, as_stream(stream), g);
    return check_launch("k_ais_symbols");
}

extern "C" int iqa_ais_frames(const void *v_dev, int64_t nsym, const int64_t count_of[IQA_AIS_PHASES], int32_t window, double step,
                              void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream)
{
    if (nsym < 0 || capacity < 0) return fail_inval("negative length");
    if (!count_of) return fail_inval("NULL count table");
    if (!counts_dev) return fail_inval("NULL device pointer");
    if (!ai_window_ok(window)) return fail_inval("window must be 1 .. 3 IQA_AIS_MAX_SPS - 1");
    if (!ai_step_ok(step)) return fail_inval("step must be sps / 8 with 5 <= sps <= IQA_AIS_MAX_SPS");
    AisFrameArgs g;
    for (int p = 0; p < IQA_AIS_PHASES; ++p) {
        if (count_of[p] < 0 || count_of[p] > nsym) return fail_inval("count_of must be 0 .. nsym");
        g.count_of[p] = count_of[p];
    }
    if (nsym > (1LL << 37)) return fail_inval("length out of range");
    if (nsym > 0 && (!v_dev || (capacity > 0 && (!list_dev || !slots_dev)))) return fail_inval("NULL device pointer");  // (a refused call clears nothing)
    if (hipMemsetAsync(counts_dev, 0, 2 * sizeof(long long), as_stream(stream)) != hipSuccess) {
        set_error("clearing the frame counts failed");
        return IQA_EHIP;
    }
    if (nsym == 0) return IQA_OK;
    g.v = static_cast<const int *>(v_dev);
    g.nsym = nsym;
    g.list = static_cast<long long *>(list_dev);
    g.slots = static_cast<unsigned char *>(slots_dev);
    g.capacity = capacity;
    g.counts = static_cast<unsigned long long *>(counts_dev);
    g.step = step;
    g.W = window;
    dim3 grid = grid1d(nsym + 1, AI_THREADS);
    grid.y = IQA_AIS_PHASES;
    hipLaunchKernelGGL(k_ais_frames, grid, dim3(AI_THREADS), 0, as_stream(stream), g);
    return check_launch("k_ais_frames");
}
