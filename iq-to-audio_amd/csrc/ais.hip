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
// k_ais_filter: sideband.h's tile and front with one tap table (sb_fir_run8<1>: one accumulator per output, 24-bit
// multiply-add).
// k_ais_symbols and k_ais_frames run once per run and read global memory directly.
#include "sideband.h"

namespace iqa {

constexpr int AI_MAX_TAPS = 3 * IQA_AIS_MAX_SPS - 1;  // 299
constexpr float AI_THETA_SCALE = 4096.0f;
constexpr int AI_MIN_FRAME = 11, AI_MAX_FRAME = IQA_AIS_SLOT_BYTES;
constexpr int AI_LEVEL_FIRST = 24, AI_LEVEL_COUNT = 16;  // the level of s: v[s-24 .. s-9]

struct AisFilterArgs {
    const float *theta;   // [n]
    const int *hist;      // [W - 1]: t in front of theta[0]; NULL = zeros
    const short *taps;    // [W]
    int *t_out;           // [n] or NULL
    int *s_out;           // [n]
    long long n;
    int W;
};

__global__ __launch_bounds__(SB_THREADS) void k_ais_filter(AisFilterArgs g)
{
    extern __shared__ int4 s_ai[];
    const int tid = threadIdx.x, W = g.W, H = sb_front(W);
    int *s_taps = reinterpret_cast<int *>(s_ai);  // [H]: h[1 + j]
    int *s_t = s_taps + H;                        // the image of t from block index A - H
    const long long A = static_cast<long long>(blockIdx.x) * SB_TILE;
    sb_stage_taps<1>(s_taps, g.taps, W, H);
    sb_stage(s_t, H, A, g.n, g.theta, SbScale{AI_THETA_SCALE}, g.hist, W - 1, g.t_out, H);
    __syncthreads();
    const long long a0 = A + tid * SB_RUN;
    if (a0 >= g.n) return;
    const int tap0[1] = {g.taps[0]};
    int sum[1][SB_RUN];
    sb_fir_run8<1>(s_ai, s_t, H + tid * SB_RUN, H, tap0, sum);
    const int(&acc)[SB_RUN] = sum[0];
    if (a0 + SB_RUN <= g.n && (reinterpret_cast<uintptr_t>(g.s_out) & 15u) == 0) {  // (a0 is a multiple of 8: 32 bytes)
        int4 *dst = reinterpret_cast<int4 *>(g.s_out + a0);
        dst[0] = make_int4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_int4(acc[4], acc[5], acc[6], acc[7]);
        return;
    }
#pragma unroll
    for (int r = 0; r < SB_RUN; ++r)
        if (a0 + r < g.n) g.s_out[a0 + r] = acc[r];
}

struct AisSymbolArgs {
    const int *s;      // [n]
    int *v;            // [8][nsym]
    long long n, nsym;
    double step;       // sps / 8
    int W;
};

__global__ __launch_bounds__(SB_THREADS) void k_ais_symbols(AisSymbolArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (i >= g.nsym) return;
    const long long at = sb_instant(g.W, g.step, i, p);
    g.v[p * g.nsym + i] = at < g.n ? g.s[at] : 0;  // (a symbol whose instant lies beyond the stream does not exist: never read)
}

struct AisFrameArgs : SbFrameArgs<int, IQA_AIS_PHASES> {};  // plane: [8][n] symbol values; counts[1]: closed candidates of >= 11 bytes

__device__ __forceinline__ unsigned ai_level(int v, long long total) { return 16LL * v > total ? 1u : 0u; }

// Bit j under the level sum ``total``: (m_j == m_{j-1}); the level in front is carried, so that each is made once.
struct AisBitSource {
    const int *__restrict__ v;
    long long total;
    unsigned m_prev;
    __device__ AisBitSource(const int *v_, long long total_, long long s) : v(v_), total(total_), m_prev(ai_level(v_[s - 1], total_)) {}
    __device__ unsigned bit(long long j)
    {
        const unsigned m = ai_level(v[j], total), b = m == m_prev ? 1u : 0u;
        m_prev = m;
        return b;
    }
    __device__ unsigned ahead(long long j) const { return ai_level(v[j], total) == m_prev ? 1u : 0u; }
};

__global__ __launch_bounds__(SB_THREADS) void k_ais_frames(AisFrameArgs g)
{
    const long long s = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    const long long nb = g.count_of[p];
    if (s < AI_LEVEL_FIRST || s > nb) return;
    const int *v = g.plane + p * g.n;
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
    const AisBitSource src(v, total, s);
    const int nbytes = sb_hdlc_walk<AI_MAX_FRAME>(src, s, nb, nullptr, crc_ok);
    if (nbytes < AI_MIN_FRAME) return;
    unsigned char *slot = sb_emit(g, crc_ok, IQA_AIS_SLOT_BYTES, p, s, p, nbytes);
    if (!slot) return;
    sb_hdlc_walk<AI_MAX_FRAME>(src, s, nb, slot, crc_ok);
    for (int k = nbytes; k < IQA_AIS_SLOT_BYTES; ++k) slot[k] = 0;
}

static_assert(sb_fir_words(1, AI_MAX_TAPS) * 4 <= 64 * 1024, "the filter window must fit the default LDS allowance");
static_assert(sb_front(AI_MAX_TAPS) % 8 == 0 && sb_front(1) == 0, "taps are read two int4 per group");
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
    const size_t lds = static_cast<size_t>(sb_fir_words(1, window)) * sizeof(int);
    hipLaunchKernelGGL(k_ais_filter, grid1d(n, SB_TILE), dim3(SB_THREADS), lds, as_stream(stream), g);
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
    dim3 grid = grid1d(nsym, SB_THREADS);
    grid.y = IQA_AIS_PHASES;
    hipLaunchKernelGGL(k_ais_symbols, grid, dim3(SB_THREADS), 0, as_stream(stream), g);
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
    if (!sb_copy_counts(count_of, nsym, g.count_of)) return fail_inval("count_of must be 0 .. nsym");
    if (nsym > (1LL << 37)) return fail_inval("length out of range");
    if (nsym > 0 && (!v_dev || (capacity > 0 && (!list_dev || !slots_dev)))) return fail_inval("NULL device pointer");  // (a refused call clears nothing)
    if (int rc = sb_clear_counts(counts_dev, stream)) return rc;
    if (nsym == 0) return IQA_OK;
    sb_fill_frames(g, v_dev, nsym, list_dev, slots_dev, capacity, counts_dev, step, window);
    hipLaunchKernelGGL(k_ais_frames, sb_frames_grid(nsym, IQA_AIS_PHASES), dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_ais_frames");
}
