// acars.hip -- ACARS (2400 bit/s audio MSK on an AM airband carrier) beside the AM demodulator, for
// gfx950.  Everything here runs once per run, on the run's stored envelope.
//
// Specification (fs the channel rate, e = |z| the stored envelope, all indices absolute, everything zero in front of the
// stream; sps = fs / 2400, L = rint(sps), W = rint(fs / 1800), c[k] = rint(256 cos(2 pi 1800 k / fs)), s[k] likewise with
// sin, k < W, int16; psi = 2 pi 1800 L / fs, cr = rint(256 cos psi), sr = rint(256 sin psi)):
//   emax    = max e;  sh = 14 - floor(log2 emax)                     (the host reads emax back once)
//   q[n]    = rint(e[n] 2^sh)                                        (int32, half-even, 0 <= q <= 2^15; integers from here on)
//   I[n]    = (sum_{k<W} c[k] q[n-k]) >> 8,  Q[n] with s             (int32 sums: q >= 0, so 2^15 sum_{c>0} c[k] < 2^31)
//   y[n]    = cr (Q I' - I Q') - sr (I I' + Q Q'),  I' = I[n-L], Q' = Q[n-L]   (int64);  same[n] = (y[n] > 0)
//   phase p = 0 .. 7, symbol i: instant n_i = W - 1 + rint((8 i + p) (sps / 8)) (one float64 product, one rint);
//   g_p[i] = same[n_i]
//   a position s opens a candidate iff g[s-31 .. s-1] are the transitions inside the 32 bits of 2A 16 16 01 (LSB first);
//   with the bit in front of s a zero, b_i = b_{i-1} xor !g[i], bytes LSB first up to the first whose low 7 bits are ETX
//   or ETB (more than 240 bytes abort), then two raw bytes; kept iff the CRC-16/KERMIT of the bytes up to ETX / ETB equals
//   those two (low byte first) and there are at least 13 of them.
//
// k_acars_detect: a workgroup evaluates I and Q at 2048 consecutive samples: the Lh = L rounded up to 8 in front of its
// outputs (a second evaluation of what the workgroup before made, Lh / 2048 of the multiply-adds, instead of a stored
// I / Q plane and a second launch: 8 more bytes written and read per sample) and its 2048 - Lh outputs.  The evaluations
// are sideband.h's tile and front with the two tap tables interleaved (sb_fir_run8<2>: 0 <= q <= 2^15 and |tap| <= 256, the
// 24-bit multiply-add).  I and Q go to LDS, padded as the q image is, and behind a barrier every output thread reads its
// eight delayed pairs from there.
// k_acars_max, k_acars_bits and k_acars_frames read global memory directly.
#include "sideband.h"

namespace iqa {

constexpr int AC_MAX_LH = sb_round8(IQA_ACARS_MAX_SPS);
constexpr int AC_OPENER = 31;                   // transition symbols in front of an opened position
constexpr unsigned AC_OPENER_BITS = 0x0116162Au;  // * SYN SYN SOH, first byte lowest, sent LSB first
constexpr int AC_MIN_BODY = 13, AC_MAX_BODY = 240;
constexpr unsigned AC_ETX = 0x03u, AC_ETB = 0x17u;

// ---- the run's maximum ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SB_THREADS) void k_acars_max(const float *__restrict__ e, long long n, unsigned *out)
{
    // non-negative floats order as their bit patterns do
    unsigned m = 0;
    const long long stride = static_cast<long long>(gridDim.x) * SB_THREADS;
    for (long long i = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x; i < n; i += stride) m = max(m, __float_as_uint(e[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, static_cast<unsigned>(__shfl_xor(static_cast<int>(m), o, kWave)));
    if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicMax(out, m);
}

// ---- quantiser, correlator, differential detector -----------------------------------------------------------------------

struct AcarsDetectArgs {
    const float *e;        // [n]
    const short *taps;     // [2][W]: c, s
    int *q_out;            // [n] or NULL
    int *i_out;            // [n] or NULL
    int *qq_out;           // [n] or NULL (Q)
    long long *y_out;      // [n] or NULL
    unsigned char *same;   // [n]
    long long n;
    int sh, W, L, cr, sr;
};

__global__ __launch_bounds__(SB_THREADS) void k_acars_detect(AcarsDetectArgs g)
{
    extern __shared__ int4 s_ac[];
    const int tid = threadIdx.x, W = g.W, H = sb_front(W), Lh = sb_round8(g.L), T = SB_TILE - Lh;
    int *s_taps = reinterpret_cast<int *>(s_ac);      // [H][2]: (c, s)[1 + j]
    int *s_q = s_taps + 2 * H;                        // the image of q from absolute index A - H
    int *s_i = s_q + sb_pad(H + SB_TILE) + 1;         // s_i[sb_pad(i)] = I at absolute index A + i, i = 0 .. SB_TILE - 1
    int *s_qq = s_i + sb_pad(SB_TILE) + 1;            // likewise Q
    const long long out0 = static_cast<long long>(blockIdx.x) * T;  // the first output of this workgroup
    const long long A = out0 - Lh;                    // the first evaluation
    sb_stage_taps<2>(s_taps, g.taps, W, H);
    sb_stage(s_q, H, A, g.n, g.e, SbLdexp{g.sh}, nullptr, 0, g.q_out, H + Lh);  // (q_out from out0 on; a < out0 + T always)
    __syncthreads();
    const int i0 = tid * SB_RUN;         // this thread's first evaluation, as an index into the workgroup's 2048
    const long long a0 = A + i0;
    int acc[2][SB_RUN];
    if (a0 < g.n && a0 + SB_RUN > 0) {
        const int tap0[2] = {g.taps[0], g.taps[W]};
        sb_fir_run8<2>(s_ac, s_q, H + i0, H, tap0, acc);
    } else {  // (q is zero under every tap, and I = Q = 0)
#pragma unroll
        for (int r = 0; r < SB_RUN; ++r) acc[0][r] = acc[1][r] = 0;
    }
#pragma unroll
    for (int r = 0; r < SB_RUN; ++r) {
        acc[0][r] >>= 8;
        acc[1][r] >>= 8;
        s_i[sb_pad(i0 + r)] = acc[0][r];
        s_qq[sb_pad(i0 + r)] = acc[1][r];
    }
    __syncthreads();
    if (i0 < Lh || a0 >= g.n) return;  // (Lh and i0 are multiples of 8: a thread is all evaluation-only or all output)
    unsigned char sg[SB_RUN];
#pragma unroll
    for (int r = 0; r < SB_RUN; ++r) {
        const int d = i0 + r - g.L;  // (>= Lh - L >= 0)
        const long long I = acc[0][r], Q = acc[1][r], Id = s_i[sb_pad(d)], Qd = s_qq[sb_pad(d)];
        const long long y = g.cr * (Q * Id - I * Qd) - g.sr * (I * Id + Q * Qd);
        sg[r] = y > 0 ? 1 : 0;
        if (a0 + r < g.n) {
            if (g.i_out) g.i_out[a0 + r] = acc[0][r];
            if (g.qq_out) g.qq_out[a0 + r] = acc[1][r];
            if (g.y_out) g.y_out[a0 + r] = y;
        }
    }
    sb_store_flags8(g.same, a0, g.n, sg);
}

// ---- symbol streams -------------------------------------------------------------------------------------------------------

struct AcarsBitArgs {
    const unsigned char *same;  // [n]
    unsigned char *bits;        // [8][nbits]
    long long n, nbits;
    double step;                // sps / 8
    int W;
};

__global__ __launch_bounds__(SB_THREADS) void k_acars_bits(AcarsBitArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (i >= g.nbits) return;
    const long long at = sb_instant(g.W, g.step, i, p);
    g.bits[p * g.nbits + i] = at < g.n ? g.same[at] : 0;  // (a symbol beyond the stream does not exist: the walker never reads it)
}

// ---- frames -----------------------------------------------------------------------------------------------------------------

struct AcarsFrameArgs : SbFrameArgs<unsigned char, IQA_ACARS_PHASES> {};  // plane: [8][n] symbols; nbytes: body + 2; counts[1]: candidates that reached ETX / ETB

// Eight symbols from j -> one byte, least significant bit first; b is the running bit.
__device__ __forceinline__ unsigned ac_byte(const unsigned char *__restrict__ g, long long j, unsigned &b)
{
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        b ^= (g[j + k] ^ 1u) & 1u;
        v |= b << k;
    }
    return v;
}

// The walk from s: -1 where ETX / ETB is not reached (the end of the stream, more than 240 bytes), else the count of bytes up
// to and including it.  kept: the two bytes behind it exist, they are the CRC of those bytes and there are >= 13 of them.
// out != NULL also stores the bytes and the two behind them.
__device__ int ac_walk(const unsigned char *__restrict__ g, long long s, long long nb, unsigned char *out, bool &kept)
{
    unsigned b = 0, crc = 0;
    int nbytes = 0;
    long long j = s;
    kept = false;
    for (;;) {
        if (j + 8 > nb) return -1;
        const unsigned v = ac_byte(g, j, b);
        j += 8;
        if (out) out[nbytes] = static_cast<unsigned char>(v);
        ++nbytes;
        crc = sb_crc16_step(crc, v);
        if ((v & 0x7Fu) == AC_ETX || (v & 0x7Fu) == AC_ETB) break;
        if (nbytes == AC_MAX_BODY) return -1;
    }
    if (j + 16 > nb) return nbytes;
    const unsigned lo = ac_byte(g, j, b), hi = ac_byte(g, j + 8, b);
    if (out) out[nbytes] = static_cast<unsigned char>(lo), out[nbytes + 1] = static_cast<unsigned char>(hi);
    kept = nbytes >= AC_MIN_BODY && crc == (lo | (hi << 8));
    return nbytes;
}

__global__ __launch_bounds__(SB_THREADS) void k_acars_frames(AcarsFrameArgs a)
{
    const long long s = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    const long long nb = a.count_of[p];
    if (s < AC_OPENER || s > nb) return;
    const unsigned char *g = a.plane + p * a.n;
    // transition j = 1 .. 31 of the opener's bits B_0 .. B_31 is (B_j == B_{j-1}); it sits at g[s - 32 + j]
    constexpr unsigned want = ~(AC_OPENER_BITS ^ (AC_OPENER_BITS >> 1)) & 0x7FFFFFFFu;  // bit j - 1: transition j
    unsigned got = 0;
    for (int j = 1; j <= AC_OPENER; ++j) got |= static_cast<unsigned>(g[s - 32 + j] & 1u) << (j - 1);
    if (got != want) return;
    bool kept;
    const int nbytes = ac_walk(g, s, nb, nullptr, kept);
    if (nbytes < 0) return;
    unsigned char *slot = sb_emit(a, kept, IQA_ACARS_SLOT_BYTES, p, s, p, nbytes + 2);
    if (!slot) return;
    ac_walk(g, s, nb, slot, kept);
    for (int k = nbytes + 2; k < IQA_ACARS_SLOT_BYTES; ++k) slot[k] = 0;
}

constexpr size_t ac_lds_ints(int W) { return static_cast<size_t>(sb_fir_words(2, W) + 2 * (sb_pad(SB_TILE) + 1)); }
static_assert(ac_lds_ints(IQA_ACARS_MAX_WINDOW) * 4 <= 64 * 1024, "the detector's images must fit the default LDS allowance");
static_assert(SB_TILE - AC_MAX_LH >= SB_RUN, "a workgroup has outputs of its own");
static_assert(IQA_ACARS_SLOT_BYTES >= AC_MAX_BODY + 2, "a slot holds the longest block and its check sequence");
// q >= 0: a sum is at most 2^15 times the sum of a table's positive (or negative) taps, below 256 (W / pi + 1)
static_assert((1LL << 15) * 256 * (IQA_ACARS_MAX_WINDOW * 113 / 355 + 2) < (1LL << 31), "the correlator sums stay inside int32");

}  // namespace iqa

using namespace iqa;

static int acars_geometry(int32_t window, int32_t delay)
{
    if (window < 1 || window > IQA_ACARS_MAX_WINDOW) return fail_inval("window must be 1 .. IQA_ACARS_MAX_WINDOW");
    if (delay < 8 || delay > IQA_ACARS_MAX_SPS) return fail_inval("delay must be 8 .. IQA_ACARS_MAX_SPS");
    return IQA_OK;
}

extern "C" int iqa_acars_max(const void *e_dev, int64_t n, void *max_out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (!max_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    if (n > 0 && !e_dev) return fail_inval("NULL device pointer");
    if (hipMemsetAsync(max_out_dev, 0, sizeof(unsigned), as_stream(stream)) != hipSuccess) {  // (behind every check)
        set_error("clearing the maximum failed");
        return IQA_EHIP;
    }
    if (n == 0) return IQA_OK;
    const int64_t blocks = (n + SB_THREADS * 16 - 1) / (SB_THREADS * 16);
    hipLaunchKernelGGL(k_acars_max, dim3(static_cast<unsigned>(blocks < 1024 ? blocks : 1024)), dim3(SB_THREADS), 0, as_stream(stream),
                       static_cast<const float *>(e_dev), static_cast<long long>(n), static_cast<unsigned *>(max_out_dev));
    return check_launch("k_acars_max");
}

extern "C" int iqa_acars_detect(const void *e_dev, int64_t n, int32_t shift, int32_t window, int32_t delay, const void *taps_dev,
                                int32_t cr, int32_t sr, void *q_out_dev, void *i_out_dev, void *qq_out_dev, void *y_out_dev,
                                void *same_out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (int rc = acars_geometry(window, delay)) return rc;
    if (shift < -160 || shift > 200) return fail_inval("shift out of range");
    if (cr < -256 || cr > 256 || sr < -256 || sr > 256) return fail_inval("|cr|, |sr| must be <= 256");
    if (n == 0) return IQA_OK;
    if (!e_dev || !taps_dev || !same_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    AcarsDetectArgs g;
    g.e = static_cast<const float *>(e_dev);
    g.taps = static_cast<const short *>(taps_dev);
    g.q_out = static_cast<int *>(q_out_dev);
    g.i_out = static_cast<int *>(i_out_dev);
    g.qq_out = static_cast<int *>(qq_out_dev);
    g.y_out = static_cast<long long *>(y_out_dev);
    g.same = static_cast<unsigned char *>(same_out_dev);
    g.n = n;
    g.sh = shift;
    g.W = window;
    g.L = delay;
    g.cr = cr;
    g.sr = sr;
    const int T = SB_TILE - sb_round8(delay);
    const size_t lds = ac_lds_ints(window) * sizeof(int);
    hipLaunchKernelGGL(k_acars_detect, grid1d(n, T), dim3(SB_THREADS), lds, as_stream(stream), g);
    return check_launch("k_acars_detect");
}

extern "C" int iqa_acars_bits(const void *same_dev, int64_t n, int32_t window, double step, int64_t nbits, void *bits_out_dev, void *stream)
{
    if (n < 0 || nbits < 0) return fail_inval("negative length");
    if (window < 1 || window > IQA_ACARS_MAX_WINDOW) return fail_inval("window must be 1 .. IQA_ACARS_MAX_WINDOW");
    if (!(step >= 1.0 && step <= IQA_ACARS_MAX_SPS / 8.0)) return fail_inval("step must be sps / 8 with 8 <= sps <= IQA_ACARS_MAX_SPS");
    if (nbits == 0) return IQA_OK;
    if (!bits_out_dev || (n > 0 && !same_dev)) return fail_inval("NULL device pointer");
    if (n > (1LL << 40) || nbits > (1LL << 37)) return fail_inval("length out of range");
    AcarsBitArgs g;
    g.same = static_cast<const unsigned char *>(same_dev);
    g.bits = static_cast<unsigned char *>(bits_out_dev);
    g.n = n;
    g.nbits = nbits;
    g.step = step;
    g.W = window;
    dim3 grid = grid1d(nbits, SB_THREADS);
    grid.y = IQA_ACARS_PHASES;
    hipLaunchKernelGGL(k_acars_bits, grid, dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_acars_bits");
}

extern "C" int iqa_acars_frames(const void *bits_dev, int64_t nbits, const int64_t count_of[IQA_ACARS_PHASES], int32_t window, double step,
                                void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream)
{
    if (nbits < 0 || capacity < 0) return fail_inval("negative length");
    if (!count_of) return fail_inval("NULL count table");
    if (!counts_dev) return fail_inval("NULL device pointer");
    if (window < 1 || window > IQA_ACARS_MAX_WINDOW) return fail_inval("window must be 1 .. IQA_ACARS_MAX_WINDOW");
    if (!(step >= 1.0 && step <= IQA_ACARS_MAX_SPS / 8.0)) return fail_inval("step must be sps / 8 with 8 <= sps <= IQA_ACARS_MAX_SPS");
    AcarsFrameArgs g;
    if (!sb_copy_counts(count_of, nbits, g.count_of)) return fail_inval("count_of must be 0 .. nbits");
    if (nbits > (1LL << 37)) return fail_inval("length out of range");
    if (nbits > 0 && (!bits_dev || (capacity > 0 && (!list_dev || !slots_dev)))) return fail_inval("NULL device pointer");
    if (int rc = sb_clear_counts(counts_dev, stream)) return rc;  // (behind every check: a refused call changes no buffer)
    if (nbits == 0) return IQA_OK;
    sb_fill_frames(g, bits_dev, nbits, list_dev, slots_dev, capacity, counts_dev, step, window);
    hipLaunchKernelGGL(k_acars_frames, sb_frames_grid(nbits, IQA_ACARS_PHASES), dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_acars_frames");
}
