// afsk.hip -- 1200-baud Bell-202 AFSK / AX.25 (HDLC) beside the NFM demodulator, for gfx950.
//
// Specification (fs the channel rate, theta the discriminator output, all indices absolute, everything zero in front of
// the stream; sps = fs / 1200, L = rint(sps), c_f[k] = rint(256 cos(2 pi f k / fs)), s_f[k] likewise with sin, int16):
//   t[n]    = rint(theta[n] 4096)                                   (int32, half-even; integers from here on)
//   I_f[n]  = sum_{k<L} c_f[k] t[n-k],  Q_f[n] with s_f             (int32: 12 868 . 256 . L < 2^31)
//   E_f[n]  = (I_f^2 + Q_f^2) >> 4                                  (int64)
//   sign[n] = bit g set iff a_g E_1200[n] - b_g E_2200[n] > 0,  (a, b) = (1,1), (1,4), (4,1)
//   variant v = 8 g + p, bit i: instant n_i = L - 1 + rint((8 i + p) (sps / 8)) (one float64 product, one rint);
//   m_i = bit g of sign[n_i];  b_i = (m_i == m_{i-1}), b_0 = 1
//   a position s opens a frame iff b[s-8 .. s-1] = 0111 1110 and b[s .. s+7] is not; bytes LSB first, a zero after five
//   ones dropped, a sixth one ends the walk (a closing flag iff the next bit is 0 and 6 bits of the current byte are
//   collected), more than 330 bytes abort; kept iff >= 17 bytes and the CRC-16/X.25 of all but the last two equals them.
//
// k_afsk_correlate: sideband.h's tile and front with the four tap tables interleaved (sb_fir_run8<4>: |t| < 2^23 and
// |tap| <= 256, the 24-bit multiply-add, which runs at the full vector rate where the 32-bit multiply runs at a quarter of
// it); the thread then makes the energies and the slicer flags of its 8 outputs.
// k_afsk_bits and k_afsk_frames run once per run on the byte plane and read global memory directly.
#include "sideband.h"

namespace iqa {

constexpr float AF_THETA_SCALE = 4096.0f;
constexpr int AF_VARIANTS = IQA_AFSK_GAINS * IQA_AFSK_PHASES;  // 24
constexpr int AF_MIN_FRAME = 17, AF_MAX_FRAME = 330;

struct AfskCorrArgs {
    const float *theta;   // [n]
    const int *hist;      // [L - 1]: t in front of theta[0]; NULL = zeros
    const short *taps;    // [4][L]: c_1200, s_1200, c_2200, s_2200
    int *t_out;           // [n]
    unsigned char *sign;  // [n]
    long long *e1200;     // [n] or NULL
    long long *e2200;     // [n] or NULL
    long long n;
    int L;
};

__global__ __launch_bounds__(SB_THREADS) void k_afsk_correlate(AfskCorrArgs g)
{
    extern __shared__ int4 s_af[];
    const int tid = threadIdx.x, L = g.L, H = sb_front(L);
    int *s_taps = reinterpret_cast<int *>(s_af);  // [H][4]: (c_1200, s_1200, c_2200, s_2200)[1 + j]
    int *s_t = s_taps + 4 * H;                    // the image of t from block index A - H
    const long long A = static_cast<long long>(blockIdx.x) * SB_TILE;
    sb_stage_taps<4>(s_taps, g.taps, L, H);
    sb_stage(s_t, H, A, g.n, g.theta, SbScale{AF_THETA_SCALE}, g.hist, L - 1, g.t_out, H);
    __syncthreads();
    const long long a0 = A + tid * SB_RUN;
    if (a0 >= g.n) return;
    const int tap0[4] = {g.taps[0], g.taps[L], g.taps[2 * L], g.taps[3 * L]};
    int acc[4][SB_RUN];
    sb_fir_run8<4>(s_af, s_t, H + tid * SB_RUN, H, tap0, acc);
    unsigned char sg[SB_RUN];
#pragma unroll
    for (int r = 0; r < SB_RUN; ++r) {
        const long long i1 = acc[0][r], q1 = acc[1][r], i2 = acc[2][r], q2 = acc[3][r];
        const long long e1 = (i1 * i1 + q1 * q1) >> 4, e2 = (i2 * i2 + q2 * q2) >> 4;
        sg[r] = static_cast<unsigned char>((e1 - e2 > 0 ? 1 : 0) | (e1 - 4 * e2 > 0 ? 2 : 0) | (4 * e1 - e2 > 0 ? 4 : 0));
        if (a0 + r < g.n) {
            if (g.e1200) g.e1200[a0 + r] = e1;
            if (g.e2200) g.e2200[a0 + r] = e2;
        }
    }
    sb_store_flags8(g.sign, a0, g.n, sg);
}

struct AfskBitArgs {
    const unsigned char *sign;  // [n]
    unsigned char *bits;        // [24][nbits]
    long long n, nbits;
    double step;                // sps / 8
    int L;
};

__global__ __launch_bounds__(SB_THREADS) void k_afsk_bits(AfskBitArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x;
    const int v = blockIdx.y, gain = v / IQA_AFSK_PHASES, p = v % IQA_AFSK_PHASES;
    if (i >= g.nbits) return;
    const long long at = sb_instant(g.L, g.step, i, p);
    unsigned char b = 0;  // (a bit whose instant lies beyond the stream does not exist: the frame kernel never reads it)
    if (at < g.n) {
        b = 1;
        if (i > 0) {
            const int m = (g.sign[at] >> gain) & 1, m_prev = (g.sign[sb_instant(g.L, g.step, i - 1, p)] >> gain) & 1;
            b = m == m_prev ? 1 : 0;
        }
    }
    g.bits[v * g.nbits + i] = b;
}

struct AfskFrameArgs : SbFrameArgs<unsigned char, IQA_AFSK_PHASES> {};  // plane: [24][n] bits; counts[1]: closed candidates of >= 17 bytes

struct AfskBitSource {
    const unsigned char *__restrict__ b;
    __device__ unsigned bit(long long j) const { return b[j]; }
    __device__ unsigned ahead(long long j) const { return b[j]; }
};

__global__ __launch_bounds__(SB_THREADS) void k_afsk_frames(AfskFrameArgs g)
{
    const long long s = static_cast<long long>(blockIdx.x) * SB_THREADS + threadIdx.x;
    const int v = blockIdx.y, p = v % IQA_AFSK_PHASES;
    const long long nb = g.count_of[p];
    if (s < 8 || s > nb) return;
    const unsigned char *b = g.plane + v * g.n;
    unsigned before = 0, after = 0;  // first bit most significant
    for (int k = 0; k < 8; ++k) before = (before << 1) | b[s - 8 + k];
    if (before != 0x7Eu) return;
    if (s + 8 <= nb) {
        for (int k = 0; k < 8; ++k) after = (after << 1) | b[s + k];
        if (after == 0x7Eu) return;
    }
    bool crc_ok;
    const AfskBitSource src{b};
    const int nbytes = sb_hdlc_walk<AF_MAX_FRAME>(src, s, nb, nullptr, crc_ok);
    if (nbytes < AF_MIN_FRAME) return;
    unsigned char *slot = sb_emit(g, crc_ok, IQA_AFSK_SLOT_BYTES, v, s, p, nbytes);
    if (!slot) return;
    sb_hdlc_walk<AF_MAX_FRAME>(src, s, nb, slot, crc_ok);
    for (int k = nbytes; k < IQA_AFSK_SLOT_BYTES; ++k) slot[k] = 0;
}

static_assert(sb_fir_words(4, IQA_AFSK_MAX_SPS) * 4 <= 64 * 1024, "the correlator window must fit the default LDS allowance");
static_assert(12868LL * 256 * 512 < (1LL << 31), "the correlator sums stay inside int32");
static_assert(IQA_AFSK_SLOT_BYTES >= AF_MAX_FRAME, "a slot holds the longest frame");

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_afsk_correlate(const void *theta_dev, int64_t n, const void *hist_dev, int32_t window, const void *taps_dev,
                                  void *t_out_dev, void *sign_out_dev, void *e1200_out_dev, void *e2200_out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (window < 8 || window > IQA_AFSK_MAX_SPS) return fail_inval("window must be 8 .. IQA_AFSK_MAX_SPS");
    if (n == 0) return IQA_OK;
    if (!theta_dev || !taps_dev || !t_out_dev || !sign_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    AfskCorrArgs g;
    g.theta = static_cast<const float *>(theta_dev);
    g.hist = static_cast<const int *>(hist_dev);
    g.taps = static_cast<const short *>(taps_dev);
    g.t_out = static_cast<int *>(t_out_dev);
    g.sign = static_cast<unsigned char *>(sign_out_dev);
    g.e1200 = static_cast<long long *>(e1200_out_dev);
    g.e2200 = static_cast<long long *>(e2200_out_dev);
    g.n = n;
    g.L = window;
    const size_t lds = static_cast<size_t>(sb_fir_words(4, window)) * sizeof(int);
    hipLaunchKernelGGL(k_afsk_correlate, grid1d(n, SB_TILE), dim3(SB_THREADS), lds, as_stream(stream), g);
    return check_launch("k_afsk_correlate");
}

extern "C" int iqa_afsk_bits(const void *sign_dev, int64_t n, int32_t window, double step, int64_t nbits, void *bits_out_dev, void *stream)
{
    if (n < 0 || nbits < 0) return fail_inval("negative length");
    if (window < 8 || window > IQA_AFSK_MAX_SPS) return fail_inval("window must be 8 .. IQA_AFSK_MAX_SPS");
    if (!(step >= 1.0 && step <= IQA_AFSK_MAX_SPS / 8.0)) return fail_inval("step must be sps / 8 with 8 <= sps <= IQA_AFSK_MAX_SPS");
    if (nbits == 0) return IQA_OK;
    if (!sign_dev || !bits_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40) || nbits > (1LL << 37)) return fail_inval("length out of range");
    AfskBitArgs g;
    g.sign = static_cast<const unsigned char *>(sign_dev);
    g.bits = static_cast<unsigned char *>(bits_out_dev);
    g.n = n;
    g.nbits = nbits;
    g.step = step;
    g.L = window;
    dim3 grid = grid1d(nbits, SB_THREADS);
    grid.y = AF_VARIANTS;
    hipLaunchKernelGGL(k_afsk_bits, grid, dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_afsk_bits");
}

extern "C" int iqa_afsk_frames(const void *bits_dev, int64_t nbits, const int64_t count_of[IQA_AFSK_PHASES], int32_t window, double step,
                               void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream)
{
    if (nbits < 0 || capacity < 0) return fail_inval("negative length");
    if (!count_of) return fail_inval("NULL count table");
    if (!counts_dev) return fail_inval("NULL device pointer");
    if (window < 8 || window > IQA_AFSK_MAX_SPS) return fail_inval("window must be 8 .. IQA_AFSK_MAX_SPS");
    if (!(step >= 1.0 && step <= IQA_AFSK_MAX_SPS / 8.0)) return fail_inval("step must be sps / 8 with 8 <= sps <= IQA_AFSK_MAX_SPS");
    AfskFrameArgs g;
    if (!sb_copy_counts(count_of, nbits, g.count_of)) return fail_inval("count_of must be 0 .. nbits");
    if (nbits > (1LL << 37)) return fail_inval("length out of range");
    if (nbits > 0 && (!bits_dev || (capacity > 0 && (!list_dev || !slots_dev)))) return fail_inval("NULL device pointer");
    if (int rc = sb_clear_counts(counts_dev, stream)) return rc;  // (behind every check: a refused call changes no buffer)
    if (nbits == 0) return IQA_OK;
    sb_fill_frames(g, bits_dev, nbits, list_dev, slots_dev, capacity, counts_dev, step, window);
    hipLaunchKernelGGL(k_afsk_frames, sb_frames_grid(nbits, AF_VARIANTS), dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_afsk_frames");
}
