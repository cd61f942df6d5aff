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
// k_afsk_correlate: a workgroup owns 2048 consecutive samples.  It quantises them (and the window in front of them) into
// LDS and stages the four tap tables as one int4 per k, zero-padded to a multiple of 8 taps.  Each thread then makes 8
// consecutive outputs of all four correlators: per group of 8 taps it reads 8 more t values into a register window of 16
// and does 8 x 8 x 4 multiply-adds (|t| < 2^23 and |tap| <= 256: the 24-bit multiply-add, which runs at the full vector
// rate where the 32-bit multiply runs at a quarter of it).  Taps are read at a wave-uniform address (a broadcast).  Lanes
// are 8 samples apart, so the t image is padded by one word per 8 as k_pocsag_integrate's is: a fixed tap of consecutive
// lanes is 9 words apart, conflict-free on the 32 banks of a ds_read_b32 half-wave.
// k_afsk_bits and k_afsk_frames run once per run on the byte plane and read global memory directly.
#include "common.h"

namespace iqa {

constexpr int AF_THREADS = 256;
constexpr int AF_RUN = 8;                       // consecutive outputs of a thread of k_afsk_correlate, and its tap group
constexpr int AF_TILE = AF_THREADS * AF_RUN;    // 2048
constexpr int AF_MAX_TAPS = (IQA_AFSK_MAX_SPS + AF_RUN - 1) / AF_RUN * AF_RUN;
constexpr float AF_THETA_SCALE = 4096.0f;
constexpr int AF_VARIANTS = IQA_AFSK_GAINS * IQA_AFSK_PHASES;  // 24
constexpr int AF_MIN_FRAME = 17, AF_MAX_FRAME = 330;
constexpr unsigned AF_CRC_POLY = 0x8408u;

__host__ __device__ constexpr int af_pad(int i) { return i + (i >> 3); }
__host__ __device__ constexpr int af_taps_padded(int L) { return (L + AF_RUN - 1) / AF_RUN * AF_RUN; }

// acc += a b for |a|, |b| < 2^23 (the low 32 bits of the 24-bit product; the operands are sign-extended from bit 23, which is
// why iqa_hotpath.h makes |t| < 2^23 a precondition of iqa_afsk_correlate).  Written out: from ``acc += __mul24(a, b)`` the
// compiler makes 256 separate products per tap group and adds them three at a time, 1.5 instructions and a live register
// per multiply-add.
__device__ __forceinline__ void af_mad24(int &acc, int a, int b)
{
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

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

__global__ __launch_bounds__(AF_THREADS) void k_afsk_correlate(AfskCorrArgs g)
{
    extern __shared__ int4 s_af[];
    // H = Lp values are staged in front of the tile: Lp - 1 that taps reach, and one more that the register window loads
    // with its last group of 8 and never uses.
    const int tid = threadIdx.x, L = g.L, Lp = af_taps_padded(L), H = Lp;
    int4 *s_taps = s_af;                               // [Lp]: (c_1200, s_1200, c_2200, s_2200)[k], zero for k >= L
    int *s_t = reinterpret_cast<int *>(s_af + Lp);     // s_t[af_pad(i)] = t at block index A - H + i, i = 0 .. H + AF_TILE - 1
    const long long A = static_cast<long long>(blockIdx.x) * AF_TILE;
    for (int k = tid; k < Lp; k += AF_THREADS) {
        int4 v = make_int4(0, 0, 0, 0);
        if (k < L) v = make_int4(g.taps[k], g.taps[L + k], g.taps[2 * L + k], g.taps[3 * L + k]);
        s_taps[k] = v;
    }
    for (int i = tid; i < H + AF_TILE; i += AF_THREADS) {
        const long long a = A - H + i;
        int v = 0;
        if (a < 0) {
            if (g.hist && a >= -(L - 1)) v = g.hist[(L - 1) + a];  // (the index is 0 .. L-2; further back only zero taps reach)
        } else if (a < g.n) {
            v = __float2int_rn(g.theta[a] * AF_THETA_SCALE);
            if (i >= H) g.t_out[a] = v;
        }
        s_t[af_pad(i)] = v;
    }
    __syncthreads();
    const long long a0 = A + tid * AF_RUN;
    if (a0 >= g.n) return;
    const int first = H + tid * AF_RUN;  // LDS index (unpadded) of this thread's first output
    int acc[4][AF_RUN];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < AF_RUN; ++r) acc[f][r] = 0;
    // w[j] = t at LDS index first - kb - 8 + j, j = 0 .. 15: output r, tap kb + kk reads index first + r - kb - kk = w[8 + r - kk]
    int w[2 * AF_RUN];
#pragma unroll
    for (int j = 0; j < AF_RUN; ++j) w[AF_RUN + j] = s_t[af_pad(first + j)];
    for (int kb = 0; kb < Lp; kb += AF_RUN) {
#pragma unroll
        for (int j = 0; j < AF_RUN; ++j) w[j] = s_t[af_pad(first - kb - AF_RUN + j)];  // (first - kb - 8 >= H - Lp = 0)
#pragma unroll
        for (int kk = 0; kk < AF_RUN; ++kk) {
            const int4 tp = s_taps[kb + kk];
#pragma unroll
            for (int r = 0; r < AF_RUN; ++r) {
                const int v = w[AF_RUN + r - kk];
                af_mad24(acc[0][r], tp.x, v);
                af_mad24(acc[1][r], tp.y, v);
                af_mad24(acc[2][r], tp.z, v);
                af_mad24(acc[3][r], tp.w, v);
            }
        }
#pragma unroll
        for (int j = 0; j < AF_RUN; ++j) w[AF_RUN + j] = w[j];
    }
    unsigned char sg[AF_RUN];
#pragma unroll
    for (int r = 0; r < AF_RUN; ++r) {
        const long long i1 = acc[0][r], q1 = acc[1][r], i2 = acc[2][r], q2 = acc[3][r];
        const long long e1 = (i1 * i1 + q1 * q1) >> 4, e2 = (i2 * i2 + q2 * q2) >> 4;
        sg[r] = static_cast<unsigned char>((e1 - e2 > 0 ? 1 : 0) | (e1 - 4 * e2 > 0 ? 2 : 0) | (4 * e1 - e2 > 0 ? 4 : 0));
        if (a0 + r < g.n) {
            if (g.e1200) g.e1200[a0 + r] = e1;
            if (g.e2200) g.e2200[a0 + r] = e2;
        }
    }
    if (a0 + AF_RUN <= g.n) {  // (a0 is a multiple of 8 and the plane comes from an allocator: 8-byte aligned)
        unsigned long long packed = 0;
#pragma unroll
        for (int r = 0; r < AF_RUN; ++r) packed |= static_cast<unsigned long long>(sg[r]) << (8 * r);
        if ((reinterpret_cast<uintptr_t>(g.sign) & 7u) == 0) {
            *reinterpret_cast<unsigned long long *>(g.sign + a0) = packed;
            return;
        }
    }
#pragma unroll
    for (int r = 0; r < AF_RUN; ++r)
        if (a0 + r < g.n) g.sign[a0 + r] = sg[r];
}

struct AfskBitArgs {
    const unsigned char *sign;  // [n]
    unsigned char *bits;        // [24][nbits]
    long long n, nbits;
    double step;                // sps / 8
    int L;
};

__device__ __forceinline__ long long af_instant(int L, double step, long long i, int p)
{
    return L - 1 + static_cast<long long>(rint(static_cast<double>(8 * i + p) * step));
}

__global__ __launch_bounds__(AF_THREADS) void k_afsk_bits(AfskBitArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * AF_THREADS + threadIdx.x;
    const int v = blockIdx.y, gain = v / IQA_AFSK_PHASES, p = v % IQA_AFSK_PHASES;
    if (i >= g.nbits) return;
    const long long at = af_instant(g.L, g.step, i, p);
    unsigned char b = 0;  // (a bit whose instant lies beyond the stream does not exist: the frame kernel never reads it)
    if (at < g.n) {
        b = 1;
        if (i > 0) {
            const int m = (g.sign[at] >> gain) & 1, m_prev = (g.sign[af_instant(g.L, g.step, i - 1, p)] >> gain) & 1;
            b = m == m_prev ? 1 : 0;
        }
    }
    g.bits[v * g.nbits + i] = b;
}

struct AfskFrameArgs {
    const unsigned char *bits;  // [24][nbits]
    long long nbits;
    long long count_of[IQA_AFSK_PHASES];  // bits of phase p that exist
    long long *list;            // [capacity][4]: variant, s, start instant, nbytes
    unsigned char *slots;       // [capacity][IQA_AFSK_SLOT_BYTES]
    long long capacity;
    unsigned long long *counts; // [2]: kept frames; closed candidates of >= 17 bytes
    double step;
    int L;
};

__device__ __forceinline__ unsigned af_crc_byte(unsigned reg, unsigned byte)
{
    reg ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) reg = (reg & 1u) ? (reg >> 1) ^ AF_CRC_POLY : reg >> 1;
    return reg;
}

// The walk from s: -1 for an abort / an over-long frame / the end of the stream, else the byte count.  crc_ok: the
// CRC-16/X.25 of all but the last two bytes equals them (low byte first).  out != NULL also stores the bytes.
__device__ int af_walk(const unsigned char *__restrict__ b, long long s, long long nb, unsigned char *out, bool &crc_ok)
{
    unsigned cur = 0, c0 = 0xFFFFu, c1 = 0xFFFFu, c2 = 0xFFFFu, last = 0, last2 = 0;  // c0: over all bytes; c2: all but two
    int have = 0, ones = 0, nbytes = 0;
    crc_ok = false;
    for (long long j = s; j < nb; ++j) {
        const unsigned bit = b[j];
        if (bit) {
            if (++ones == 6) {
                if (!(j + 1 < nb && b[j + 1] == 0 && have == 6)) return -1;
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
            if (nbytes == AF_MAX_FRAME) return -1;
            if (out) out[nbytes] = static_cast<unsigned char>(cur);
            ++nbytes;
            c2 = c1, c1 = c0, c0 = af_crc_byte(c0, cur);
            last2 = last, last = cur;
            cur = 0, have = 0;
        }
    }
    return -1;
}

__global__ __launch_bounds__(AF_THREADS) void k_afsk_frames(AfskFrameArgs g)
{
    const long long s = static_cast<long long>(blockIdx.x) * AF_THREADS + threadIdx.x;
    const int v = blockIdx.y, p = v % IQA_AFSK_PHASES;
    const long long nb = g.count_of[p];
    if (s < 8 || s > nb) return;
    const unsigned char *b = g.bits + v * g.nbits;
    unsigned before = 0, after = 0;  // first bit most significant
    for (int k = 0; k < 8; ++k) before = (before << 1) | b[s - 8 + k];
    if (before != 0x7Eu) return;
    if (s + 8 <= nb) {
        for (int k = 0; k < 8; ++k) after = (after << 1) | b[s + k];
        if (after == 0x7Eu) return;
    }
    bool crc_ok;
    const int nbytes = af_walk(b, s, nb, nullptr, crc_ok);
    if (nbytes < AF_MIN_FRAME) return;
    atomicAdd(g.counts + 1, 1ULL);
    if (!crc_ok) return;
    const unsigned long long at = atomicAdd(g.counts, 1ULL);
    if (at >= static_cast<unsigned long long>(g.capacity)) return;
    long long *e4 = g.list + 4 * at;
    e4[0] = v;
    e4[1] = s;
    e4[2] = af_instant(g.L, g.step, s, p);
    e4[3] = nbytes;
    unsigned char *slot = g.slots + at * IQA_AFSK_SLOT_BYTES;
    af_walk(b, s, nb, slot, crc_ok);
    for (int k = nbytes; k < IQA_AFSK_SLOT_BYTES; ++k) slot[k] = 0;
}

static_assert((4 * AF_MAX_TAPS + af_pad(AF_MAX_TAPS + AF_TILE) + 1) * 4 <= 64 * 1024, "the correlator window must fit the default LDS allowance");
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
    const int Lp = af_taps_padded(window);
    const size_t lds = static_cast<size_t>(4 * Lp + af_pad(Lp + AF_TILE) + 1) * sizeof(int);
    hipLaunchKernelGGL(k_afsk_correlate, grid1d(n, AF_TILE), dim3(AF_THREADS), lds, as_stream(stream), g);
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
    dim3 grid = grid1d(nbits, AF_THREADS);
    grid.y = AF_VARIANTS;
    hipLaunchKernelGGL(k_afsk_bits, grid, dim3(AF_THREADS), 0, as_stream(stream), g);
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
    for (int p = 0; p < IQA_AFSK_PHASES; ++p) {
        if (count_of[p] < 0 || count_of[p] > nbits) return fail_inval("count_of must be 0 .. nbits");
        g.count_of[p] = count_of[p];
    }
    if (nbits > (1LL << 37)) return fail_inval("length out of range");
    if (hipMemsetAsync(counts_dev, 0, 2 * sizeof(long long), as_stream(stream)) != hipSuccess) {
        set_error("clearing the frame counts failed");
        return IQA_EHIP;
    }
    if (nbits == 0) return IQA_OK;
    if (!bits_dev || (capacity > 0 && (!list_dev || !slots_dev))) return fail_inval("NULL device pointer");
    g.bits = static_cast<const unsigned char *>(bits_dev);
    g.nbits = nbits;
    g.list = static_cast<long long *>(list_dev);
    g.slots = static_cast<unsigned char *>(slots_dev);
    g.capacity = capacity;
    g.counts = static_cast<unsigned long long *>(counts_dev);
    g.step = step;
    g.L = window;
    dim3 grid = grid1d(nbits + 1, AF_THREADS);
    grid.y = AF_VARIANTS;
    hipLaunchKernelGGL(k_afsk_frames, grid, dim3(AF_THREADS), 0, as_stream(stream), g);
    return check_launch("k_afsk_frames");
}
