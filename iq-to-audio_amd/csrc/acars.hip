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
// I / Q plane and a second launch: 8 more bytes written and read per sample) and its 2048 - Lh outputs.  It quantises
// them and the W taps in front of them into LDS and stages the two tap tables as one int2 per k, zero-padded to a
// multiple of 8 taps.  Each thread makes 8 consecutive I and Q: per group of 8 taps it reads 8 more q values into a
// register window of 16 and does 8 x 8 x 2 multiply-adds (0 <= q <= 2^15 and |tap| <= 256: the 24-bit multiply-add).  Taps
// are read at a wave-uniform address (a broadcast).  Lanes are 8 samples apart, so the q image and the I / Q planes are
// padded by one word per 8 as k_afsk_correlate's t image is: a fixed tap of consecutive lanes is 9 words apart,
// conflict-free on the 32 banks of a ds_read_b32 half-wave.  I and Q go to LDS, and behind a barrier every output thread
// reads its eight delayed pairs from there.
// k_acars_max, k_acars_bits and k_acars_frames read global memory directly.
#include "common.h"

namespace iqa {

constexpr int AC_THREADS = 256;
constexpr int AC_RUN = 8;                       // consecutive I / Q of a thread of k_acars_detect, and its tap group
constexpr int AC_TILE = AC_THREADS * AC_RUN;    // 2048 evaluations of I / Q per workgroup
constexpr int AC_MAX_TAPS = (IQA_ACARS_MAX_WINDOW + AC_RUN - 1) / AC_RUN * AC_RUN;
constexpr int AC_MAX_LH = (IQA_ACARS_MAX_SPS + AC_RUN - 1) / AC_RUN * AC_RUN;
constexpr int AC_OPENER = 31;                   // transition symbols in front of an opened position
constexpr unsigned AC_OPENER_BITS = 0x0116162Au;  // * SYN SYN SOH, first byte lowest, sent LSB first
constexpr int AC_MIN_BODY = 13, AC_MAX_BODY = 240;
constexpr unsigned AC_CRC_POLY = 0x8408u;
constexpr unsigned AC_ETX = 0x03u, AC_ETB = 0x17u;

__host__ __device__ constexpr int ac_pad(int i) { return i + (i >> 3); }
__host__ __device__ constexpr int ac_round8(int v) { return (v + AC_RUN - 1) / AC_RUN * AC_RUN; }

// acc += a b for |a|, |b| < 2^23 (the low 32 bits of the 24-bit product; see af_mad24 in afsk.hip).
__device__ __forceinline__ void ac_mad24(int &acc, int a, int b)
{
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

// ---- the run's maximum ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(AC_THREADS) void k_acars_max(const float *__restrict__ e, long long n, unsigned *out)
{
    // non-negative floats order as their bit patterns do
    unsigned m = 0;
    const long long stride = static_cast<long long>(gridDim.x) * AC_THREADS;
    for (long long i = static_cast<long long>(blockIdx.x) * AC_THREADS + threadIdx.x; i < n; i += stride) m = max(m, __float_as_uint(e[i]));
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

__global__ __launch_bounds__(AC_THREADS) void k_acars_detect(AcarsDetectArgs g)
{
    extern __shared__ int2 s_ac[];
    // H = Wp values are staged in front of the evaluations: Wp - 1 that taps reach, and one more that the register window
    // loads with its last group of 8 and never uses.
    const int tid = threadIdx.x, W = g.W, Wp = ac_round8(W), H = Wp, Lh = ac_round8(g.L), T = AC_TILE - Lh;
    int2 *s_taps = s_ac;                              // [Wp]: (c, s)[k], zero for k >= W
    int *s_q = reinterpret_cast<int *>(s_ac + Wp);    // s_q[ac_pad(j)] = q at absolute index A - H + j, j = 0 .. H + AC_TILE - 1
    int *s_i = s_q + ac_pad(H + AC_TILE) + 1;         // s_i[ac_pad(i)] = I at absolute index A + i, i = 0 .. AC_TILE - 1
    int *s_qq = s_i + ac_pad(AC_TILE) + 1;            // likewise Q
    const long long out0 = static_cast<long long>(blockIdx.x) * T;  // the first output of this workgroup
    const long long A = out0 - Lh;                    // the first evaluation
    for (int k = tid; k < Wp; k += AC_THREADS) s_taps[k] = k < W ? make_int2(g.taps[k], g.taps[W + k]) : make_int2(0, 0);
    for (int j = tid; j < H + AC_TILE; j += AC_THREADS) {
        const long long a = A - H + j;
        int v = 0;
        if (a >= 0 && a < g.n) {
            v = __float2int_rn(ldexpf(g.e[a], g.sh));
            if (g.q_out && a >= out0) g.q_out[a] = v;  // (a < out0 + T always: j < H + Lh + T)
        }
        s_q[ac_pad(j)] = v;
    }
    __syncthreads();
    const int i0 = tid * AC_RUN;         // this thread's first evaluation, as an index into the workgroup's 2048
    const long long a0 = A + i0;
    const bool live = a0 < g.n && a0 + AC_RUN > 0;  // (elsewhere q is zero under every tap, and I = Q = 0)
    int acc[2][AC_RUN];
#pragma unroll
    for (int r = 0; r < AC_RUN; ++r) acc[0][r] = acc[1][r] = 0;
    if (live) {
        const int first = H + i0;  // index (unpadded) into s_q of this thread's first evaluation
        // w[j] = q at s_q index first - kb - 8 + j, j = 0 .. 15: evaluation r, tap kb + kk reads index first + r - kb - kk = w[8 + r - kk]
        int w[2 * AC_RUN];
#pragma unroll
        for (int j = 0; j < AC_RUN; ++j) w[AC_RUN + j] = s_q[ac_pad(first + j)];
        for (int kb = 0; kb < Wp; kb += AC_RUN) {
#pragma unroll
            for (int j = 0; j < AC_RUN; ++j) w[j] = s_q[ac_pad(first - kb - AC_RUN + j)];  // (first - kb - 8 >= H - Wp = 0)
#pragma unroll
            for (int kk = 0; kk < AC_RUN; ++kk) {
                const int2 tp = s_taps[kb + kk];
#pragma unroll
                for (int r = 0; r < AC_RUN; ++r) {
                    const int v = w[AC_RUN + r - kk];
                    ac_mad24(acc[0][r], tp.x, v);
                    ac_mad24(acc[1][r], tp.y, v);
                }
            }
#pragma unroll
            for (int j = 0; j < AC_RUN; ++j) w[AC_RUN + j] = w[j];
        }
    }
#pragma unroll
    for (int r = 0; r < AC_RUN; ++r) {
        acc[0][r] >>= 8;
        acc[1][r] >>= 8;
        s_i[ac_pad(i0 + r)] = acc[0][r];
        s_qq[ac_pad(i0 + r)] = acc[1][r];
    }
    __syncthreads();
    if (i0 < Lh || a0 >= g.n) return;  // (Lh and i0 are multiples of 8: a thread is all evaluation-only or all output)
    unsigned char sg[AC_RUN];
#pragma unroll
    for (int r = 0; r < AC_RUN; ++r) {
        const int d = i0 + r - g.L;  // (>= Lh - L >= 0)
        const long long I = acc[0][r], Q = acc[1][r], Id = s_i[ac_pad(d)], Qd = s_qq[ac_pad(d)];
        const long long y = g.cr * (Q * Id - I * Qd) - g.sr * (I * Id + Q * Qd);
        sg[r] = y > 0 ? 1 : 0;
        if (a0 + r < g.n) {
            if (g.i_out) g.i_out[a0 + r] = acc[0][r];
            if (g.qq_out) g.qq_out[a0 + r] = acc[1][r];
            if (g.y_out) g.y_out[a0 + r] = y;
        }
    }
    if (a0 + AC_RUN <= g.n) {  // (a0 is a multiple of 8)
        unsigned long long packed = 0;
#pragma unroll
        for (int r = 0; r < AC_RUN; ++r) packed |= static_cast<unsigned long long>(sg[r]) << (8 * r);
        if ((reinterpret_cast<uintptr_t>(g.same) & 7u) == 0) {
            *reinterpret_cast<unsigned long long *>(g.same + a0) = packed;
            return;
        }
    }
#pragma unroll
    for (int r = 0; r < AC_RUN; ++r)
        if (a0 + r < g.n) g.same[a0 + r] = sg[r];
}

// ---- symbol streams -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ long long ac_instant(int W, double step, long long i, int p)
{
    return W - 1 + static_cast<long long>(rint(static_cast<double>(8 * i + p) * step));
}

struct AcarsBitArgs {
    const unsigned char *same;  // [n]
    unsigned char *bits;        // [8][nbits]
    long long n, nbits;
    double step;                // sps / 8
    int W;
};

__global__ __launch_bounds__(AC_THREADS) void k_acars_bits(AcarsBitArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * AC_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    if (i >= g.nbits) return;
    const long long at = ac_instant(g.W, g.step, i, p);
    g.bits[p * g.nbits + i] = at < g.n ? g.same[at] : 0;  // (a symbol beyond the stream does not exist: the walker never reads it)
}

// ---- frames -----------------------------------------------------------------------------------------------------------------

struct AcarsFrameArgs {
    const unsigned char *bits;  // [8][nbits]
    long long nbits;
    long long count_of[IQA_ACARS_PHASES];  // symbols of phase p that exist
    long long *list;            // [capacity][4]: phase, s, start instant, nbytes (body + 2)
    unsigned char *slots;       // [capacity][IQA_ACARS_SLOT_BYTES]
    long long capacity;
    unsigned long long *counts; // [2]: kept blocks; candidates that reached ETX / ETB
    double step;
    int W;
};

__device__ __forceinline__ unsigned ac_crc_byte(unsigned reg, unsigned byte)
{
    reg ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) reg = (reg & 1u) ? (reg >> 1) ^ AC_CRC_POLY : reg >> 1;
    return reg;
}

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
        crc = ac_crc_byte(crc, v);
        if ((v & 0x7Fu) == AC_ETX || (v & 0x7Fu) == AC_ETB) break;
        if (nbytes == AC_MAX_BODY) return -1;
    }
    if (j + 16 > nb) return nbytes;
    const unsigned lo = ac_byte(g, j, b), hi = ac_byte(g, j + 8, b);
    if (out) out[nbytes] = static_cast<unsigned char>(lo), out[nbytes + 1] = static_cast<unsigned char>(hi);
    kept = nbytes >= AC_MIN_BODY && crc == (lo | (hi << 8));
    return nbytes;
}

__global__ __launch_bounds__(AC_THREADS) void k_acars_frames(AcarsFrameArgs a)
{
    const long long s = static_cast<long long>(blockIdx.x) * AC_THREADS + threadIdx.x;
    const int p = blockIdx.y;
    const long long nb = a.count_of[p];
    if (s < AC_OPENER || s > nb) return;
    const unsigned char *g = a.bits + p * a.nbits;
    // transition j = 1 .. 31 of the opener's bits B_0 .. B_31 is (B_j == B_{j-1}); it sits at g[s - 32 + j]
    constexpr unsigned want = ~(AC_OPENER_BITS ^ (AC_OPENER_BITS >> 1)) & 0x7FFFFFFFu;  // bit j - 1: transition j
    unsigned got = 0;
    for (int j = 1; j <= AC_OPENER; ++j) got |= static_cast<unsigned>(g[s - 32 + j] & 1u) << (j - 1);
    if (got != want) return;
    bool kept;
    const int nbytes = ac_walk(g, s, nb, nullptr, kept);
    if (nbytes < 0) return;
    atomicAdd(a.counts + 1, 1ULL);
    if (!kept) return;
    const unsigned long long at = atomicAdd(a.counts, 1ULL);
    if (at >= static_cast<unsigned long long>(a.capacity)) return;
    long long *e4 = a.list + 4 * at;
    e4[0] = p;
    e4[1] = s;
    e4[2] = ac_instant(a.W, a.step, s, p);
    e4[3] = nbytes + 2;
    unsigned char *slot = a.slots + at * IQA_ACARS_SLOT_BYTES;
    ac_walk(g, s, nb, slot, kept);
    for (int k = nbytes + 2; k < IQA_ACARS_SLOT_BYTES; ++k) slot[k] = 0;
}

constexpr size_t ac_lds_ints(int Wp) { return static_cast<size_t>(2 * Wp + ac_pad(Wp + AC_TILE) + 1 + 2 * (ac_pad(AC_TILE) + 1)); }
static_assert(ac_lds_ints(AC_MAX_TAPS) * 4 <= 64 * 1024, "the detector's images must fit the default LDS allowance");
static_assert(AC_TILE - AC_MAX_LH >= AC_RUN, "a workgroup has outputs of its own");
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
    if (hipMemsetAsync(max_out_dev, 0, sizeof(unsigned), as_stream(stream)) != hipSuccess) {
        set_error("clearing the maximum failed");
        return IQA_EHIP;
    }
    if (n == 0) return IQA_OK;
    if (!e_dev) return fail_inval("NULL device pointer");
    const int64_t blocks = (n + AC_THREADS * 16 - 1) / (AC_THREADS * 16);
    hipLaunchKernelGGL(k_acars_max, dim3(static_cast<unsigned>(blocks < 1024 ? blocks : 1024)), dim3(AC_THREADS), 0, as_stream(stream),
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
    const int T = AC_TILE - ac_round8(delay);
    const size_t lds = ac_lds_ints(ac_round8(window)) * sizeof(int);
    hipLaunchKernelGGL(k_acars_detect, grid1d(n, T), dim3(AC_THREADS), lds, as_stream(stream), g);
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
    dim3 grid = grid1d(nbits, AC_THREADS);
    grid.y = IQA_ACARS_PHASES;
    hipLaunchKernelGGL(k_acars_bits, grid, dim3(AC_THREADS), 0, as_stream(stream), g);
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
    for (int p = 0; p < IQA_ACARS_PHASES; ++p) {
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
    g.W = window;
    dim3 grid = grid1d(nbits + 1, AC_THREADS);
    grid.y = IQA_ACARS_PHASES;
    hipLaunchKernelGGL(k_acars_frames, grid, dim3(AC_THREADS), 0, as_stream(stream), g);
    return check_launch("k_acars_frames");
}
