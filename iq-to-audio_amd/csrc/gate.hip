// gate.hip -- the carrier squelch of a run's targets (--squelch), for gfx950: the power of the channel
// stream in integer cells per block, and at the end of the run the frames, the noise floor, the open / closed state per frame
// and the gated audio.
//
// Specification (z the channel stream, sample m its absolute index, n its length; a the channel-rate audio; Lf, H, M, A, R,
// num_open, num_close, ramp the gate plan's):
//   q      = clamp(rintf(ldexpf(x, sh)), -32767, 32767) per component     (float32, half-even; NaN -> 0, +-inf -> +-32767)
//   p      = qi^2 + qq^2 (< 2^31);  cell c = m / 256 of the absolute position holds P = sum p (int64)
//   F      = max(1, n / Lf);  frame f holds samples [f Lf, (f + 1) Lf), the last one runs to n;  E[f] the sum of its cells,
//            N[f] its samples, v[f] = 16 E[f] / N[f]
//   floor  = max(1, the value of rank (F - 1) / 10 among v)
//   open   = 1024 v >= num_open floor;  keep = 1024 v >= num_close floor;  s[f] = 1 where open, 0 where not keep, else s[f - 1]
//   s2[f]  = s[f] and the run of ones of s around f has at least M frames
//   g[f]   = some s2[f'] = 1 with max(0, f - H) <= f' <= min(F - 1, f + A);  (lo, hi)[f] = (f0, f1 + 1) of the run of ones of
//            g around f, or (-1, -1)
//   out[m] = 0 where g[f] = 0, f = min(m / Lf, F - 1);  else a[m] (k < R ? ramp[k] : 1) with k = min(m - lo Lf, b - 1 - m),
//            b = hi Lf, or n where hi = F
//
// k_gate_power: the side-band tile (256 threads x 8 consecutive samples) laid on the absolute tile and clipped to the call, as
// k_keying lays it.  A thread's 8 samples lie in one cell; the 32 threads of a cell add in int64 by an integer butterfly of
// width 32 and one of them stores the cell.  No LDS, no atomics, nothing but integers behind the quantiser.
// k_gate_frames: a thread per frame.  k_gate_floor: one workgroup, a binary search over the value range that counts v <= mid.
// k_gate_state: one workgroup that walks the frames in chunks of 1024 with a carry, five times; every step is the same scan,
// "the nearest frame at or before (behind) this one that has the property".  k_gate_apply: a thread per 8 samples.
#include "sideband.h"

namespace iqa {

constexpr int GT_CELL = 256;
constexpr int GT_CELL_THREADS = GT_CELL / SB_RUN;  // 32
constexpr int GT_Q_MAX = 32767;
constexpr int GT_THREADS = 1024;  // of the one-workgroup kernels
constexpr int GT_WAVES = GT_THREADS / kWave;
constexpr int GT_V_BITS = 36;  // v < 2^36

__device__ __forceinline__ int gt_quantise(float x, int sh)
{
    const float v = rintf(ldexpf(x, sh));  // (a NaN fails every comparison below)
    return v >= static_cast<float>(GT_Q_MAX) ? GT_Q_MAX : (v <= static_cast<float>(-GT_Q_MAX) ? -GT_Q_MAX : (v == v ? static_cast<int>(v) : 0));
}

__device__ __forceinline__ long long gt_power(float re, float im, int sh)
{
    const int qi = gt_quantise(re, sh), qq = gt_quantise(im, sh);
    return static_cast<long long>(qi * qi + qq * qq);
}

// ---- the cells --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SB_THREADS) void k_gate_power(const float2 *__restrict__ z, long long n, long long pos, int sh,
                                                           long long *__restrict__ cells)
{
    const int tid = threadIdx.x;
    const long long m0 = (pos / SB_TILE + blockIdx.x) * SB_TILE + tid * SB_RUN;  // absolute
    const long long a0 = m0 - pos;  // the call's index of the thread's first sample
    long long sum = 0;
    if (a0 >= 0 && a0 + SB_RUN <= n && (reinterpret_cast<uintptr_t>(z + a0) & 15u) == 0) {
        const float4 *v = reinterpret_cast<const float4 *>(z + a0);
#pragma unroll
        for (int j = 0; j < SB_RUN / 2; ++j) {
            const float4 two = v[j];
            sum += gt_power(two.x, two.y, sh) + gt_power(two.z, two.w, sh);
        }
    } else {
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j)
            if (a0 + j >= 0 && a0 + j < n) {
                const float2 one = z[a0 + j];
                sum += gt_power(one.x, one.y, sh);
            }
    }
#pragma unroll
    for (int o = GT_CELL_THREADS / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, kWave);
    const long long c = m0 / GT_CELL, first = pos / GT_CELL, last = (pos + n - 1) / GT_CELL;
    if (tid % GT_CELL_THREADS == 0 && c >= first && c <= last) cells[c - first] = sum;
}

__global__ __launch_bounds__(256) void k_gate_add_cells(const long long *__restrict__ part, long long k, long long *__restrict__ cells)
{
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i < k) cells[i] += part[i];
}

// ---- the frames and the floor -----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_gate_frames(const long long *__restrict__ cells, long long n, long long n_cells, int K, int F,
                                                     long long *__restrict__ v)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const long long c0 = static_cast<long long>(f) * K, c1 = f == F - 1 ? n_cells : c0 + K;
    const long long count = f == F - 1 ? n - c0 * GT_CELL : static_cast<long long>(K) * GT_CELL;
    long long e = 0;
    for (long long c = c0; c < c1; ++c) e += cells[c];
    v[f] = 16 * e / count;
}

// The sum of one int per thread over the workgroup, in every thread.  s_part: GT_WAVES ints; two barriers.
__device__ __forceinline__ int gt_block_sum(int x, int *s_part)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    if (threadIdx.x % kWave == 0) s_part[threadIdx.x / kWave] = x;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < GT_WAVES; ++w) total += s_part[w];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(GT_THREADS) void k_gate_floor(const long long *__restrict__ v, int F, long long *__restrict__ floor_out)
{
    __shared__ int s_part[GT_WAVES];
    const int rank = (F - 1) / 10;
    long long a = 0, b = (1LL << GT_V_BITS) - 1;  // the answer is the least x with more than `rank` values <= x
    while (a < b) {  // (a and b are the same in every thread)
        const long long mid = a + ((b - a) >> 1);
        int count = 0;
        for (int f = threadIdx.x; f < F; f += GT_THREADS) count += v[f] <= mid ? 1 : 0;
        if (gt_block_sum(count, s_part) > rank) b = mid;
        else a = mid + 1;
    }
    if (threadIdx.x == 0) *floor_out = a > 1 ? a : 1;
}

// ---- the state --------------------------------------------------------------------------------------------------------------

// The largest key of the threads 0 .. tid of this chunk and of the chunks before it (*s_carry, which then takes the chunk's
// largest).  Keys are not negative and 0 means "none".  Three barriers.
__device__ __forceinline__ int gt_scan_max(int key, int *s_wave, int *s_carry)
{
    const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int other = __shfl_up(key, o, kWave);
        if (lane >= o) key = max(key, other);
    }
    if (lane == kWave - 1) s_wave[w] = key;
    __syncthreads();
    int front = *s_carry;
    for (int i = 0; i < w; ++i) front = max(front, s_wave[i]);
    key = max(key, front);
    __syncthreads();
    if (threadIdx.x == GT_THREADS - 1) *s_carry = key;
    __syncthreads();
    return key;
}

struct GateStateArgs {
    const long long *v;      // [F]
    const long long *floor;  // [1]
    unsigned char *s, *s2, *g;  // [F]
    int *lo, *hi;            // [F]
    int *work;               // [2 F]: the last closed frame of s at or before f; the last frame of s2 at or before f
    long long num_open, num_close;
    int F, M, H, A;
};

__global__ __launch_bounds__(GT_THREADS) void k_gate_state(GateStateArgs g)
{
    __shared__ int s_wave[GT_WAVES];
    __shared__ int s_carry[2];
    const int tid = threadIdx.x, F = g.F;
    int *last_closed = g.work, *last_kept = g.work + F;
    const long long floor = *g.floor;

    // s: the last frame that is not "hold" decides (its key carries its state in bit 0); and the last closed frame of s
    if (tid < 2) s_carry[tid] = 0;
    __syncthreads();
    for (int base = 0; base < F; base += GT_THREADS) {
        const int f = base + tid;
        int key = 0;
        if (f < F) {
            const long long x = 1024 * g.v[f];
            const bool open = x >= g.num_open * floor, keep = x >= g.num_close * floor;
            if (open || !keep) key = 2 * (f + 1) + (open ? 1 : 0);
        }
        key = gt_scan_max(key, s_wave, s_carry);
        const int s = key & 1;  // (no decision in front: key 0, closed)
        const int closed = gt_scan_max(f < F && !s ? f + 1 : 0, s_wave, s_carry + 1);
        if (f < F) {
            g.s[f] = static_cast<unsigned char>(s);
            last_closed[f] = closed - 1;
        }
    }
    __syncthreads();

    // s2: from the end, the next closed frame of s; the run of ones around f lies between the two
    if (tid == 0) s_carry[0] = 0;
    __syncthreads();
    for (int top = F - 1; top >= 0; top -= GT_THREADS) {
        const int f = top - tid;
        const int s = f >= 0 ? g.s[f] : 1;
        const int key = gt_scan_max(f >= 0 && !s ? F - f : 0, s_wave, s_carry);
        if (f >= 0) g.s2[f] = static_cast<unsigned char>(s && static_cast<long long>(F - key) - last_closed[f] - 1 >= g.M ? 1 : 0);
    }
    __syncthreads();

    // the last frame of s2 at or before f
    if (tid == 0) s_carry[0] = 0;
    __syncthreads();
    for (int base = 0; base < F; base += GT_THREADS) {
        const int f = base + tid;
        const int key = gt_scan_max(f < F && g.s2[f] ? f + 1 : 0, s_wave, s_carry);
        if (f < F) last_kept[f] = key - 1;
    }
    __syncthreads();

    // g: a frame of s2 lies in [f - H, f + A] iff the last one at or before f + A does; lo: behind the last closed frame of g
    if (tid == 0) s_carry[0] = 0;
    __syncthreads();
    for (int base = 0; base < F; base += GT_THREADS) {
        const int f = base + tid;
        int on = 0;
        if (f < F) {
            const long long reach = min(static_cast<long long>(F) - 1, static_cast<long long>(f) + g.A);
            const long long from = max(0LL, static_cast<long long>(f) - g.H);
            on = last_kept[reach] >= from ? 1 : 0;
            g.g[f] = static_cast<unsigned char>(on);
        }
        const int key = gt_scan_max(f < F && !on ? f + 1 : 0, s_wave, s_carry);
        if (f < F) g.lo[f] = on ? key : -1;
    }
    __syncthreads();

    // hi: from the end, the next closed frame of g
    if (tid == 0) s_carry[0] = 0;
    __syncthreads();
    for (int top = F - 1; top >= 0; top -= GT_THREADS) {
        const int f = top - tid;
        const int on = f >= 0 ? g.g[f] : 1;
        const int key = gt_scan_max(f >= 0 && !on ? F - f : 0, s_wave, s_carry);
        if (f >= 0) g.hi[f] = on ? F - key : -1;
    }
}

// ---- the gated audio --------------------------------------------------------------------------------------------------------

struct GateApplyArgs {
    const float *a;  // [n]
    float *out;      // [n]
    const unsigned char *g;  // [F]
    const int *lo, *hi;      // [F]
    const float *ramp;       // [R]
    long long n;
    int Lf, K, F, R, vec;  // K = Lf / 256; vec: a and out are 16-byte aligned
};

__global__ __launch_bounds__(256) void k_gate_apply(GateApplyArgs g)
{
    const long long m0 = (static_cast<long long>(blockIdx.x) * 256 + threadIdx.x) * SB_RUN;
    if (m0 >= g.n) return;
    // the 8 samples lie in one cell, so in one frame
    const int f = static_cast<int>(min((m0 / GT_CELL) / g.K, static_cast<long long>(g.F) - 1));
    float r[SB_RUN];
    if (!g.g[f]) {
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j) r[j] = 0.0f;
    } else {
        const int hi = g.hi[f];
        const long long start = static_cast<long long>(g.lo[f]) * g.Lf, b = hi == g.F ? g.n : static_cast<long long>(hi) * g.Lf;
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j) {
            const long long m = m0 + j, k = min(m - start, b - 1 - m);
            r[j] = (k >= 0 && k < g.R) ? g.ramp[k] : 1.0f;  // (k < 0 only behind n, where nothing is stored)
        }
    }
    const bool on = g.g[f] != 0;
    if (g.vec && m0 + SB_RUN <= g.n) {
        const float4 *src = reinterpret_cast<const float4 *>(g.a + m0);
        float4 *dst = reinterpret_cast<float4 *>(g.out + m0);
        float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f), y = x;
        if (on) {
            x = src[0], y = src[1];
            x.x *= r[0], x.y *= r[1], x.z *= r[2], x.w *= r[3];
            y.x *= r[4], y.y *= r[5], y.z *= r[6], y.w *= r[7];
        }
        dst[0] = x, dst[1] = y;
        return;
    }
#pragma unroll
    for (int j = 0; j < SB_RUN; ++j)
        if (m0 + j < g.n) g.out[m0 + j] = on ? g.a[m0 + j] * r[j] : 0.0f;
}

static_assert(GT_CELL % SB_RUN == 0 && SB_TILE % GT_CELL == 0, "a thread's run lies in one cell and a tile holds whole cells");
static_assert(kWave % GT_CELL_THREADS == 0, "the threads of a cell lie in one wave");

}  // namespace iqa

using namespace iqa;

constexpr int64_t GT_MAX_POS = 1LL << 62;

static int gate_check_frames(int64_t n, int32_t Lf, int32_t F)
{
    if (n < 0) return fail_inval("negative length");
    if (Lf < GT_CELL || Lf > IQA_GATE_MAX_FRAME || Lf % GT_CELL != 0) return fail_inval("Lf must be a multiple of 256, 256 .. IQA_GATE_MAX_FRAME");
    if (n >= GT_MAX_POS) return fail_inval("n must stay below 2^62");
    const int64_t frames = n / Lf > 1 ? n / Lf : 1;
    if (frames > IQA_GATE_MAX_FRAMES) return fail_inval("more than IQA_GATE_MAX_FRAMES frames");
    if (F != frames) return fail_inval("F must be max(1, n / Lf)");
    return IQA_OK;
}

extern "C" int64_t iqa_gate_cells(int64_t pos, int64_t n)
{
    if (n <= 0 || pos < 0) return 0;
    return (pos + n - 1) / GT_CELL - pos / GT_CELL + 1;
}

extern "C" int iqa_gate_power(const void *z_dev, int64_t n, int64_t pos, int32_t sh, void *cells_dev, void *stream)
{
    if (n < 0 || pos < 0) return fail_inval("negative length or position");
    if (sh < -IQA_GATE_MAX_SHIFT || sh > IQA_GATE_MAX_SHIFT) return fail_inval("sh must be -30 .. 30");
    if (pos >= GT_MAX_POS || n >= GT_MAX_POS - pos) return fail_inval("pos + n must stay below 2^62");
    if (n == 0) return IQA_OK;
    if (!z_dev || !cells_dev) return fail_inval("NULL device pointer");
    if (reinterpret_cast<uintptr_t>(z_dev) & 7u) return fail_inval("z must be 8-byte aligned");
    const int64_t tiles = (pos + n - 1) / SB_TILE - pos / SB_TILE + 1;
    if (tiles > 0x7fffffffLL) return fail_inval("n out of range");
    hipLaunchKernelGGL(k_gate_power, dim3(static_cast<unsigned>(tiles)), dim3(SB_THREADS), 0, as_stream(stream),
                       static_cast<const float2 *>(z_dev), static_cast<long long>(n), static_cast<long long>(pos), sh,
                       static_cast<long long *>(cells_dev));
    return check_launch("k_gate_power");
}

extern "C" int iqa_gate_add_cells(const void *part_dev, int64_t k, void *cells_dev, void *stream)
{
    if (k < 0) return fail_inval("negative length");
    if (k > (1LL << 38)) return fail_inval("k out of range");
    if (k == 0) return IQA_OK;
    if (!part_dev || !cells_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_gate_add_cells, grid1d(k, 256), dim3(256), 0, as_stream(stream), static_cast<const long long *>(part_dev),
                       static_cast<long long>(k), static_cast<long long *>(cells_dev));
    return check_launch("k_gate_add_cells");
}

extern "C" int iqa_gate_decide(const void *cells_dev, int64_t n, int32_t Lf, int32_t F, int64_t num_open, int64_t num_close, int32_t M,
                               int32_t H, int32_t A, void *v_dev, void *floor_dev, void *s_dev, void *s2_dev, void *g_dev, void *lo_dev,
                               void *hi_dev, void *work_dev, void *stream)
{
    const int rc = gate_check_frames(n, Lf, F);
    if (rc != IQA_OK) return rc;
    if (num_open < 1 || num_open > IQA_GATE_MAX_NUM) return fail_inval("num_open must be 1 .. IQA_GATE_MAX_NUM");
    if (num_close < 1 || num_close > num_open) return fail_inval("num_close must be 1 .. num_open");
    if (M < 1 || H < 0 || A < 0) return fail_inval("M must be at least 1 and H and A must not be negative");
    if (n == 0) return IQA_OK;
    if (!cells_dev || !v_dev || !floor_dev || !s_dev || !s2_dev || !g_dev || !lo_dev || !hi_dev || !work_dev) return fail_inval("NULL device pointer");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_gate_frames, grid1d(F, 256), dim3(256), 0, st, static_cast<const long long *>(cells_dev), static_cast<long long>(n),
                       static_cast<long long>((n + GT_CELL - 1) / GT_CELL), Lf / GT_CELL, F, static_cast<long long *>(v_dev));
    int launched = check_launch("k_gate_frames");
    if (launched != IQA_OK) return launched;
    hipLaunchKernelGGL(k_gate_floor, dim3(1), dim3(GT_THREADS), 0, st, static_cast<const long long *>(v_dev), F, static_cast<long long *>(floor_dev));
    launched = check_launch("k_gate_floor");
    if (launched != IQA_OK) return launched;
    GateStateArgs g;
    g.v = static_cast<const long long *>(v_dev);
    g.floor = static_cast<const long long *>(floor_dev);
    g.s = static_cast<unsigned char *>(s_dev);
    g.s2 = static_cast<unsigned char *>(s2_dev);
    g.g = static_cast<unsigned char *>(g_dev);
    g.lo = static_cast<int *>(lo_dev);
    g.hi = static_cast<int *>(hi_dev);
    g.work = static_cast<int *>(work_dev);
    g.num_open = num_open;
    g.num_close = num_close;
    g.F = F;
    g.M = M;
    g.H = H;
    g.A = A;
    hipLaunchKernelGGL(k_gate_state, dim3(1), dim3(GT_THREADS), 0, st, g);
    return check_launch("k_gate_state");
}

extern "C" int iqa_gate_apply(const void *audio_dev, int64_t n, int32_t Lf, int32_t F, const void *g_dev, const void *lo_dev,
                              const void *hi_dev, const void *ramp_dev, int32_t R, void *out_dev, void *stream)
{
    const int rc = gate_check_frames(n, Lf, F);
    if (rc != IQA_OK) return rc;
    if (R < 0) return fail_inval("R must not be negative");
    if (n == 0) return IQA_OK;
    if (!audio_dev || !g_dev || !lo_dev || !hi_dev || !out_dev) return fail_inval("NULL device pointer");
    if (R > 0 && !ramp_dev) return fail_inval("NULL ramp table");
    if (audio_dev == out_dev) return fail_inval("out must be a buffer of its own");
    const int64_t threads = (n + SB_RUN - 1) / SB_RUN;
    if ((threads + 255) / 256 > 0x7fffffffLL) return fail_inval("n out of range");
    GateApplyArgs g;
    g.a = static_cast<const float *>(audio_dev);
    g.out = static_cast<float *>(out_dev);
    g.g = static_cast<const unsigned char *>(g_dev);
    g.lo = static_cast<const int *>(lo_dev);
    g.hi = static_cast<const int *>(hi_dev);
    g.ramp = static_cast<const float *>(ramp_dev);
    g.n = n;
    g.Lf = Lf;
    g.K = Lf / GT_CELL;
    g.F = F;
    g.R = R;
    g.vec = ((reinterpret_cast<uintptr_t>(audio_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15u) == 0 ? 1 : 0;
    hipLaunchKernelGGL(k_gate_apply, grid1d(threads, 256), dim3(256), 0, as_stream(stream), g);
    return check_launch("k_gate_apply");
}
