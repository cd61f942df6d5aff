// describe.hip -- what a found channel is (--find-describe), for gfx950: eight integer sums of a channel's
// complex baseband, gated by the finder's activity.
//
// Specification (z the channel stream, sample m its absolute index; D, delay the channelizer's; hop, T, F, S the find plan's;
// gate uint8[S] the eroded activity of the channel):
//   q       = clamp(rintf(ldexpf(x, sh)), -32767, 32767) per component     (float32, half-even; NaN -> 0, +-inf -> +-32767)
//   gate(m) = gate[min(max(m D - delay, 0) / hop, F - 1) / T]              (int64)
//   p = qi^2 + qq^2 (< 2^31);  for m >= 1, with ' the sample in front:  cr = qi qi' + qq qq',  ci = qq qi' - qi qq',
//   a = isqrt(p p')  (cr^2 + ci^2 = p p' < 2^62; isqrt the exact floor)
//   a row of eight int64 per tile of 2048 consecutive samples of the call:
//     N = sum gate(m), NP = sum gate(m) gate(m - 1), S1 = sum_gate p, S2 = sum_gate (p >> 8)^2, E = sum_gate isqrt(p),
//     CR, CI, A = the sums of cr, ci, a over the pairs with both gates on
//   the sample in front of the call's first one is *prev; without it sample 0 of the call forms no pair.
//
// k_describe: the side-band tile (256 threads x 8 consecutive samples).  The workgroup quantises the tile and the sample in
// front of it into LDS, coalesced (image index i at word sb_pad(i): lanes read 9 words apart, conflict-free); a thread takes
// its nine values from there, finds the slice of the sample in front of its run by one division and walks on by compares (a
// division again only where a slice ends), forms its sums in registers, and the workgroup adds them by the integer butterfly
// and one LDS step across the four waves.  Thread 0 stores the row.  No atomics, no float behind the quantiser but the root.
#include "sideband.h"

namespace iqa {

constexpr int DS_SUMS = 8;
constexpr int DS_Q_MAX = 32767;
constexpr int DS_WAVES = SB_THREADS / kWave;
constexpr int DS_IMAGE = sb_pad(SB_TILE + 1) + 1;  // words of one component's image: the tile and the sample in front

struct DescribeArgs {
    const float2 *z;            // [n]
    const float2 *prev;         // [1] or NULL
    const unsigned char *gate;  // [S]
    long long *partials;        // [tiles][8]
    long long n, pos, delay, hop, F, slice_raw;  // slice_raw = hop T: the raw frames of a whole slice
    int sh, D, T, S;
};

__device__ __forceinline__ int ds_quantise(float x, int sh)
{
    const float v = rintf(ldexpf(x, sh));  // (a NaN fails every comparison below)
    return v >= static_cast<float>(DS_Q_MAX) ? DS_Q_MAX : (v <= static_cast<float>(-DS_Q_MAX) ? -DS_Q_MAX : (v == v ? static_cast<int>(v) : 0));
}

// floor(sqrt(v)) for v < 2^62: the root in double is within one of it.
__device__ __forceinline__ unsigned long long ds_isqrt(unsigned long long v)
{
    unsigned long long r = static_cast<unsigned long long>(sqrt(static_cast<double>(v)));
    if (r * r > v) --r;
    else if ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

__global__ __launch_bounds__(SB_THREADS) void k_describe(DescribeArgs g)
{
    __shared__ int s_i[DS_IMAGE], s_q[DS_IMAGE];
    __shared__ long long s_part[DS_WAVES][DS_SUMS];
    const int tid = threadIdx.x;
    const long long base = static_cast<long long>(blockIdx.x) * SB_TILE;  // the call's index of the tile's first sample
    for (int i = tid; i < SB_TILE + 1; i += SB_THREADS) {
        const long long a = base - 1 + i;
        float2 v = make_float2(0.0f, 0.0f);
        if (a >= 0) {
            if (a < g.n) v = g.z[a];
        } else if (g.prev) {
            v = *g.prev;
        }
        s_i[sb_pad(i)] = ds_quantise(v.x, g.sh);
        s_q[sb_pad(i)] = ds_quantise(v.y, g.sh);
    }
    __syncthreads();

    const long long a0 = base + tid * SB_RUN;  // the call's index of the thread's first sample
    long long sum[DS_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (a0 < g.n) {
        // the sample in front of the run: its values, whether it exists, its slice
        int pi = s_i[sb_pad(tid * SB_RUN)], pq = s_q[sb_pad(tid * SB_RUN)];
        long long m = g.pos + a0 - 1;  // absolute; -1 only where the stream starts here
        bool have = a0 > 0 || g.prev != nullptr;
        long long raw = m * g.D - g.delay, bound = 0;  // (m >= -1 and (pos + n) D < 2^62: no overflow)
        int s = 0;
        bool stale = true;  // the slice is found by division
        int gp = 0;
        unsigned pp = static_cast<unsigned>(pi * pi + pq * pq);
        if (m >= 0) {
            const long long r = raw > 0 ? raw : 0;
            const long long f = min(r / g.hop, g.F - 1);
            s = static_cast<int>(f / g.T);
            bound = s == g.S - 1 ? 0x7fffffffffffffffLL : (s + 1LL) * g.slice_raw;
            stale = false;
            gp = g.gate[s] ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j) {
            if (a0 + j >= g.n) break;
            raw += g.D;
            const long long r = raw > 0 ? raw : 0;
            if (stale || r >= bound) {
                const long long f = min(r / g.hop, g.F - 1);
                s = static_cast<int>(f / g.T);
                bound = s == g.S - 1 ? 0x7fffffffffffffffLL : (s + 1LL) * g.slice_raw;
                stale = false;
            }
            const int gc = g.gate[s] ? 1 : 0;
            const int qi = s_i[sb_pad(tid * SB_RUN + 1 + j)], qq = s_q[sb_pad(tid * SB_RUN + 1 + j)];
            const unsigned p = static_cast<unsigned>(qi * qi + qq * qq);
            if (gc) {
                const long long h = p >> 8;
                sum[0] += 1;
                sum[2] += p;
                sum[3] += h * h;
                sum[4] += static_cast<long long>(ds_isqrt(p));
                if (gp && have) {
                    sum[1] += 1;
                    sum[5] += static_cast<long long>(qi) * pi + static_cast<long long>(qq) * pq;
                    sum[6] += static_cast<long long>(qq) * pi - static_cast<long long>(qi) * pq;
                    sum[7] += static_cast<long long>(ds_isqrt(static_cast<unsigned long long>(p) * pp));
                }
            }
            pi = qi, pq = qq, pp = p, gp = gc, have = true;
        }
    }
#pragma unroll
    for (int k = 0; k < DS_SUMS; ++k) sum[k] = wave_sum(sum[k]);
    if (tid % kWave == 0) {
#pragma unroll
        for (int k = 0; k < DS_SUMS; ++k) s_part[tid / kWave][k] = sum[k];
    }
    __syncthreads();
    if (tid == 0) {
        long long *row = g.partials + static_cast<long long>(blockIdx.x) * DS_SUMS;
#pragma unroll
        for (int k = 0; k < DS_SUMS; ++k) {
            long long t = 0;
#pragma unroll
            for (int w = 0; w < DS_WAVES; ++w) t += s_part[w][k];
            row[k] = t;
        }
    }
}

static_assert(2LL * DS_Q_MAX * DS_Q_MAX < (1LL << 31), "p stays inside int32");
static_assert((2LL * DS_Q_MAX * DS_Q_MAX >> 8) * (2LL * DS_Q_MAX * DS_Q_MAX >> 8) * SB_TILE < (1LL << 57), "S2 of a tile");

}  // namespace iqa

using namespace iqa;

constexpr int64_t DS_MAX_N = 1LL << 36;  // samples of one call: 2^25 tiles

extern "C" int64_t iqa_describe_tiles(int64_t n) { return n <= 0 ? 0 : (n + SB_TILE - 1) / SB_TILE; }

extern "C" int iqa_describe_accumulate(const void *z_dev, int64_t n, int64_t pos, const void *prev_dev, int32_t sh, int32_t D,
                                       int32_t delay, int32_t hop, int32_t T, int64_t F, int32_t S, const void *gate_dev,
                                       void *partials_dev, void *stream)
{
    if (n < 0 || pos < 0) return fail_inval("negative length or position");
    if (n > DS_MAX_N) return fail_inval("n out of range");
    if (sh < -IQA_DESCRIBE_MAX_SHIFT || sh > IQA_DESCRIBE_MAX_SHIFT) return fail_inval("sh must be -IQA_DESCRIBE_MAX_SHIFT .. IQA_DESCRIBE_MAX_SHIFT");
    if (D < 1 || delay < 0 || hop < 1) return fail_inval("D and hop must be at least 1 and delay must not be negative");
    if (T < 1 || T > IQA_FIND_MAX_SLICE_FRAMES) return fail_inval("T must be 1 .. IQA_FIND_MAX_SLICE_FRAMES");
    if (F < 1 || S < 1 || F > static_cast<int64_t>(S) * T || F <= static_cast<int64_t>(S - 1) * T) return fail_inval("S must be ceil(F / T)");
    if (pos > (1LL << 62) / D - n) return fail_inval("(pos + n) D must stay below 2^62");
    if (prev_dev && pos == 0) return fail_inval("the stream's first sample has none in front: prev must be NULL at pos 0");
    if (n == 0) return IQA_OK;
    if (!z_dev || !gate_dev || !partials_dev) return fail_inval("NULL device pointer");
    DescribeArgs g;
    g.z = static_cast<const float2 *>(z_dev);
    g.prev = static_cast<const float2 *>(prev_dev);
    g.gate = static_cast<const unsigned char *>(gate_dev);
    g.partials = static_cast<long long *>(partials_dev);
    g.n = n;
    g.pos = pos;
    g.delay = delay;
    g.hop = hop;
    g.F = F;
    g.slice_raw = static_cast<long long>(hop) * T;
    g.sh = sh;
    g.D = D;
    g.T = T;
    g.S = S;
    hipLaunchKernelGGL(k_describe, grid1d(n, SB_TILE), dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_describe");
}
