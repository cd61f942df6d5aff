// keying.hip -- whether a found channel's discriminator switches on a symbol clock (--find-decode), for
// gfx950: per window of 2048 samples the gated pairs, the level crossings and, for seven candidate bauds, the sum of a unit
// vector at the clock phase of every crossing.
//
// Specification (theta the discriminator output of the channel stream, sample m its absolute index; D, delay the channelizer's;
// hop, T, F, S the find plan's; gate uint8[S] the eroded activity of the channel; c the centre; inc[7] the clock steps; cs the
// table int16[1024][2] of 1024 cos, 1024 sin):
//   t       = clamp(rintf(theta 4096), -32767, 32767)                         (float32, half-even; NaN -> 0, +-inf -> +-32767)
//   gate(m) = gate[min(max(m D - delay, 0) / hop, F - 1) / T]                  (int64)
//   s       = t >= c;  sample m >= 1 is a pair iff gate(m) and gate(m - 1), a crossing iff it is a pair and s != s'
//   a row of sixteen int32 per window w = m / 2048 of the absolute position, clipped to the call:
//     P = pairs, K = crossings, (C_k, Q_k) = sum over the crossings of cs[((m inc_k) mod 2^32) >> 22], k = 0 .. 6
//   the value in front of the call's first one is *front; without it sample 0 of the call forms no pair.
//
// k_keying: the side-band tile (256 threads x 8 consecutive samples) laid on the absolute window.  sb_stage quantises the
// window's samples and the one in front of it into LDS (image index i at word sb_pad(i): lanes read 9 words apart); the table
// goes to LDS beside it.  A thread takes its nine values from there, walks the gate as k_describe does (one division for the
// run, then a compare per sample, a division again only where a slice ends), forms its flags and sums in registers, and the
// workgroup adds them by the integer butterfly and one LDS step across the four waves.  Thread 0 stores the row.  No atomics,
// nothing but integers behind the quantiser.  (m inc) mod 2^32 needs the low words only: one 32-bit multiply per candidate.
#include "sideband.h"

namespace iqa {

constexpr int KY_BAUDS = 7;
constexpr int KY_SUMS = 2 + 2 * KY_BAUDS;  // 16
constexpr int KY_T_MAX = 32767;
constexpr int KY_TABLE = 1024;
constexpr int KY_WAVES = SB_THREADS / kWave;
constexpr int KY_IMAGE = sb_pad(SB_TILE + 1) + 1;  // words of the image: the window and the sample in front

struct KeyingArgs {
    const float *theta;         // [n]
    const float *front;         // [1] or NULL
    const unsigned char *gate;  // [S]
    const int *cs;              // [1024]: cos in the low half, sin in the high half (int16 each)
    int *rows;                  // [windows][16]
    long long n, pos, delay, hop, F, slice_raw;  // slice_raw = hop T: the raw frames of a whole slice
    int D, T, S, c;
    unsigned inc[KY_BAUDS];
};

__global__ __launch_bounds__(SB_THREADS) void k_keying(KeyingArgs g)
{
    __shared__ int s_t[KY_IMAGE];
    __shared__ int s_cs[KY_TABLE];
    __shared__ int s_part[KY_WAVES][KY_SUMS];
    const int tid = threadIdx.x;
    // the call's index of the window's first sample: negative where the call begins inside the window
    const long long base = (g.pos / SB_TILE + blockIdx.x) * SB_TILE - g.pos;
    sb_stage(s_t, 1, base, g.n, g.theta, SbScale{4096.0f}, nullptr, 0, nullptr, 0);
    // image index -base holds the sample in front of the call (left zero by sb_stage); its owner in sb_stage fills it
    if (g.front && base <= 0 && tid == static_cast<int>(-base) % SB_THREADS) s_t[sb_pad(static_cast<int>(-base))] = SbScale{4096.0f}(*g.front);
    for (int i = tid; i < KY_TABLE; i += SB_THREADS) s_cs[i] = g.cs[i];
    __syncthreads();

    const long long a0 = base + tid * SB_RUN;  // the call's index of the thread's first sample
    int sum[KY_SUMS];
#pragma unroll
    for (int k = 0; k < KY_SUMS; ++k) sum[k] = 0;
    if (a0 < g.n && a0 + SB_RUN > 0) {
        const long long first = a0 > 0 ? a0 : 0;  // the first sample of the run that lies in the call
        // the sample in front of it: whether it exists, its slice
        long long m = g.pos + first - 1;  // absolute; -1 only where the stream starts here
        bool have = first > 0 || g.front != nullptr;
        long long raw = m * g.D - g.delay, bound = 0;  // (m >= -1 and (pos + n) D < 2^62: no overflow)
        int s = 0;
        bool stale = true;  // the slice is found by division
        int gp = 0;
        if (m >= 0) {
            const long long r = raw > 0 ? raw : 0;
            const long long f = min(r / g.hop, g.F - 1);
            s = static_cast<int>(f / g.T);
            bound = s == g.S - 1 ? 0x7fffffffffffffffLL : (s + 1LL) * g.slice_raw;
            stale = false;
            gp = g.gate[s] ? 1 : 0;
        }
        int tp = s_t[sb_pad(tid * SB_RUN)];
        tp = min(max(tp, -KY_T_MAX), KY_T_MAX);
        const unsigned m_lo = static_cast<unsigned>(static_cast<unsigned long long>(g.pos + a0));  // the low word of the run's first position
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j) {
            int tc = s_t[sb_pad(tid * SB_RUN + 1 + j)];
            tc = min(max(tc, -KY_T_MAX), KY_T_MAX);
            if (a0 + j >= 0 && a0 + j < g.n) {
                raw += g.D;
                const long long r = raw > 0 ? raw : 0;
                if (stale || r >= bound) {
                    const long long f = min(r / g.hop, g.F - 1);
                    s = static_cast<int>(f / g.T);
                    bound = s == g.S - 1 ? 0x7fffffffffffffffLL : (s + 1LL) * g.slice_raw;
                    stale = false;
                }
                const int gc = g.gate[s] ? 1 : 0;
                if (gc && gp && have) {
                    sum[0] += 1;
                    if ((tc >= g.c) != (tp >= g.c)) {
                        sum[1] += 1;
#pragma unroll
                        for (int k = 0; k < KY_BAUDS; ++k) {
                            const unsigned ph = (m_lo + static_cast<unsigned>(j)) * g.inc[k];
                            const int v = s_cs[ph >> 22];
                            sum[2 + 2 * k] += static_cast<short>(v & 0xffff);
                            sum[3 + 2 * k] += v >> 16;
                        }
                    }
                }
                gp = gc, have = true;
            }
            tp = tc;
        }
    }
#pragma unroll
    for (int k = 0; k < KY_SUMS; ++k) sum[k] = wave_sum(sum[k]);
    if (tid % kWave == 0) {
#pragma unroll
        for (int k = 0; k < KY_SUMS; ++k) s_part[tid / kWave][k] = sum[k];
    }
    __syncthreads();
    if (tid == 0) {
        int *row = g.rows + static_cast<long long>(blockIdx.x) * KY_SUMS;
#pragma unroll
        for (int k = 0; k < KY_SUMS; ++k) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < KY_WAVES; ++w) t += s_part[w][k];
            row[k] = t;
        }
    }
}

static_assert(static_cast<long long>(SB_TILE) * 1024 < (1LL << 31), "C and Q of a window stay inside int32");

}  // namespace iqa

using namespace iqa;

constexpr int64_t KY_MAX_N = 1LL << 36;  // samples of one call: 2^25 windows and one

extern "C" int64_t iqa_keying_windows(int64_t pos, int64_t n)
{
    if (n <= 0 || pos < 0) return 0;
    return (pos + n - 1) / SB_TILE - pos / SB_TILE + 1;
}

extern "C" int iqa_keying_accumulate(const void *theta_dev, int64_t n, int64_t pos, const void *front_dev, int32_t c, const int32_t *inc,
                                     const void *cs_dev, int32_t D, int32_t delay, int32_t hop, int32_t T, int64_t F, int32_t S,
                                     const void *gate_dev, void *rows_dev, void *stream)
{
    if (n < 0 || pos < 0) return fail_inval("negative length or position");
    if (n > KY_MAX_N) return fail_inval("n out of range");
    if (c < -KY_T_MAX || c > KY_T_MAX) return fail_inval("the centre must be -32767 .. 32767");
    for (int k = 0; inc && k < KY_BAUDS; ++k)
        if (inc[k] < 0 || inc[k] >= (1 << 30)) return fail_inval("a clock step must be 0 .. 2^30 - 1");
    if (D < 1 || delay < 0 || hop < 1) return fail_inval("D and hop must be at least 1 and delay must not be negative");
    if (T < 1 || T > IQA_FIND_MAX_SLICE_FRAMES) return fail_inval("T must be 1 .. IQA_FIND_MAX_SLICE_FRAMES");
    if (F < 1 || S < 1 || F > static_cast<int64_t>(S) * T || F <= static_cast<int64_t>(S - 1) * T) return fail_inval("S must be ceil(F / T)");
    if (pos > (1LL << 62) / D - n) return fail_inval("(pos + n) D must stay below 2^62");
    if (front_dev && pos == 0) return fail_inval("the stream's first sample has none in front: front must be NULL at pos 0");
    if (n == 0) return IQA_OK;
    if (!inc) return fail_inval("inc must name IQA_KEYING_BAUDS clock steps");
    if (!theta_dev || !cs_dev || !gate_dev || !rows_dev) return fail_inval("NULL device pointer");
    KeyingArgs g;
    g.theta = static_cast<const float *>(theta_dev);
    g.front = static_cast<const float *>(front_dev);
    g.gate = static_cast<const unsigned char *>(gate_dev);
    g.cs = static_cast<const int *>(cs_dev);
    g.rows = static_cast<int *>(rows_dev);
    g.n = n;
    g.pos = pos;
    g.delay = delay;
    g.hop = hop;
    g.F = F;
    g.slice_raw = static_cast<long long>(hop) * T;
    g.D = D;
    g.T = T;
    g.S = S;
    g.c = c;
    for (int k = 0; k < KY_BAUDS; ++k) g.inc[k] = static_cast<unsigned>(inc[k]);
    hipLaunchKernelGGL(k_keying, dim3(static_cast<unsigned>(iqa_keying_windows(pos, n))), dim3(SB_THREADS), 0, as_stream(stream), g);
    return check_launch("k_keying");
}
