// tones.hip -- CTCSS tones and DTMF digits beside the NFM demodulator, for gfx950.
//
// Specification (fs the channel rate, theta the discriminator output, all indices absolute, everything zero in front of
// the stream; R = floor(fs / 8000), fd = fs / R; a bank is (N, H, tones) with taps c_f[k] = rint(256 cos(2 pi f k / fd)),
// s_f[k] likewise with sin, int16, k < N):
//   t[n]   = rint(theta[n] 4096)                                         (int32, half-even; integers from here on)
//   u[m]   = floor(sum_{j<2R-1} min(j+1, 2R-1-j) t[(m+1)R - 1 - j] / R)  (int32 sum: R^2 12 868 < 2^26; floor division)
//   frame i of a bank = u[iH .. iH+N-1];  I_f = sum_k c_f[k] u[iH+k], Q_f with s_f     (int64: |I| < 2^41)
//   E_f    = (I_f >> 12)^2 + (Q_f >> 12)^2,  P = sum_k u[iH+k]^2                       (int64, arithmetic shifts)
//   CTCSS code: k* = lowest index of the maximum of the 50 energies, med = their 25th smallest;
//               k* iff (E[k*] >> 6) >= med and E[k*] >= 2^16, else 255
//   DTMF code:  r, c = lowest indices of the row (0..3) and column (4..7) maxima, r2, c2 the largest of the others in each
//               group; 4r + c iff E_r >= 8 r2, E_c >= 8 c2, E_c <= 16 E_r, E_r <= 16 E_c, E_r >= 2^16, E_c >= 2^16 and
//               1024 (E_r + E_c) >= N P, else 255
//
// k_tones_decimate: a workgroup owns MB consecutive outputs (MB R <= 8192 input samples).  It quantises those samples and
// the R - 1 in front of them into LDS (from the carried history where they lie in front of the block), stores t, and one
// thread per output forms the weighted sum.  The tiles are laid on the absolute index, so that a block of any length (a
// single sample; one that completes no output) is handled by the same code: the last tile also takes the samples behind
// the last completed output.
// k_tones_bank: one workgroup per frame; the frame sits in LDS; the four waves split the tones (and the power sum, where
// it is asked for), lanes stride over k, every lane adds in int64 and the wave total is an integer butterfly.
// k_tones_decide: one thread per frame; the median by rank counting (no sort, no per-thread array).
#include "common.h"

namespace iqa {

constexpr int TN_THREADS = 256;
constexpr int TN_WAVES = TN_THREADS / kWave;
constexpr int TN_SPAN = 8192;  // most input samples a decimator tile owns
constexpr float TN_THETA_SCALE = 4096.0f;
constexpr int TN_CTCSS = IQA_TONES_CTCSS, TN_DTMF = IQA_TONES_DTMF;
constexpr long long TN_FLOOR = 1LL << 16;  // least energy of a hit

__host__ __device__ constexpr int tn_tile_outputs(int R) { return TN_SPAN / R < TN_THREADS ? TN_SPAN / R : TN_THREADS; }

struct TonesDecArgs {
    const float *theta;  // [n]
    const int *hist;     // [2R - 2]: t in front of theta[0]; NULL = zeros
    int *t_out;          // [n]
    int *u_out;          // [m_end - m_first]
    long long n, pos;    // pos: the absolute index of theta[0]
    long long m_first, m_end;  // the outputs this block completes: pos / R .. (pos + n) / R - 1
    int R, MB;
};

__global__ __launch_bounds__(TN_THREADS) void k_tones_decimate(TonesDecArgs g)
{
    extern __shared__ int s_t[];  // s_t[i] = t at absolute index S - (R - 1) + i, i = 0 .. R - 1 + MB R - 1
    const int tid = threadIdx.x, R = g.R, halo = R - 1, span = g.MB * R, back = 2 * R - 2;
    const long long m0 = g.m_first + static_cast<long long>(blockIdx.x) * g.MB;
    const long long S = m0 * R, end = g.pos + g.n;
    for (int i = tid; i < halo + span; i += TN_THREADS) {
        const long long x = S - halo + i;
        int v = 0;
        if (x >= g.pos) {
            if (x < end) {
                v = __float2int_rn(g.theta[x - g.pos] * TN_THETA_SCALE);
                if (i >= halo) g.t_out[x - g.pos] = v;  // (x >= S: every sample of the block lies in exactly one tile's own span)
            }
        } else if (g.hist && x >= g.pos - back) {
            v = g.hist[x - (g.pos - back)];  // (S - halo >= pos - back: the history is exactly what a tile can reach)
        }
        s_t[i] = v;
    }
    __syncthreads();
    const long long m = m0 + tid;
    if (tid >= g.MB || m >= g.m_end) return;
    // output m reads absolute (m+1)R - 1 - j, j = 0 .. 2R - 2: LDS index tid R + q with q = 2R - 2 - j, and w is symmetric
    const int *p = s_t + tid * R;
    int sum = 0;
    for (int q = 0; q <= back; ++q) sum += min(q + 1, 2 * R - 1 - q) * p[q];
    int quot = sum / R;
    if (sum % R != 0 && sum < 0) --quot;  // floor, not truncation
    g.u_out[m - g.m_first] = quot;
}

struct TonesBankArgs {
    const int *u;        // [M]
    const short *taps;   // [ntones][2][N]: c_f, s_f
    long long *E;        // [F][ntones]
    long long *P;        // [F] or NULL
    int N, H, ntones;
};

__device__ __forceinline__ long long tn_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__global__ __launch_bounds__(TN_THREADS) void k_tones_bank(TonesBankArgs g)
{
    extern __shared__ int s_u[];  // [N]: the frame
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, N = g.N;
    const long long frame = blockIdx.x;
    const int *u = g.u + frame * g.H;
    for (int k = tid; k < N; k += TN_THREADS) s_u[k] = u[k];
    __syncthreads();
    const int jobs = g.ntones + (g.P ? 1 : 0);  // (the power sum is one more job)
    for (int f = wave; f < jobs; f += TN_WAVES) {
        long long a = 0, b = 0;
        if (f < g.ntones) {
            const short *c = g.taps + static_cast<long long>(2 * f) * N, *s = c + N;
            for (int k = lane; k < N; k += kWave) {
                const int v = s_u[k];
                a += static_cast<long long>(c[k]) * v;
                b += static_cast<long long>(s[k]) * v;
            }
        } else {
            for (int k = lane; k < N; k += kWave) {
                const int v = s_u[k];
                a += static_cast<long long>(v) * v;
            }
        }
        a = tn_wave_sum(a);
        b = tn_wave_sum(b);
        if (lane != 0) continue;
        if (f < g.ntones) {
            const long long i = a >> 12, q = b >> 12;
            g.E[frame * g.ntones + f] = i * i + q * q;
        } else {
            g.P[frame] = a;
        }
    }
}

struct TonesDecideArgs {
    const long long *Ec;  // [Fc][50]
    const long long *Ed;  // [Fd][8]
    const long long *P;   // [Fd]
    unsigned char *ctcss; // [Fc]
    unsigned char *dtmf;  // [Fd]
    long long Fc, Fd;
    int Nd;
};

// The largest of four and its lowest index; second: the largest of the other three (a tie for the maximum counts).
__device__ __forceinline__ void tn_group(const long long *e, int &at, long long &best, long long &second)
{
    at = 0, best = e[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (e[k] > best) best = e[k], at = k;
    second = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k != at && e[k] > second) second = e[k];
}

__global__ __launch_bounds__(TN_THREADS) void k_tones_decide(TonesDecideArgs g)
{
    const long long i = static_cast<long long>(blockIdx.x) * TN_THREADS + threadIdx.x;
    if (i < g.Fc) {
        const long long *e = g.Ec + i * TN_CTCSS;
        long long best = e[0], med = 0;
        int at = 0;
        for (int k = 1; k < TN_CTCSS; ++k)
            if (e[k] > best) best = e[k], at = k;
        for (int j = 0; j < TN_CTCSS; ++j) {  // sorted[24] is the value with at most 24 below it and more than 24 at or below it
            const long long ej = e[j];
            int less = 0, leq = 0;
            for (int k = 0; k < TN_CTCSS; ++k) less += e[k] < ej ? 1 : 0, leq += e[k] <= ej ? 1 : 0;
            if (less <= 24 && leq > 24) med = ej;
        }
        const bool hit = (best >> 6) >= med && best >= TN_FLOOR;
        g.ctcss[i] = static_cast<unsigned char>(hit ? at : IQA_TONES_NONE);
    }
    if (i < g.Fd) {
        long long e[TN_DTMF];
#pragma unroll
        for (int k = 0; k < TN_DTMF; ++k) e[k] = g.Ed[i * TN_DTMF + k];
        int r, c;
        long long er, ec, r2, c2;
        tn_group(e, r, er, r2);
        tn_group(e + 4, c, ec, c2);
        const bool hit = er >= 8 * r2 && ec >= 8 * c2 && ec <= 16 * er && er <= 16 * ec && er >= TN_FLOOR && ec >= TN_FLOOR &&
                         1024 * (er + ec) >= g.Nd * g.P[i];
        g.dtmf[i] = static_cast<unsigned char>(hit ? 4 * r + c : IQA_TONES_NONE);
    }
}

static_assert((TN_SPAN + IQA_TONES_MAX_R - 1) * 4 <= 64 * 1024, "a decimator tile must fit the default LDS allowance");
static_assert(IQA_TONES_MAX_FRAME * 4 <= 64 * 1024, "a frame must fit the default LDS allowance");
static_assert(12868LL * IQA_TONES_MAX_R * IQA_TONES_MAX_R < (1LL << 31), "the decimator sum stays inside int32");
static_assert(tn_tile_outputs(IQA_TONES_MAX_R) >= 1 && tn_tile_outputs(1) == TN_THREADS, "one thread per output of a tile");

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_tones_decimate(const void *theta_dev, int64_t n, int64_t pos, const void *hist_dev, int32_t R, void *t_out_dev,
                                  void *u_out_dev, void *stream)
{
    if (n < 0 || pos < 0) return fail_inval("negative length or position");
    if (R < 1 || R > IQA_TONES_MAX_R) return fail_inval("R must be 1 .. IQA_TONES_MAX_R");
    if (n == 0) return IQA_OK;
    if (n > (1LL << 40) || pos > (1LL << 50)) return fail_inval("length or position out of range");
    TonesDecArgs g;
    g.m_first = pos / R;
    g.m_end = (pos + n) / R;
    if (!theta_dev || !t_out_dev || (g.m_end > g.m_first && !u_out_dev)) return fail_inval("NULL device pointer");
    g.theta = static_cast<const float *>(theta_dev);
    g.hist = R > 1 ? static_cast<const int *>(hist_dev) : nullptr;
    g.t_out = static_cast<int *>(t_out_dev);
    g.u_out = static_cast<int *>(u_out_dev);
    g.n = n;
    g.pos = pos;
    g.R = R;
    g.MB = tn_tile_outputs(R);
    const int span = g.MB * R;
    const size_t lds = static_cast<size_t>(R - 1 + span) * sizeof(int);
    hipLaunchKernelGGL(k_tones_decimate, grid1d(pos + n - g.m_first * R, span), dim3(TN_THREADS), lds, as_stream(stream), g);
    return check_launch("k_tones_decimate");
}

extern "C" int iqa_tones_bank(const void *u_dev, int64_t m, int32_t frame, int32_t hop, int32_t ntones, const void *taps_dev,
                              void *e_out_dev, void *p_out_dev, void *stream)
{
    if (m < 0) return fail_inval("negative length");
    if (frame < 1 || frame > IQA_TONES_MAX_FRAME) return fail_inval("frame must be 1 .. IQA_TONES_MAX_FRAME");
    if (hop < 1 || hop > frame) return fail_inval("hop must be 1 .. frame");
    if (ntones < 1 || ntones > IQA_TONES_MAX_TONES) return fail_inval("ntones must be 1 .. IQA_TONES_MAX_TONES");
    if (m < frame) return IQA_OK;  // no frame: nothing is written
    if (!u_dev || !taps_dev || !e_out_dev) return fail_inval("NULL device pointer");
    const int64_t frames = (m - frame) / hop + 1;
    if (frames > (1LL << 30)) return fail_inval("length out of range");
    TonesBankArgs g;
    g.u = static_cast<const int *>(u_dev);
    g.taps = static_cast<const short *>(taps_dev);
    g.E = static_cast<long long *>(e_out_dev);
    g.P = static_cast<long long *>(p_out_dev);
    g.N = frame;
    g.H = hop;
    g.ntones = ntones;
    hipLaunchKernelGGL(k_tones_bank, dim3(static_cast<unsigned>(frames)), dim3(TN_THREADS), static_cast<size_t>(frame) * sizeof(int),
                       as_stream(stream), g);
    return check_launch("k_tones_bank");
}

extern "C" int iqa_tones_decide(const void *e_ctcss_dev, int64_t frames_ctcss, const void *e_dtmf_dev, const void *p_dev,
                                int64_t frames_dtmf, int32_t frame_dtmf, void *ctcss_out_dev, void *dtmf_out_dev, void *stream)
{
    if (frames_ctcss < 0 || frames_dtmf < 0) return fail_inval("negative length");
    if (frame_dtmf < 1 || frame_dtmf > IQA_TONES_MAX_FRAME) return fail_inval("frame must be 1 .. IQA_TONES_MAX_FRAME");
    if (frames_ctcss > (1LL << 30) || frames_dtmf > (1LL << 30)) return fail_inval("length out of range");
    if (frames_ctcss > 0 && (!e_ctcss_dev || !ctcss_out_dev)) return fail_inval("NULL device pointer");
    if (frames_dtmf > 0 && (!e_dtmf_dev || !p_dev || !dtmf_out_dev)) return fail_inval("NULL device pointer");
    const int64_t most = frames_ctcss > frames_dtmf ? frames_ctcss : frames_dtmf;
    if (most == 0) return IQA_OK;
    TonesDecideArgs g;
    g.Ec = static_cast<const long long *>(e_ctcss_dev);
    g.Ed = static_cast<const long long *>(e_dtmf_dev);
    g.P = static_cast<const long long *>(p_dev);
    g.ctcss = static_cast<unsigned char *>(ctcss_out_dev);
    g.dtmf = static_cast<unsigned char *>(dtmf_out_dev);
    g.Fc = frames_ctcss;
    g.Fd = frames_dtmf;
    g.Nd = frame_dtmf;
    hipLaunchKernelGGL(k_tones_decide, grid1d(most, TN_THREADS), dim3(TN_THREADS), 0, as_stream(stream), g);
    return check_launch("k_tones_decide");
}
