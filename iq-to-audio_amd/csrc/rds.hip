// rds.hip -- RDS (57 kHz subcarrier) demodulation beside the wideband FM stereo matrix, for gfx950.
//
// Specification (float64 statement; N, D = (N-1)/2, h_p, m, md[n] = m[n-D], p = h_p * m, u = p / |p| are section 10's;
// R = round(fs / 19 000), h_r the antisymmetric matched filter of 2M+1 taps, f = 57 000 / fs, all indices absolute):
//   y0[j]  = sum_k h_r[k] md[jR-k] exp(-j 2 pi frac(f (jR-k)))
//   y[j]   = y0[j] exp(+j 2 pi frac(f jR)) conj(u[jR])^3
//   dev[j] = angle(u[jR] conj(u[(j-1)R]) exp(-j 2 pi 19 000 R / fs)),  dev[0] = 0,  q[j] = rint(dev[j] / (2 pi) 2^44)
//   Phi[j] = sum_{i<=j} q[i]   (int64, exact),   psi[j] = (j 19 000 R / fs + Phi[j] 2^-44) / 16
//   Z = sum_{j>=j0} |y[j]|^2 exp(-j 2 pi psi[j]),  tau = -arg Z / (2 pi),  r = psi - tau
//   s[k] = y[j-1] + (y[j] - y[j-1]) (k - r[j-1]) / (r[j] - r[j-1])  wherever k = floor(r[j]) > floor(r[j-1])
//   d[k] = Re(s[k] conj(s[k-1])) < 0;  W[i] = bits i .. i+25, S[i] = crc10(W[i] >> 10) xor (W[i] & 0x3FF)
//
// k_rds_baseband: one workgroup owns `tile` consecutive decimated outputs.  It stages, in LDS, the composite its pilot
// instants need and the mixed composite md[i] exp(-j 2 pi frac(f i)) its matched filter needs (each mixed sample is made
// once per tile, its phase from the absolute index in float64), then one WAVE computes one output at a time: the 64 lanes
// take the tap pairs k = lane, lane + 64, ... (consecutive LDS addresses, consecutive taps), each lane in ascending k with
// one float32 fmaf per pair and component, and the 64 partial sums are added by the xor butterfly.  The order of every sum
// is fixed by k alone, so a value depends neither on the tile size, nor on the tile, nor on where the caller cuts blocks.
#include "common.h"

#include <cmath>

namespace iqa {

constexpr int RDS_THREADS = 256;
constexpr int RDS_WAVES = RDS_THREADS / kWave;
constexpr int RDS_MAX_TILE = 64;
constexpr int RDS_MIN_TILE = 8;
constexpr int RDS_LDS_LIMIT = 64 * 1024 - 64;
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct RdsArgs {
    const float *mf_taps;     // [M]: h_r[0..M-1] (h_r[2M-k] = -h_r[k], h_r[M] = 0)
    const float *pilot_taps;  // [2 (D+1)]: Re h_p[0..D], Im h_p[0..D]
    const float *theta;       // [n]
    const float *hist;        // [2M + 2(N-1)]: the discriminator values in front of theta[0]; NULL = zeros
    float2 *y_out;            // [nj]
    long long *q_out;         // [nj]
    long long pos;            // absolute index of theta[0]
    long long n;
    long long j_first;        // ceil(pos / R)
    long long nj;
    double f_mix;             // 57 000 / fs, cycles per sample
    double rot_re, rot_im;    // exp(-j 2 pi 19 000 R / fs)
    int ntaps, half, decim, tile;
    float scale;
};

// floats of dynamic LDS: pilot window (tile R + N, + 1 of alignment) + mixed window 2 ((tile - 1) R + 1 + 2M) + pilot values 2 (tile + 1)
__host__ __device__ constexpr long long rds_lds_floats(int ntaps, int half, int decim, int tile)
{
    return static_cast<long long>(tile) * decim + ntaps + 1 + 2LL * ((tile - 1LL) * decim + 1 + 2LL * half) + 2LL * (tile + 1);
}

// the largest tile of 64, 32, 16, 8 outputs whose windows fit the LDS allowance; 0 if none does
static int rds_pick_tile(int ntaps, int half, int decim)
{
    for (int t = RDS_MAX_TILE; t >= RDS_MIN_TILE; t >>= 1)
        if (rds_lds_floats(ntaps, half, decim, t) * 4 <= RDS_LDS_LIMIT) return t;
    return 0;
}

__global__ __launch_bounds__(RDS_THREADS) void k_rds_baseband(RdsArgs g)
{
    extern __shared__ float s_mem[];
    const int N = g.ntaps, D = (N - 1) / 2, H = N - 1, M = g.half, R = g.decim, T = g.tile;
    const int HL = 2 * M + 2 * H;             // length of the carried history
    const int nx = T * R + N;                 // s_x[i] = m at absolute index nA - R - H + i
    const int nc = (T - 1) * R + 1 + 2 * M;   // s_c[i] = mixed md at absolute md index nA - 2M + i
    float *s_x = s_mem;
    float2 *s_c = reinterpret_cast<float2 *>(s_x + nx + (nx & 1));  // (8-byte aligned)
    float2 *s_p = s_c + nc;                   // s_p[e] = p at instant nA + (e - 1) R, e = 0 .. T
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long jA = g.j_first + static_cast<long long>(blockIdx.x) * T;
    const long long nA = jA * R;
    const long long left = g.j_first + g.nj - jA;
    const int Tt = left < T ? static_cast<int>(left) : T;  // outputs of this tile

    // m at absolute index a (0 in front of the stream and behind the block; the block's last instant is inside it)
    auto composite = [&](long long a) -> float {
        const long long rel = a - g.pos;
        float v = 0.f;
        if (rel >= 0) {
            if (rel < g.n) v = g.theta[rel];
        } else if (g.hist != nullptr && rel >= -static_cast<long long>(HL)) {
            v = g.hist[HL + rel];
        }
        return v * g.scale;
    };

    for (int i = tid; i < nx; i += RDS_THREADS) s_x[i] = composite(nA - R - H + i);
    for (int i = tid; i < nc; i += RDS_THREADS) {
        const long long a = nA - 2 * M + i;  // md index; md[a] = m[a - D]
        const float v = composite(a - D);
        double ph = __dmul_rn(g.f_mix, static_cast<double>(a));
        ph -= floor(ph);
        float sn, cs;
        sincospif(2.0f * static_cast<float>(ph), &sn, &cs);
        s_c[i] = make_float2(v * cs, -v * sn);
    }
    __syncthreads();

    // pilot at the tile's instants and the one in front of them: x[i] = m[P - H + i], P = nA + (e - 1) R
    const float *hr = g.pilot_taps, *hi = g.pilot_taps + (D + 1);
    for (int e = wave; e <= Tt; e += RDS_WAVES) {
        const float *x = s_x + e * R;
        float pr = 0.f, pi = 0.f;
        for (int k = lane; k < D; k += kWave) {
            const float x1 = x[H - k], x2 = x[k];  // taps k and N-1-k
            pr = fmaf(hr[k], x1 + x2, pr);
            pi = fmaf(hi[k], x1 - x2, pi);
        }
        pr = wave_sum(pr);
        pi = wave_sum(pi);
        pr = fmaf(hr[D], x[D], pr);
        if (lane == 0) s_p[e] = make_float2(pr, pi);
    }

    // matched filter: output t at md index nA + t R, centre of its window at s_c[t R + M]
    float yr = 0.f, yi = 0.f;  // lane t of a wave keeps the wave's t-th result (t = wave + 4 lane)
    for (int t = wave; t < Tt; t += RDS_WAVES) {
        const float2 *hiw = s_c + t * R + 2 * M;  // hiw[-k] = c[n - k]
        const float2 *low = s_c + t * R;          // low[k] = c[n - 2M + k]
        float ar = 0.f, ai = 0.f;
        for (int k = lane; k < M; k += kWave) {
            const float h = g.mf_taps[k];
            const float2 c1 = hiw[-k], c2 = low[k];
            ar = fmaf(h, c1.x - c2.x, ar);
            ai = fmaf(h, c1.y - c2.y, ai);
        }
        ar = wave_sum(ar);
        ai = wave_sum(ai);
        if (lane == t / RDS_WAVES) {
            yr = ar;
            yi = ai;
        }
    }
    __syncthreads();

    // y and q of output t = wave + 4 lane, in float64 from the float32 sums
    const int t = wave + RDS_WAVES * lane;
    if (t < Tt) {
        const long long j = jA + t;
        const float2 p1 = s_p[t + 1], p0 = s_p[t];
        const double m1 = sqrt(static_cast<double>(p1.x) * p1.x + static_cast<double>(p1.y) * p1.y);
        const double m0 = sqrt(static_cast<double>(p0.x) * p0.x + static_cast<double>(p0.y) * p0.y);
        const double ur = m1 < 1e-12 ? 0.0 : p1.x / m1, ui = m1 < 1e-12 ? 0.0 : p1.y / m1;
        const double vr = m0 < 1e-12 ? 0.0 : p0.x / m0, vi = m0 < 1e-12 ? 0.0 : p0.y / m0;
        // u conj(v) rot
        const double wr = ur * vr + ui * vi, wi = ui * vr - ur * vi;
        const double zr = wr * g.rot_re - wi * g.rot_im, zi = wr * g.rot_im + wi * g.rot_re;
        const double dev = (j == 0 || (zr == 0.0 && zi == 0.0)) ? 0.0 : atan2(zi, zr);
        g.q_out[j - g.j_first] = static_cast<long long>(rint(dev / kTwoPi * 17592186044416.0));  // 2^44
        // y0 exp(+j 2 pi frac(f n)) conj(u)^3
        double ph = __dmul_rn(g.f_mix, static_cast<double>(j * R));
        ph -= floor(ph);
        double sn, cs;
        sincospi(2.0 * ph, &sn, &cs);
        const double u2r = ur * ur - ui * ui, u2i = 2.0 * ur * ui;
        const double u3r = u2r * ur - u2i * ui, u3i = u2r * ui + u2i * ur;
        const double er = cs * u3r + sn * u3i, ei = sn * u3r - cs * u3i;  // exp(+j phi) conj(u^3)
        g.y_out[j - g.j_first] = make_float2(static_cast<float>(yr * er - yi * ei), static_cast<float>(yr * ei + yi * er));
    }
}

constexpr int RDS_CLOCK_CHUNK = 4096;  // values per workgroup of the clock's scan

// sum over the 256 threads of a workgroup, in every thread (integers: exact in any order)
__device__ __forceinline__ long long rds_block_sum(long long v, long long *s_w)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = v;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// reduce: sums[c] = the sum of chunk c of q
__global__ __launch_bounds__(RDS_THREADS) void k_rds_clock_reduce(const long long *q, long long n, long long *sums)
{
    __shared__ long long s_w[RDS_WAVES];
    const long long base = static_cast<long long>(blockIdx.x) * RDS_CLOCK_CHUNK;
    long long v = 0;
#pragma unroll
    for (int r = 0; r < RDS_CLOCK_CHUNK / RDS_THREADS; ++r) {
        const long long i = base + threadIdx.x + r * RDS_THREADS;
        if (i < n) v += q[i];
    }
    v = rds_block_sum(v, s_w);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

// apply: chunk c starts from *total + sums[0] + .. + sums[c-1] and scans its values 256 at a time; also psi
__global__ __launch_bounds__(RDS_THREADS) void k_rds_clock_apply(const long long *q, long long n, long long j_first, double step,
                                                               const long long *total, const long long *sums, long long *phi,
                                                               double *psi)
{
    __shared__ long long s_w[RDS_WAVES];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    long long front = 0;
    for (int c = tid; c < static_cast<int>(blockIdx.x); c += RDS_THREADS) front += sums[c];
    long long carry = *total + rds_block_sum(front, s_w);
    const long long base = static_cast<long long>(blockIdx.x) * RDS_CLOCK_CHUNK;
    for (int r = 0; r < RDS_CLOCK_CHUNK / RDS_THREADS; ++r) {
        const long long i = base + tid + r * RDS_THREADS;
        long long v = i < n ? q[i] : 0;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const long long up = __shfl_up(v, o, kWave);
            if (lane >= o) v += up;
        }
        __syncthreads();
        if (lane == kWave - 1) s_w[wave] = v;
        __syncthreads();
        long long before = carry, all = carry;
#pragma unroll
        for (int w = 0; w < RDS_WAVES; ++w) {
            if (w < wave) before += s_w[w];
            all += s_w[w];
        }
        if (i < n) {
            const long long f = before + v;
            phi[i] = f;
            {
                // three float64 operations, each rounded once: no contraction of j step + b into one fma (__dmul_rn and
                // __dadd_rn are a plain product and sum to this compiler, and fuse)
#pragma clang fp contract(off)
                const double a = static_cast<double>(j_first + i) * step;
                const double b = static_cast<double>(f) * 5.6843418860808015e-14;  // 2^-44
                psi[i] = (a + b) * 0.0625;
            }
        }
        carry = all;
    }
}

// carry: *total += the sum of all chunks (after the apply pass has read it)
__global__ __launch_bounds__(RDS_THREADS) void k_rds_clock_carry(const long long *sums, long long chunks, long long *total)
{
    __shared__ long long s_w[RDS_WAVES];
    long long v = 0;
    for (long long c = threadIdx.x; c < chunks; c += RDS_THREADS) v += sums[c];
    v = rds_block_sum(v, s_w);
    if (threadIdx.x == 0) *total += v;
}

constexpr int RDS_TIMING_TILE = 1024;

// per tile of 1024 absolute indices: sum |y|^2 cos, -sum |y|^2 sin, sum |y|^2 over j >= j0, float64, fixed order
__global__ __launch_bounds__(RDS_THREADS) void k_rds_timing_tiles(const float2 *y, const double *psi, long long n, long long j0,
                                                                double *partials)
{
    __shared__ double s_red[3][RDS_WAVES];
    const int tid = threadIdx.x;
    double zr = 0.0, zi = 0.0, pw = 0.0;
#pragma unroll
    for (int r = 0; r < RDS_TIMING_TILE / RDS_THREADS; ++r) {
        const long long j = static_cast<long long>(blockIdx.x) * RDS_TIMING_TILE + tid + r * RDS_THREADS;
        if (j < n && j >= j0) {
            const float2 v = y[j];
            const double e = static_cast<double>(v.x) * v.x + static_cast<double>(v.y) * v.y;
            double ph = psi[j];
            ph -= floor(ph);
            double sn, cs;
            sincospi(2.0 * ph, &sn, &cs);
            zr += e * cs;
            zi -= e * sn;
            pw += e;
        }
    }
    zr = wave_sum(zr);
    zi = wave_sum(zi);
    pw = wave_sum(pw);
    if ((tid & (kWave - 1)) == 0) {
        s_red[0][tid / kWave] = zr;
        s_red[1][tid / kWave] = zi;
        s_red[2][tid / kWave] = pw;
    }
    __syncthreads();
    if (tid < 3) partials[3LL * blockIdx.x + tid] = (s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]);
}

// out[c] = sum of partials[3 t + c] over the tiles: thread i adds tiles i, i + 256, ... in that order, then the butterfly
__global__ __launch_bounds__(RDS_THREADS) void k_rds_timing_total(const double *partials, long long tiles, double *out)
{
    __shared__ double s_red[3][RDS_WAVES];
    const int tid = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long t = tid; t < tiles; t += RDS_THREADS)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += partials[3 * t + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        acc[c] = wave_sum(acc[c]);
        if ((tid & (kWave - 1)) == 0) s_red[c][tid / kWave] = acc[c];
    }
    __syncthreads();
    if (tid < 3) out[tid] = (s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]);
}

// the scatter: a symbol wherever floor(psi - tau) steps up, written at index k - k_first
__global__ __launch_bounds__(256) void k_rds_symbols(const float2 *y, const double *psi, long long n, long long j0, double tau,
                                                   long long k_first, long long nsym, float2 *sym)
{
    const long long j = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (j >= n || j <= j0) return;
    const double r1 = __dadd_rn(psi[j], -tau), r0 = __dadd_rn(psi[j - 1], -tau);
    const double k = floor(r1);
    if (!(k > floor(r0))) return;
    const long long o = static_cast<long long>(k) - k_first;
    if (o < 0 || o >= nsym) return;
    const double fr = (k - r0) / (r1 - r0);
    const float2 a = y[j - 1], b = y[j];
    sym[o] = make_float2(static_cast<float>(a.x + (static_cast<double>(b.x) - a.x) * fr),
                         static_cast<float>(a.y + (static_cast<double>(b.y) - a.y) * fr));
}

// bits[i] = Re(s[i+1] conj(s[i])) < 0
__global__ __launch_bounds__(256) void k_rds_bits(const float2 *sym, long long nsym, unsigned char *bits)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i + 1 >= nsym) return;
    const float2 a = sym[i], b = sym[i + 1];
    const double re = static_cast<double>(b.x) * a.x + static_cast<double>(b.y) * a.y;
    bits[i] = re < 0.0 ? 1 : 0;
}

// one thread per bit offset: the 26-bit word (first bit most significant) and its syndrome
__global__ __launch_bounds__(256) void k_rds_syndromes(const unsigned char *bits, long long nbits, unsigned int *words,
                                                     unsigned short *synd)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i + 26 > nbits) return;
    unsigned int w = 0;
#pragma unroll
    for (int b = 0; b < 26; ++b) w = (w << 1) | (bits[i + b] & 1u);
    unsigned int r = w & ~0x3FFu;  // (W >> 10) x^10
#pragma unroll
    for (int b = 25; b >= 10; --b)
        if ((r >> b) & 1u) r ^= 0x5B9u << (b - 10);
    words[i] = w;
    synd[i] = static_cast<unsigned short>((r ^ w) & 0x3FFu);
}

static_assert(RDS_WAVES == 4, "the reductions add four waves");
static_assert(rds_lds_floats(IQA_WFM_MAX_TAPS, IQA_RDS_MAX_HALF, IQA_RDS_MAX_DECIM, RDS_MIN_TILE) * 4 <= RDS_LDS_LIMIT,
              "the largest rate the stereo matrix admits must fit the default LDS allowance");

}  // namespace iqa

using namespace iqa;

extern "C" int64_t iqa_rds_hist_len(int32_t ntaps, int32_t half_taps)
{
    if (ntaps < 3 || half_taps < 1) return 0;
    return 2LL * half_taps + 2LL * (ntaps - 1);
}

extern "C" int64_t iqa_rds_outputs(int64_t pos, int64_t n, int32_t decim)
{
    if (pos < 0 || n <= 0 || decim < 1) return 0;
    return (pos + n + decim - 1) / decim - (pos + decim - 1) / decim;
}

extern "C" int64_t iqa_rds_lds_bytes(int32_t ntaps, int32_t half_taps, int32_t decim)
{
    if (ntaps < 3 || half_taps < 1 || decim < 1) return 0;
    const int t = rds_pick_tile(ntaps, half_taps, decim);
    return t ? rds_lds_floats(ntaps, half_taps, decim, t) * 4 : 0;
}

extern "C" int iqa_rds_baseband(int32_t ntaps, const void *pilot_taps_dev, int32_t half_taps, const void *mf_taps_dev, int32_t decim,
                                float m_scale, double f_mix, double clock_step, const void *theta_dev, int64_t n, int64_t pos,
                                const void *hist_dev, void *y_out_dev, void *q_out_dev, void *stream)
{
    if (ntaps < 3 || ntaps > IQA_WFM_MAX_TAPS || (ntaps & 1) == 0) return fail_inval("ntaps must be odd, 3 .. IQA_WFM_MAX_TAPS");
    if (half_taps < 1 || half_taps > IQA_RDS_MAX_HALF) return fail_inval("half_taps must be 1 .. IQA_RDS_MAX_HALF");
    if (decim < 1 || decim > IQA_RDS_MAX_DECIM) return fail_inval("decimation must be 1 .. IQA_RDS_MAX_DECIM");
    if (n < 0) return fail_inval("negative length");
    if (pos < 0) return fail_inval("negative stream position");
    if (!std::isfinite(m_scale)) return fail_inval("composite scale is not finite");
    if (!std::isfinite(f_mix) || !std::isfinite(clock_step)) return fail_inval("mixer or clock step is not finite");
    if (n > (1LL << 40) || pos > (1LL << 44)) return fail_inval("length out of range");
    const int tile = rds_pick_tile(ntaps, half_taps, decim);
    if (tile == 0) return fail_inval("the filter windows do not fit the LDS (ntaps, half_taps, decimation too large together)");
    const int64_t nj = iqa_rds_outputs(pos, n, decim);
    if (nj == 0) return IQA_OK;
    if (!pilot_taps_dev || !mf_taps_dev || !theta_dev || !y_out_dev || !q_out_dev) return fail_inval("NULL device pointer");
    RdsArgs g;
    g.mf_taps = static_cast<const float *>(mf_taps_dev);
    g.pilot_taps = static_cast<const float *>(pilot_taps_dev);
    g.theta = static_cast<const float *>(theta_dev);
    g.hist = static_cast<const float *>(hist_dev);
    g.y_out = static_cast<float2 *>(y_out_dev);
    g.q_out = static_cast<long long *>(q_out_dev);
    g.pos = pos;
    g.n = n;
    g.j_first = (pos + decim - 1) / decim;
    g.nj = nj;
    g.f_mix = f_mix;
    g.rot_re = std::cos(kTwoPi * clock_step);
    g.rot_im = -std::sin(kTwoPi * clock_step);
    g.ntaps = ntaps;
    g.half = half_taps;
    g.decim = decim;
    g.tile = tile;
    g.scale = m_scale;
    const size_t lds = static_cast<size_t>(rds_lds_floats(ntaps, half_taps, decim, tile)) * sizeof(float);
    hipLaunchKernelGGL(k_rds_baseband, dim3(static_cast<unsigned>((nj + tile - 1) / tile)), dim3(RDS_THREADS), lds, as_stream(stream), g);
    return check_launch("k_rds_baseband");
}

extern "C" int64_t iqa_rds_clock_chunks(int64_t n) { return n <= 0 ? 0 : (n + RDS_CLOCK_CHUNK - 1) / RDS_CLOCK_CHUNK; }

extern "C" int iqa_rds_clock(const void *q_dev, int64_t n, int64_t j_first, double clock_step, void *total_dev, void *work_dev,
                             void *phi_out_dev, void *psi_out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (j_first < 0) return fail_inval("negative output index");
    if (!std::isfinite(clock_step)) return fail_inval("clock step is not finite");
    if (n == 0) return IQA_OK;
    if (!q_dev || !total_dev || !work_dev || !phi_out_dev || !psi_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    const long long chunks = iqa_rds_clock_chunks(n);
    const long long *q = static_cast<const long long *>(q_dev);
    long long *sums = static_cast<long long *>(work_dev), *total = static_cast<long long *>(total_dev);
    hipLaunchKernelGGL(k_rds_clock_reduce, dim3(static_cast<unsigned>(chunks)), dim3(RDS_THREADS), 0, as_stream(stream), q, (long long)n, sums);
    hipLaunchKernelGGL(k_rds_clock_apply, dim3(static_cast<unsigned>(chunks)), dim3(RDS_THREADS), 0, as_stream(stream), q, (long long)n,
                       (long long)j_first, clock_step, total, sums, static_cast<long long *>(phi_out_dev),
                       static_cast<double *>(psi_out_dev));
    hipLaunchKernelGGL(k_rds_clock_carry, dim3(1), dim3(RDS_THREADS), 0, as_stream(stream), sums, chunks, total);
    return check_launch("k_rds_clock");
}

extern "C" int64_t iqa_rds_timing_partials(int64_t n) { return n <= 0 ? 0 : (n + RDS_TIMING_TILE - 1) / RDS_TIMING_TILE; }

extern "C" int iqa_rds_timing(const void *y_dev, const void *psi_dev, int64_t n, int64_t j0, void *partials_dev, void *out_dev,
                              void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (j0 < 0) return fail_inval("negative first index");
    if (!out_dev) return fail_inval("NULL device pointer");
    if (n > 0 && (!y_dev || !psi_dev || !partials_dev)) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    const int64_t tiles = iqa_rds_timing_partials(n);
    if (tiles)
        hipLaunchKernelGGL(k_rds_timing_tiles, dim3(static_cast<unsigned>(tiles)), dim3(RDS_THREADS), 0, as_stream(stream),
                           static_cast<const float2 *>(y_dev), static_cast<const double *>(psi_dev), (long long)n, (long long)j0,
                           static_cast<double *>(partials_dev));
    hipLaunchKernelGGL(k_rds_timing_total, dim3(1), dim3(RDS_THREADS), 0, as_stream(stream), static_cast<const double *>(partials_dev),
                       (long long)tiles, static_cast<double *>(out_dev));
    return check_launch("k_rds_timing");
}

extern "C" int iqa_rds_symbols(const void *y_dev, const void *psi_dev, int64_t n, int64_t j0, double tau, int64_t k_first,
                               int64_t nsym, void *sym_out_dev, void *bits_out_dev, void *stream)
{
    if (n < 0 || nsym < 0) return fail_inval("negative length");
    if (j0 < 0) return fail_inval("negative first index");
    if (!std::isfinite(tau)) return fail_inval("timing offset is not finite");
    if (n == 0 || nsym == 0) return IQA_OK;
    if (!y_dev || !psi_dev || !sym_out_dev || !bits_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40) || nsym > (1LL << 40)) return fail_inval("length out of range");
    hipLaunchKernelGGL(k_rds_symbols, grid1d(n, 256), dim3(256), 0, as_stream(stream), static_cast<const float2 *>(y_dev),
                       static_cast<const double *>(psi_dev), (long long)n, (long long)j0, tau, (long long)k_first, (long long)nsym,
                       static_cast<float2 *>(sym_out_dev));
    if (nsym > 1)
        hipLaunchKernelGGL(k_rds_bits, grid1d(nsym - 1, 256), dim3(256), 0, as_stream(stream), static_cast<const float2 *>(sym_out_dev),
                           (long long)nsym, static_cast<unsigned char *>(bits_out_dev));
    return check_launch("k_rds_symbols");
}

extern "C" int iqa_rds_syndromes(const void *bits_dev, int64_t nbits, void *words_out_dev, void *synd_out_dev, void *stream)
{
    if (nbits < 0) return fail_inval("negative length");
    if (nbits < 26) return IQA_OK;
    if (!bits_dev || !words_out_dev || !synd_out_dev) return fail_inval("NULL device pointer");
    if (nbits > (1LL << 40)) return fail_inval("length out of range");
    hipLaunchKernelGGL(k_rds_syndromes, grid1d(nbits - 25, 256), dim3(256), 0, as_stream(stream),
                       static_cast<const unsigned char *>(bits_dev), (long long)nbits, static_cast<unsigned int *>(words_out_dev),
                       static_cast<unsigned short *>(synd_out_dev));
    return check_launch("k_rds_syndromes");
}
