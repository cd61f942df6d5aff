// wfm.hip -- wideband FM stereo decoding over the composite, for gfx950.
//
// Specification (float64 statement; this kernel computes it in float32 in a fixed order):
//   m[n]  = theta[n] * fs / (2 pi 75 000)                 theta = iqa_quadrature of the channel (radians per sample)
//   p[n]  = sum_k h_p[k] m[n-k]                           analytic pilot, h_p[k] = h_lp1500[k] exp(+j 2 pi 19 000 (k - D) / fs)
//   c[n]  = -Im(u[n]^2), u = p / |p|   (0 where |p| < 1e-12)   = sin 2 theta_pilot[n - D]
//   md[n] = m[n - D],  D = (N - 1) / 2
//   a     = h_a * md                                      mono (L + R)
//   b     = h_a * (2 md c)                                stereo difference (L - R)
// with N-tap causal filters of zero initial state; h_a (16.5 kHz low-pass) and h_lp1500 are symmetric, so h_p[N-1-k] =
// conj(h_p[k]).  The caller carries the last 2(N-1) discriminator values of the stream across calls.
//
// One workgroup owns WFM_TILE consecutive outputs.  It stages the composite of its outputs plus a halo of 2(N-1)
// samples in LDS, computes the product q = 2 md c over its outputs plus a halo of N-1 (the halo is recomputed by the
// neighbouring tile: every value of q comes out of the same instructions whichever tile computes it), then both
// low-passes from LDS.  Every FIR sum runs over the symmetric tap pairs k = 0 .. D-1 in that order and ends with the
// centre tap, each term one float32 fmaf: an output does not depend on the tiling, nor on where the caller's blocks
// begin.  The per-tile sum of |p|^2 over the tile's own outputs (float64) is the stereo decision's statistic.
#include "common.h"

#include <cmath>

namespace iqa {

constexpr int WFM_THREADS = 256;
constexpr int WFM_TILE = 2048;                   // outputs per workgroup
constexpr int WFM_PER = WFM_TILE / WFM_THREADS;  // outputs per thread, WFM_THREADS apart (conflict-free LDS reads)

struct WfmArgs {
    const float *taps;   // [3 (D+1)]: h_a[0..D], Re h_p[0..D], Im h_p[0..D]
    const float *theta;  // [n]
    const float *hist;   // [2(N-1)]: the discriminator values in front of theta[0]; NULL = zeros (start of a stream)
    float *m_out;        // optional [n]
    float *a_out;        // [n]
    float *b_out;        // [n]
    double *partials;    // optional [ceil(n / WFM_TILE)]
    long long n;
    int ntaps;
    float scale;         // composite per radian
};

__host__ __device__ constexpr int wfm_lds_floats(int ntaps)
{
    // taps + composite window (2(N-1) + TILE) + products (N-1 + TILE)
    return 3 * ((ntaps - 1) / 2 + 1) + 3 * (ntaps - 1) + 2 * WFM_TILE;
}

__global__ __launch_bounds__(WFM_THREADS) void k_wfm_stereo(WfmArgs g)
{
    extern __shared__ float s_mem[];
    __shared__ double s_red[WFM_THREADS / kWave];
    const int N = g.ntaps, D = (N - 1) / 2, H = N - 1;
    const int nx = 2 * H + WFM_TILE, nq = H + WFM_TILE;
    float *s_h = s_mem;
    float *s_x = s_h + 3 * (D + 1);  // s_x[i] = m at position n0 - 2H + i
    float *s_q = s_x + nx;           // s_q[j] = q at position n0 - H + j
    const float *ha = s_h, *hr = s_h + (D + 1), *hi = s_h + 2 * (D + 1);
    const int tid = threadIdx.x;
    const long long n0 = static_cast<long long>(blockIdx.x) * WFM_TILE;

    for (int i = tid; i < 3 * (D + 1); i += WFM_THREADS) s_h[i] = g.taps[i];
    for (int i = tid; i < nx; i += WFM_THREADS) {
        const long long pos = n0 - 2 * H + i;
        float v = 0.f;
        if (pos >= 0) {
            if (pos < g.n) v = g.theta[pos];
        } else if (g.hist != nullptr) {
            v = g.hist[2 * H + pos];  // pos >= -2H
        }
        s_x[i] = v * g.scale;
    }
    __syncthreads();

    // pilot, carrier and product over the tile's outputs and the N-1 positions in front of them
    double pw = 0.0;
    for (int j = tid; j < nq; j += WFM_THREADS) {
        const float *x = s_x + j;  // x[i] = m at position P - H + i, P = n0 - H + j
        float pr = 0.f, pi = 0.f;
        for (int k = 0; k < D; ++k) {
            const float x1 = x[H - k], x2 = x[k];  // taps k and N-1-k
            pr = fmaf(hr[k], x1 + x2, pr);
            pi = fmaf(hi[k], x1 - x2, pi);
        }
        pr = fmaf(hr[D], x[D], pr);
        const float pp = pr * pr + pi * pi;
        const float c = pp < 1e-24f ? 0.f : -2.f * pr * pi / pp;
        s_q[j] = 2.f * x[D] * c;  // x[D] = m[P - D] = md[P]
        if (j >= H && n0 + (j - H) < g.n) pw += static_cast<double>(pr) * pr + static_cast<double>(pi) * pi;
    }
    __syncthreads();

    // both low-passes; output t of the tile: md[n - k] = s_x[t + 3D - k], q[n - k] = s_q[t + 2D - k]
    float acc_a[WFM_PER], acc_b[WFM_PER];
#pragma unroll
    for (int r = 0; r < WFM_PER; ++r) acc_a[r] = acc_b[r] = 0.f;
    for (int k = 0; k < D; ++k) {
        const float h = ha[k];
#pragma unroll
        for (int r = 0; r < WFM_PER; ++r) {
            const int t = tid + r * WFM_THREADS;
            acc_a[r] = fmaf(h, s_x[t + 3 * D - k] + s_x[t + D + k], acc_a[r]);
            acc_b[r] = fmaf(h, s_q[t + 2 * D - k] + s_q[t + k], acc_b[r]);
        }
    }
    const float hc = ha[D];
#pragma unroll
    for (int r = 0; r < WFM_PER; ++r) {
        const int t = tid + r * WFM_THREADS;
        const long long pos = n0 + t;
        if (pos < g.n) {
            g.a_out[pos] = fmaf(hc, s_x[t + 2 * D], acc_a[r]);
            g.b_out[pos] = fmaf(hc, s_q[t + D], acc_b[r]);
            if (g.m_out != nullptr) g.m_out[pos] = s_x[t + 2 * H];
        }
    }

    if (g.partials != nullptr) {
        pw = wave_sum(pw);
        if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = pw;
        __syncthreads();
        if (tid == 0) g.partials[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    }
}

// L = a + b, R = a - b (in place allowed: left == a, right == b)
__global__ __launch_bounds__(256) void k_wfm_matrix(const float *a, const float *b, long long n, float *left, float *right)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float av = a[i], bv = b[i];
    left[i] = av + bv;
    right[i] = av - bv;
}

static_assert(WFM_THREADS / kWave == 4, "the partial-sum reduction adds four waves");
static_assert(wfm_lds_floats(IQA_WFM_MAX_TAPS) * 4 <= 64 * 1024 - 64, "the longest filter must fit the default LDS allowance");

}  // namespace iqa

using namespace iqa;

extern "C" int64_t iqa_wfm_partials(int64_t n) { return n <= 0 ? 0 : (n + WFM_TILE - 1) / WFM_TILE; }

extern "C" int iqa_wfm_stereo(int32_t ntaps, const void *taps_dev, float m_scale, const void *theta_dev, int64_t n,
                              const void *hist_dev, void *m_out_dev, void *a_out_dev, void *b_out_dev, void *partials_dev,
                              void *stream)
{
    if (ntaps < 3 || ntaps > IQA_WFM_MAX_TAPS || (ntaps & 1) == 0) return fail_inval("ntaps must be odd, 3 .. IQA_WFM_MAX_TAPS");
    if (n < 0) return fail_inval("negative length");
    if (!std::isfinite(m_scale)) return fail_inval("composite scale is not finite");
    if (n == 0) return IQA_OK;
    if (!taps_dev || !theta_dev || !a_out_dev || !b_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    WfmArgs g;
    g.taps = static_cast<const float *>(taps_dev);
    g.theta = static_cast<const float *>(theta_dev);
    g.hist = static_cast<const float *>(hist_dev);
    g.m_out = static_cast<float *>(m_out_dev);
    g.a_out = static_cast<float *>(a_out_dev);
    g.b_out = static_cast<float *>(b_out_dev);
    g.partials = static_cast<double *>(partials_dev);
    g.n = n;
    g.ntaps = ntaps;
    g.scale = m_scale;
    const size_t lds = static_cast<size_t>(wfm_lds_floats(ntaps)) * sizeof(float);
    hipLaunchKernelGGL(k_wfm_stereo, dim3(static_cast<unsigned>(iqa_wfm_partials(n))), dim3(WFM_THREADS), lds, as_stream(stream), g);
    return check_launch("k_wfm_stereo");
}

extern "C" int iqa_wfm_matrix(const void *a_dev, const void *b_dev, int64_t n, void *left_dev, void *right_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!a_dev || !b_dev || !left_dev || !right_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_wfm_matrix, grid1d(n, 256), dim3(256), 0, as_stream(stream), static_cast<const float *>(a_dev),
                       static_cast<const float *>(b_dev), (long long)n, static_cast<float *>(left_dev), static_cast<float *>(right_dev));
    return check_launch("k_wfm_matrix");
}
