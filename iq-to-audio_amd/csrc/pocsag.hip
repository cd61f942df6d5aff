// pocsag.hip -- POCSAG paging (512 / 1200 / 2400 baud 2-FSK) beside the NFM demodulator, for gfx950.
//
// Specification (fs the channel rate, theta the discriminator output, all indices absolute, everything zero in front of
// the stream; per baud B: sps = fs / B, L = rint(sps), h = floor(sps / 2), off[i] = rint(i sps) half-even in float64):
//   t[n]   = rint(theta[n] 2^20)                            (int32, half-even; integers from here on)
//   S[n]   = t[n] + t[n-1] + .. + t[n-L+1]                  (int32: L pi 2^20 < 2^31)
//   v_i    = S[n + off[i]], i = 0 .. 31;  Sigma = sum v_i;  x_i = 32 v_i - Sigma;  w_i = (x_i < 0);  W = w_0 .. w_31
//   d+     = popcount(W xor 0x7CD215D8), d- = 32 - d+;  E = sum |x_i|
//   n is a candidate iff min(d+, d-) <= 2 and 128 min |x_i| >= E; kept iff no candidate within +-h has a larger E
//   (or the same E at a smaller index).  Codeword c, bit b of a kept sync: (32 S[n + off[32 (1 + c) + b]] < Sigma) xor inverted,
//   then the BCH(31,21) syndrome (g = 0x769), the parity of all 32 bits and single-error correction.
//
// k_pocsag_integrate: sideband.h's tile with all hist_len >= max L - 1 carried values as its front; each thread then makes
// 8 consecutive outputs per baud: one full window sum, then seven slides.
// k_pocsag_score: a workgroup stages 1024 + off[31] integrator values; a thread evaluates one n at a time, and for a fixed
// bit i consecutive lanes read consecutive words.  k_pocsag_keep and k_pocsag_codewords work on the few candidates and
// kept syncs and read global memory directly.
#include "sideband.h"

#include <climits>

namespace iqa {

constexpr int PG_THREADS = SB_THREADS;
constexpr int PG_SYNC_TILE = 1024;              // positions per workgroup of k_pocsag_score
constexpr unsigned PG_SYNC_WORD = 0x7CD215D8u;
constexpr unsigned PG_POLY = 0x769u;            // x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
constexpr float PG_THETA_SCALE = 1048576.0f;    // 2^20

struct PocsagIntArgs {
    const float *theta;  // [n]
    const int *hist;     // [hist_len]: t in front of theta[0]; NULL = zeros
    int *t_out;          // [n]
    int *s_out[IQA_POCSAG_BAUDS];  // [n] each; NULL where window = 0
    long long n;
    int hist_len;
    int window[IQA_POCSAG_BAUDS];
};

__global__ __launch_bounds__(PG_THREADS) void k_pocsag_integrate(PocsagIntArgs g)
{
    extern __shared__ int s_t[];  // the image of t from block index A - H
    const int tid = threadIdx.x, H = g.hist_len;
    const long long A = static_cast<long long>(blockIdx.x) * SB_TILE;
    sb_stage(s_t, H, A, g.n, g.theta, SbScale{PG_THETA_SCALE}, g.hist, H, g.t_out, H);
    __syncthreads();
    const int first = H + tid * SB_RUN;  // LDS index (unpadded) of this thread's first output
    const long long a0 = A + tid * SB_RUN;
    if (a0 >= g.n) return;
#pragma unroll
    for (int b = 0; b < IQA_POCSAG_BAUDS; ++b) {
        const int L = g.window[b];
        if (L == 0) continue;
        int *out = g.s_out[b];
        int acc = 0;
        for (int k = 0; k < L; ++k) acc += s_t[sb_pad(first - k)];  // (first - k >= H - (L - 1) >= 0)
        out[a0] = acc;
#pragma unroll
        for (int r = 1; r < SB_RUN; ++r) {
            acc += s_t[sb_pad(first + r)] - s_t[sb_pad(first + r - L)];
            if (a0 + r < g.n) out[a0 + r] = acc;
        }
    }
}

struct PocsagOffsets {
    int off[32];
};

// Sigma, W, E and min |x| of the 32 values v_i
__device__ __forceinline__ void pg_eval(const int (&v)[32], long long &sum, unsigned &word, long long &energy, long long &least)
{
    sum = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) sum += v[i];
    word = 0;
    energy = 0;
    least = LLONG_MAX;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const long long x = 32LL * v[i] - sum;
        const long long ax = x < 0 ? -x : x;
        word = (word << 1) | (x < 0 ? 1u : 0u);
        energy += ax;
        least = ax < least ? ax : least;
    }
}

__global__ __launch_bounds__(PG_THREADS) void k_pocsag_score(const int *__restrict__ S, long long n, long long n_eval,
                                                             PocsagOffsets o, long long *__restrict__ score)
{
    extern __shared__ int s_s[];  // s_s[i] = S[A + i], i = 0 .. PG_SYNC_TILE + off[31] - 1
    const int tid = threadIdx.x;
    const long long A = static_cast<long long>(blockIdx.x) * PG_SYNC_TILE;
    const int width = PG_SYNC_TILE + o.off[31];
    for (int i = tid; i < width; i += PG_THREADS) s_s[i] = A + i < n ? S[A + i] : 0;
    __syncthreads();
    for (int m = tid; m < PG_SYNC_TILE; m += PG_THREADS) {
        const long long a = A + m;
        if (a >= n) return;
        long long out = 0;
        if (a < n_eval) {
            int v[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) v[i] = s_s[m + o.off[i]];
            long long sum, energy, least;
            unsigned word;
            pg_eval(v, sum, word, energy, least);
            const int dp = __popc(word ^ PG_SYNC_WORD), dn = 32 - dp;
            if ((dp <= 2 || dn <= 2) && 128 * least >= energy) out = 2 * energy + (dn < dp ? 1 : 0);
        }
        score[a] = out;
    }
}

__global__ __launch_bounds__(PG_THREADS) void k_pocsag_keep(const int *__restrict__ S, long long n, PocsagOffsets o, int half_bit,
                                                            const long long *__restrict__ score, long long *__restrict__ list,
                                                            long long capacity, unsigned long long *count)
{
    const long long a = static_cast<long long>(blockIdx.x) * PG_THREADS + threadIdx.x;
    if (a >= n) return;
    const long long sc = score[a];
    if (sc == 0) return;
    const long long e = sc >> 1;
    const long long lo = a - half_bit < 0 ? 0 : a - half_bit, hi = a + half_bit > n - 1 ? n - 1 : a + half_bit;
    for (long long m = lo; m <= hi; ++m) {
        const long long em = score[m] >> 1;  // (0 where m is no candidate: e > 0 for every candidate)
        if (em > e || (em == e && m < a)) return;
    }
    int v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = S[a + o.off[i]];  // (a candidate: a + off[31] < n)
    long long sum, energy, least;
    unsigned word;
    pg_eval(v, sum, word, energy, least);
    const int dp = __popc(word ^ PG_SYNC_WORD), dn = 32 - dp;
    const unsigned long long at = atomicAdd(count, 1ULL);
    if (at < static_cast<unsigned long long>(capacity)) {
        long long *e4 = list + 4 * at;
        e4[0] = a;
        e4[1] = sum;
        e4[2] = dn < dp ? 1 : 0;
        e4[3] = dn < dp ? dn : dp;
    }
}

// remainder of the upper 31 bits of a codeword modulo g (10 bits)
__host__ __device__ constexpr unsigned pg_syndrome(unsigned cw)
{
    unsigned r = cw >> 1;
    for (int i = 30; i >= 10; --i)
        if ((r >> i) & 1u) r ^= PG_POLY << (i - 10);
    return r & 0x3FFu;
}

__global__ __launch_bounds__(PG_THREADS) void k_pocsag_codewords(const int *__restrict__ S, long long n, const long long *__restrict__ list,
                                                                 long long nsync, const int *__restrict__ offs,
                                                                 unsigned *__restrict__ fixed_out, unsigned *__restrict__ raw_out,
                                                                 unsigned char *__restrict__ status_out)
{
    const long long id = static_cast<long long>(blockIdx.x) * PG_THREADS + threadIdx.x;
    if (id >= nsync * 16) return;
    const long long k = id >> 4;
    const int c = static_cast<int>(id & 15), base = 32 * (1 + c);
    const long long m = list[4 * k], sum = list[4 * k + 1];
    const unsigned inv = list[4 * k + 2] ? 1u : 0u;
    unsigned raw = 0, fixed = 0;
    unsigned char status = 3;
    if (m >= 0 && m + offs[base + 31] < n) {
        for (int b = 0; b < 32; ++b) {
            const long long v = S[m + offs[base + b]];
            raw = (raw << 1) | ((32 * v < sum ? 1u : 0u) ^ inv);
        }
        const unsigned syn = pg_syndrome(raw), odd = __popc(raw) & 1u;
        fixed = raw;
        status = 2;
        if (syn == 0) {
            status = odd ? 1 : 0;
            fixed = raw ^ odd;  // (an odd word with a clean syndrome: the parity bit itself)
        } else if (odd) {
            for (int pos = 1; pos < 32; ++pos)
                if (pg_syndrome(1u << pos) == syn) {  // (distance 5: the 31 single-bit syndromes are distinct)
                    fixed = raw ^ (1u << pos);
                    status = 1;
                    break;
                }
        }
    }
    fixed_out[id] = fixed;
    raw_out[id] = raw;
    status_out[id] = status;
}

static_assert(pg_syndrome(PG_SYNC_WORD) == 0 && pg_syndrome(0x7A89C197u) == 0, "the sync and idle words are codewords of g");
static_assert((PG_SYNC_TILE + 31 * IQA_POCSAG_MAX_SPS) * 4 <= 64 * 1024, "the sync window must fit the default LDS allowance");
static_assert(sb_pad(IQA_POCSAG_MAX_SPS + SB_TILE) * 4 + 4 <= 64 * 1024, "the integrator window must fit the default LDS allowance");

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_pocsag_integrate(const void *theta_dev, int64_t n, const void *hist_dev, int32_t hist_len,
                                    const int32_t window[IQA_POCSAG_BAUDS], void *t_out_dev, void *const s_out_dev[IQA_POCSAG_BAUDS],
                                    void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (!window || !s_out_dev) return fail_inval("NULL window or output table");
    if (hist_len < 0 || hist_len > IQA_POCSAG_MAX_SPS) return fail_inval("hist_len must be 0 .. IQA_POCSAG_MAX_SPS");
    PocsagIntArgs g;
    int longest = 0;
    for (int b = 0; b < IQA_POCSAG_BAUDS; ++b) {
        if (window[b] < 0 || window[b] > IQA_POCSAG_MAX_SPS) return fail_inval("window must be 0 .. IQA_POCSAG_MAX_SPS");
        if (window[b] > 0 && n > 0 && !s_out_dev[b]) return fail_inval("NULL integrator output for an active baud");
        g.window[b] = window[b];
        g.s_out[b] = static_cast<int *>(s_out_dev[b]);
        longest = window[b] > longest ? window[b] : longest;
    }
    if (longest == 0) return fail_inval("no active baud");
    if (hist_len < longest - 1) return fail_inval("hist_len must be at least the longest window - 1");
    if (n == 0) return IQA_OK;
    if (!theta_dev || !t_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    g.theta = static_cast<const float *>(theta_dev);
    g.hist = static_cast<const int *>(hist_dev);
    g.t_out = static_cast<int *>(t_out_dev);
    g.n = n;
    g.hist_len = hist_len;
    const size_t lds = static_cast<size_t>(sb_pad(hist_len + SB_TILE) + 1) * sizeof(int);
    hipLaunchKernelGGL(k_pocsag_integrate, grid1d(n, SB_TILE), dim3(PG_THREADS), lds, as_stream(stream), g);
    return check_launch("k_pocsag_integrate");
}

extern "C" int iqa_pocsag_sync(const void *s_dev, int64_t n, const int32_t offsets[32], int32_t half_bit, void *score_dev,
                               void *list_dev, int64_t capacity, void *count_dev, void *stream)
{
    if (n < 0 || capacity < 0) return fail_inval("negative length");
    if (!offsets) return fail_inval("NULL offsets");
    if (!count_dev) return fail_inval("NULL device pointer");
    if (half_bit < 0 || half_bit > IQA_POCSAG_MAX_SPS) return fail_inval("half_bit must be 0 .. IQA_POCSAG_MAX_SPS");
    PocsagOffsets o;
    for (int i = 0; i < 32; ++i) {
        if (offsets[i] < (i ? offsets[i - 1] : 0) || (i == 0 && offsets[0] != 0)) return fail_inval("offsets must ascend from 0");
        o.off[i] = offsets[i];
    }
    if (o.off[31] > 31 * IQA_POCSAG_MAX_SPS) return fail_inval("offsets[31] must not exceed 31 IQA_POCSAG_MAX_SPS");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    if (n > 0 && (!s_dev || !score_dev || (capacity > 0 && !list_dev))) return fail_inval("NULL device pointer");
    if (hipMemsetAsync(count_dev, 0, sizeof(long long), as_stream(stream)) != hipSuccess) {  // (behind every check)
        set_error("clearing the sync count failed");
        return IQA_EHIP;
    }
    if (n == 0) return IQA_OK;
    const int *S = static_cast<const int *>(s_dev);
    long long *score = static_cast<long long *>(score_dev);
    const long long n_eval = n - o.off[31] > 0 ? n - o.off[31] : 0;
    const size_t lds = static_cast<size_t>(PG_SYNC_TILE + o.off[31]) * sizeof(int);
    hipLaunchKernelGGL(k_pocsag_score, grid1d(n, PG_SYNC_TILE), dim3(PG_THREADS), lds, as_stream(stream), S, (long long)n, n_eval, o, score);
    hipLaunchKernelGGL(k_pocsag_keep, grid1d(n, PG_THREADS), dim3(PG_THREADS), 0, as_stream(stream), S, (long long)n, o, (int)half_bit,
                       static_cast<const long long *>(score), static_cast<long long *>(list_dev), (long long)capacity,
                       static_cast<unsigned long long *>(count_dev));
    return check_launch("k_pocsag_sync");
}

extern "C" int iqa_pocsag_codewords(const void *s_dev, int64_t n, const void *list_dev, int64_t nsync, const void *offsets_dev,
                                    void *fixed_out_dev, void *raw_out_dev, void *status_out_dev, void *stream)
{
    if (n < 0 || nsync < 0) return fail_inval("negative length");
    if (nsync == 0) return IQA_OK;
    if (!s_dev || !list_dev || !offsets_dev || !fixed_out_dev || !raw_out_dev || !status_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40) || nsync > (1LL << 32)) return fail_inval("length out of range");
    hipLaunchKernelGGL(k_pocsag_codewords, grid1d(nsync * 16, PG_THREADS), dim3(PG_THREADS), 0, as_stream(stream),
                       static_cast<const int *>(s_dev), (long long)n, static_cast<const long long *>(list_dev), (long long)nsync,
                       static_cast<const int *>(offsets_dev), static_cast<unsigned *>(fixed_out_dev),
                       static_cast<unsigned *>(raw_out_dev), static_cast<unsigned char *>(status_out_dev));
    return check_launch("k_pocsag_codewords");
}
