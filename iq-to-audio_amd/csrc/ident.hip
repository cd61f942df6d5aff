// ident.hip -- which protocol a keyed channel carries, by its frame synchronisation words (--find-identify, DESIGN.md section
// 25), for gfx950: a symbol-long integrator over the stored discriminator stream, the normalised correlation of every sync
// pattern of the channel's family at every sample, and the list of the local maxima.
//
// Specification (theta the stored discriminator stream of n samples, index 0 its first sample and t - c = 0 in front of it; c
// the centre; L = rint(sps), h = floor(sps / 2), sh the shift, o[i] = rint(i sps) for i = -16 .. 47, half-even in float64):
//   t    = clamp(rintf(theta 4096), -32767, 32767)                        (float32, half-even; NaN -> 0, +-inf -> +-32767)
//   S[m] = sum_{j < L, j <= m} (t[m - j] - c)                              (int32: 224 * 65534 < 2^24)
//   v[m] = S[m] >> sh                                                      (arithmetic; |v| <= 64 * 65534)
//   per pattern p of N symbols p_i in {-3, -1, +1, +3}, at every m with m + o[N - 1] < n:
//     C = sum p_i v[m + o[i]], E = sum v[m + o[i]]^2, Pn = sum p_i^2       (int64)
//     m is a candidate iff E > 0 and 16 C^2 >= 13 Pn E; its score is 2 |C| + (C < 0), 0 for every other m
//     kept iff no candidate of p within +-h has a larger |C|, or the same |C| at a smaller index
//   a kept hit appends (p, m, C, E, pre, post): bit k of pre = (v[m + o[-16 + k]] > 0), of post = (v[m + o[N + k]] > 0),
//   k = 0 .. 15, 0 where the position lies outside the stream.
//
// k_ident_integrate: the side-band tile of sideband.h (256 threads x 8 consecutive samples) with the L - 1 values in front;
// a thread makes one full window sum and seven slides.  k_ident_score: a workgroup stages 1024 positions and the longest
// span of v into LDS, the offsets and the symbols beside them; for a fixed symbol consecutive lanes read consecutive words.
// k_ident_keep: one thread per position and pattern on the few candidates, reading global memory directly, appending through
// one atomic counter as k_pocsag_keep does, pre and post through protocol.h's checked read; the host prologue is protocol.h's
// too.  Integers only behind the quantiser; plain C++ stores, no inline assembly.
#include "protocol.h"
#include "sideband.h"

namespace iqa {

constexpr int ID_THREADS = SB_THREADS;
constexpr int ID_T_MAX = 32767;
constexpr int ID_MAX_L = IQA_IDENT_MAX_SPS;                       // 224
constexpr int ID_FRONT = sb_front(ID_MAX_L);                      // 224: the largest front of the integrator's image
constexpr int ID_IMAGE = sb_pad(ID_FRONT + SB_TILE) + 1;          // words of the integrator's image
constexpr int ID_SCORE_TILE = 1024;                               // positions per workgroup of k_ident_score
constexpr int ID_OFFS = IQA_IDENT_OFFSETS;                        // 64: o[-16] .. o[47]
constexpr int ID_LEAD = 16;                                       // o[i] sits at index 16 + i
constexpr int ID_SYMS = IQA_IDENT_MAX_SYMBOLS;                    // 32
constexpr int ID_PATS = IQA_IDENT_MAX_PATTERNS;                   // 8
constexpr long long ID_V_MAX = PL_V_MAX;                          // |v|
constexpr int ID_RECORD = IQA_IDENT_RECORD;                       // 6 int64 of a kept hit

// every product of the candidate test stays inside int64
static_assert(ID_V_MAX * 3 * ID_SYMS < (1LL << 29), "|C| < 2^29, so 2 |C| + 1 fits the int32 score");
static_assert(16.0 * (double(ID_V_MAX) * 3 * ID_SYMS) * (double(ID_V_MAX) * 3 * ID_SYMS) < 9.2e18, "16 C^2 < 2^63");
static_assert(13.0 * (9 * ID_SYMS) * (double(ID_V_MAX) * ID_V_MAX * ID_SYMS) < 9.2e18, "13 Pn E < 2^63");
static_assert((static_cast<long long>(ID_MAX_L) * 65534) < (1LL << 24), "S stays inside int32");
static_assert((ID_SCORE_TILE + (ID_SYMS - 1) * ID_MAX_L) * 4 + (ID_OFFS + ID_PATS * ID_SYMS + 2 * ID_PATS) * 4 <= 64 * 1024,
              "the score tile and its span must fit the default LDS allowance");

struct IdentTable {
    int o[ID_OFFS];                   // o[-16 .. 47] at index 16 + i
    int nsym[ID_PATS];
    int pn[ID_PATS];                  // sum p_i^2
    signed char sym[ID_PATS][ID_SYMS];
    int npat;
};

__device__ __forceinline__ int id_clamp(int t) { return min(max(t, -ID_T_MAX), ID_T_MAX); }

__global__ __launch_bounds__(ID_THREADS) void k_ident_integrate(const float *__restrict__ theta, long long n, int L, int sh, int c,
                                                                int *__restrict__ v_out)
{
    __shared__ int s_t[ID_IMAGE];  // the image of rint(theta 4096) from stream index A - H
    const int tid = threadIdx.x, H = sb_front(L);
    const long long A = static_cast<long long>(blockIdx.x) * SB_TILE;
    sb_stage(s_t, H, A, n, theta, SbScale{4096.0f}, nullptr, 0, nullptr, 0);
    __syncthreads();
    const int first = H + tid * SB_RUN;  // image index (unpadded) of this thread's first output
    const long long a0 = A + tid * SB_RUN;
    if (a0 >= n) return;
    int acc = 0;
    for (int k = 0; k < L; ++k) acc += id_clamp(s_t[sb_pad(first - k)]);  // (first - k >= H - (L - 1) >= 0; zeros in front of the stream)
#pragma unroll
    for (int r = 0; r < SB_RUN; ++r) {
        if (r) acc += id_clamp(s_t[sb_pad(first + r)]) - id_clamp(s_t[sb_pad(first + r - L)]);
        const long long have = a0 + r + 1;  // samples of the stream up to this one: the window holds min(L, have) of them
        const int cnt = have < L ? static_cast<int>(have) : L;
        if (a0 + r < n) v_out[a0 + r] = (acc - c * cnt) >> sh;
    }
}

// C and E of pattern symbols sym[0 .. N) at the values x[off[i]], i = 0 .. N - 1
template <class Load>
__device__ __forceinline__ void id_eval(Load load, const int *sym, const int *off, int N, int &C, long long &E)
{
    C = 0;
    E = 0;
    for (int i = 0; i < N; ++i) {
        const int x = load(off[i]);
        C += sym[i] * x;  // (|C| < 2^29)
        E += static_cast<long long>(x) * x;
    }
}

__device__ __forceinline__ bool id_candidate(int C, long long E, int pn)
{
    const long long c = C;
    return E > 0 && 16 * c * c >= 13LL * pn * E;
}

__global__ __launch_bounds__(ID_THREADS) void k_ident_score(const int *__restrict__ v, long long n, IdentTable tb, int span,
                                                            int *__restrict__ score)
{
    extern __shared__ int s_v[];  // s_v[i] = v[A + i], i = 0 .. ID_SCORE_TILE + span - 1
    __shared__ int s_o[ID_OFFS];
    __shared__ int s_sym[ID_PATS * ID_SYMS];
    const int tid = threadIdx.x;
    const long long A = static_cast<long long>(blockIdx.x) * ID_SCORE_TILE;
    const int width = ID_SCORE_TILE + span;
    for (int i = tid; i < width; i += ID_THREADS) s_v[i] = A + i < n ? v[A + i] : 0;
    if (tid < ID_OFFS) s_o[tid] = tb.o[tid];
    for (int i = tid; i < tb.npat * ID_SYMS; i += ID_THREADS) s_sym[i] = tb.sym[i / ID_SYMS][i % ID_SYMS];
    __syncthreads();
    for (int m = tid; m < ID_SCORE_TILE; m += ID_THREADS) {
        const long long a = A + m;
        if (a >= n) return;
        for (int p = 0; p < tb.npat; ++p) {
            const int N = tb.nsym[p];
            int out = 0;
            if (a + s_o[ID_LEAD + N - 1] < n) {  // (o[N - 1] <= span: every read stays inside the staged width)
                int C;
                long long E;
                id_eval([&](int off) { return s_v[m + off]; }, s_sym + p * ID_SYMS, s_o + ID_LEAD, N, C, E);
                if (id_candidate(C, E, tb.pn[p])) out = C < 0 ? 2 * -C + 1 : 2 * C;
            }
            score[static_cast<long long>(p) * n + a] = out;
        }
    }
}

__global__ __launch_bounds__(ID_THREADS) void k_ident_keep(const int *__restrict__ v, long long n, IdentTable tb, int half,
                                                           const int *__restrict__ score, long long *__restrict__ list,
                                                           long long capacity, unsigned long long *count)
{
    __shared__ int s_o[ID_OFFS];
    __shared__ int s_sym[ID_SYMS];
    const int tid = threadIdx.x, p = blockIdx.y;
    if (tid < ID_OFFS) s_o[tid] = tb.o[tid];
    if (tid < ID_SYMS) s_sym[tid] = tb.sym[p][tid];
    __syncthreads();
    const long long a = static_cast<long long>(blockIdx.x) * ID_THREADS + tid;
    if (a >= n) return;
    const int *plane = score + static_cast<long long>(p) * n;
    const int sc = plane[a];
    if (sc == 0) return;
    const int mine = sc >> 1;
    const long long lo = a - half < 0 ? 0 : a - half, hi = a + half > n - 1 ? n - 1 : a + half;
    for (long long m = lo; m <= hi; ++m) {
        const int other = plane[m] >> 1;  // (0 where m is no candidate: |C| > 0 for every candidate)
        if (other > mine || (other == mine && m < a)) return;
    }
    const int N = tb.nsym[p];
    int C;
    long long E;
    id_eval([&](int off) { return v[a + off]; }, s_sym, s_o + ID_LEAD, N, C, E);  // (a candidate: a + o[N - 1] < n)
    unsigned pre = 0, post = 0;
#pragma unroll 1  // (unrolled, the 32 reads of a kept hit are issued at once and take 74 registers, not 23)
    for (int k = 0; k < 16; ++k) {
        bool inside;  // (an instant outside the stream reads as 0: its bit stays clear)
        if (pl_read(v, n, a + s_o[k], inside) > 0) pre |= 1u << k;
        if (pl_read(v, n, a + s_o[ID_LEAD + N + k], inside) > 0) post |= 1u << k;
    }
    const unsigned long long at = atomicAdd(count, 1ULL);
    if (at < static_cast<unsigned long long>(capacity)) {
        long long *e = list + ID_RECORD * at;
        e[0] = p;
        e[1] = a;
        e[2] = C;
        e[3] = E;
        e[4] = pre;
        e[5] = post;
    }
}

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_ident_integrate(const void *theta_dev, int64_t n, int32_t L, int32_t sh, int32_t c, void *v_dev, void *stream)
{
    if (const int rc = pl_check_lengths(n, 0)) return rc;
    if (L < IQA_IDENT_MIN_SPS || L > IQA_IDENT_MAX_SPS) return fail_inval("L must be IQA_IDENT_MIN_SPS .. IQA_IDENT_MAX_SPS");
    if (sh < 0 || sh > 8 || ((static_cast<long long>(L) * 65534) >> sh) > ID_V_MAX) return fail_inval("sh must be 0 .. 8 and keep |v| within 64 * 65534");
    if (c < -ID_T_MAX || c > ID_T_MAX) return fail_inval("the centre must be -32767 .. 32767");
    if (n == 0) return IQA_OK;
    if (!theta_dev || !v_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_ident_integrate, grid1d(n, SB_TILE), dim3(ID_THREADS), 0, as_stream(stream),
                       static_cast<const float *>(theta_dev), (long long)n, (int)L, (int)sh, (int)c, static_cast<int *>(v_dev));
    return check_launch("k_ident_integrate");
}

extern "C" int iqa_ident_search(const void *v_dev, int64_t n, const int32_t offsets[IQA_IDENT_OFFSETS], int32_t npat,
                                const int8_t *symbols, const int32_t *nsym, int32_t half, void *score_dev, void *list_dev,
                                int64_t capacity, void *count_dev, void *stream)
{
    if (capacity < 0) return fail_inval("negative length");
    if (const int rc = pl_check_lengths(n, 0)) return rc;
    if (!offsets || !symbols || !nsym) return fail_inval("NULL offsets, symbols or symbol counts");
    if (npat < 1 || npat > ID_PATS) return fail_inval("npat must be 1 .. IQA_IDENT_MAX_PATTERNS");
    if (half < 0 || half > IQA_IDENT_MAX_SPS) return fail_inval("half must be 0 .. IQA_IDENT_MAX_SPS");
    IdentTable tb;
    if (const int rc = pl_copy_offsets(offsets, ID_OFFS, ID_LEAD, "offsets", tb.o)) return rc;
    int span = 0;
    tb.npat = npat;
    for (int p = 0; p < ID_PATS; ++p) {
        tb.nsym[p] = tb.pn[p] = 0;
        for (int i = 0; i < ID_SYMS; ++i) tb.sym[p][i] = 0;
    }
    for (int p = 0; p < npat; ++p) {
        const int N = nsym[p];
        if (N < 1 || N > ID_SYMS) return fail_inval("a pattern must hold 1 .. IQA_IDENT_MAX_SYMBOLS symbols");
        tb.nsym[p] = N;
        for (int i = 0; i < N; ++i) {
            const int s = symbols[p * ID_SYMS + i];
            if (s != -3 && s != -1 && s != 1 && s != 3) return fail_inval("a symbol must be -3, -1, +1 or +3");
            tb.sym[p][i] = static_cast<signed char>(s);
            tb.pn[p] += s * s;
        }
        span = tb.o[ID_LEAD + N - 1] > span ? tb.o[ID_LEAD + N - 1] : span;
    }
    if (span > (ID_SYMS - 1) * ID_MAX_L) return fail_inval("o[N - 1] must not exceed 31 IQA_IDENT_MAX_SPS");
    if (n == 0) return IQA_OK;  // (nothing to search: no pointer is touched, the count stays as it is)
    if (!v_dev || !score_dev || !count_dev || (capacity > 0 && !list_dev)) return fail_inval("NULL device pointer");
    if (hipMemsetAsync(count_dev, 0, sizeof(long long), as_stream(stream)) != hipSuccess) {  // (behind every check)
        set_error("clearing the hit count failed");
        return IQA_EHIP;
    }
    const int *v = static_cast<const int *>(v_dev);
    int *score = static_cast<int *>(score_dev);
    const size_t lds = static_cast<size_t>(ID_SCORE_TILE + span) * sizeof(int);
    hipLaunchKernelGGL(k_ident_score, grid1d(n, ID_SCORE_TILE), dim3(ID_THREADS), lds, as_stream(stream), v, (long long)n, tb, span, score);
    dim3 grid = grid1d(n, ID_THREADS);
    grid.y = npat;
    hipLaunchKernelGGL(k_ident_keep, grid, dim3(ID_THREADS), 0, as_stream(stream), v, (long long)n, tb, (int)half,
                       static_cast<const int *>(score), static_cast<long long *>(list_dev), (long long)capacity,
                       static_cast<unsigned long long *>(count_dev));
    return check_launch("k_ident_search");
}
