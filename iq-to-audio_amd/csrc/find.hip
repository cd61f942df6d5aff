// find.hip -- the occupied channels of a capture (--find-channels), for gfx950.
//
// Specification (row[f][k] the float32 dB rows of iqa_psd_frames, frame f of the run at sample f hop, F frames in all, all
// indices absolute; T frames to a slice, S = ceil(F / T) slices; everything behind c is integer):
//   c[f][k]  = clamp(rint(100.0f row[f][k]), -30000, 30000)              (one float32 product, half-even; NaN -> -30000)
//   sum[k]   = sum_f c  (int64),  max[k] = max_f c  (int32, -30000 before any frame),  slice[s][k] = sum_{f / T = s} c  (int32)
//   mean[k]  = floor(sum[k] / F)
//   floor[k] = the value of rank ((hi - lo) num) / den, 0-based ascending, among plane[lo .. hi], lo = max(0, k - h),
//              hi = min(nbins - 1, k + h); fmean from mean, fmax from max
//   x[k]     = max(mean - fmean - thr, max - fmax - thr_peak);  hot = x >= 0 and |k - dc_bin| > dc_guard
//   closed   = hot, or hot bins a < k < b with b - a - 1 <= gap;  mask byte: bit 0 hot, bit 1 closed
//   a run is a maximal stretch [lo, hi] of closed bins; its record (int64[8]): lo, hi, the hot count, the lowest index of the
//   maximum of e = mean - fmean, e there, sum w, sum w (k - lo) with w = max(e, 0), max_k (max - fmax); kept iff the hot
//   count >= min_hot
//   on[j][s] = sum_{k = lo .. hi} (slice[s][k] - T_s fmean[k]) >= T_s (hi - lo + 1) thr_act      (int64; T_s = min(T, F - s T))
//
// k_find_accumulate: one thread per bin walks the batch's frames in order (a wave reads 64 consecutive floats of a row); the
// slice sum is kept in a register and flushed when the frame's slice changes.
// k_find_floor: a workgroup owns FD_TILE bins and stages them and h neighbours on either side in LDS as halfwords (the planes
// are centi-dB within +-30000); each thread finds its order statistic by a binary search over the 2^16 halfword values,
// counting the window's values <= mid: 16 passes, no sort, no per-thread array.
// k_find_mask: the hot bits of a tile and gap + 1 neighbours on either side in LDS; a bin is closed when the nearest hot bins
// on its two sides are no more than gap cold bins apart.
// k_find_runs: the thread of a run's first bin walks it and appends the record through one atomic counter.
// k_find_activity: one wave per (run, slice); lanes stride over the run's bins, add in int64, integer butterfly.
#include "common.h"

namespace iqa {

constexpr int FD_THREADS = 256;
constexpr int FD_WAVES = FD_THREADS / kWave;
constexpr int FD_TILE = FD_THREADS;  // bins of one workgroup of the floor and mask kernels: one per thread
constexpr int FD_C_MIN = IQA_FIND_C_MIN, FD_C_MAX = -IQA_FIND_C_MIN;
constexpr int FD_RECORD = 8;

// ---- accumulate ---------------------------------------------------------------------------------------------------------

struct FindAccArgs {
    const float *rows;   // [n_frames][nbins]
    long long *sum;      // [nbins]
    int *max;            // [nbins]
    int *slice;          // [S][nbins]
    short *c_out;        // [n_frames][nbins] or NULL
    long long first;     // the run's index of rows[0]
    int n_frames, nbins, T;
};

__device__ __forceinline__ int fd_quantise(float row)
{
    const float x = rintf(100.0f * row);  // (NaN fails both comparisons below and is sent to the bottom)
    return x >= static_cast<float>(FD_C_MAX) ? FD_C_MAX : (x > static_cast<float>(FD_C_MIN) ? static_cast<int>(x) : FD_C_MIN);
}

__global__ __launch_bounds__(FD_THREADS) void k_find_accumulate(FindAccArgs g)
{
    const int k = blockIdx.x * FD_THREADS + threadIdx.x;
    if (k >= g.nbins) return;
    long long total = 0, s = g.first / g.T;
    int left = g.T - static_cast<int>(g.first % g.T);  // frames until the slice changes
    int most = FD_C_MIN, part = 0;
    for (int f = 0; f < g.n_frames; ++f) {
        const long long at = static_cast<long long>(f) * g.nbins + k;
        const int c = fd_quantise(g.rows[at]);
        if (g.c_out) g.c_out[at] = static_cast<short>(c);
        total += c;
        most = max(most, c);
        part += c;
        if (--left == 0) {
            g.slice[s * g.nbins + k] += part;
            part = 0, left = g.T, ++s;
        }
    }
    if (left != g.T) g.slice[s * g.nbins + k] += part;  // (the batch ended inside slice s)
    g.sum[k] += total;
    g.max[k] = max(g.max[k], most);
}

__global__ __launch_bounds__(FD_THREADS) void k_find_mean(const long long *__restrict__ sum, int nbins, long long F, int *__restrict__ mean)
{
    const int k = blockIdx.x * FD_THREADS + threadIdx.x;
    if (k >= nbins) return;
    const long long v = sum[k];
    long long q = v / F;
    if (v % F != 0 && v < 0) --q;  // floor, not truncation
    mean[k] = static_cast<int>(q);
}

// ---- the local floor ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(FD_THREADS) void k_find_floor(const int *__restrict__ plane, int nbins, int h, int num, int den,
                                                           int *__restrict__ out)
{
    extern __shared__ short s_v[];  // s_v[i] = plane[t0 - h + i], i < FD_TILE + 2 h
    const int tid = threadIdx.x, t0 = blockIdx.x * FD_TILE;
    for (int i = tid; i < FD_TILE + 2 * h; i += FD_THREADS) {
        const int b = t0 - h + i;
        s_v[i] = (b >= 0 && b < nbins) ? static_cast<short>(min(max(plane[b], -32768), 32767)) : static_cast<short>(0);
    }
    __syncthreads();
    const int k = t0 + tid;
    if (k >= nbins) return;
    const int lo = max(0, k - h), hi = min(nbins - 1, k + h);
    const int rank = static_cast<int>((static_cast<long long>(hi - lo) * num) / den);
    const short *w = s_v + (lo - (t0 - h));
    const int len = hi - lo + 1;
    int a = -32768, b = 32767;  // the answer is the least v with more than `rank` values <= v
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        int count = 0;
        for (int i = 0; i < len; ++i) count += w[i] <= mid ? 1 : 0;
        if (count > rank) b = mid;
        else a = mid + 1;
    }
    out[k] = a;
}

// ---- the mask -----------------------------------------------------------------------------------------------------------

struct FindMaskArgs {
    const int *mean, *fmean, *max, *fmax;  // [nbins]
    int *x;                                // [nbins]
    unsigned char *mask;                   // [nbins]
    int nbins, thr, thr_peak, gap, dc_bin, dc_guard;
};

__global__ __launch_bounds__(FD_THREADS) void k_find_mask(FindMaskArgs g)
{
    __shared__ unsigned char s_hot[FD_TILE + 2 * (IQA_FIND_MAX_GAP + 1)];
    const int tid = threadIdx.x, t0 = blockIdx.x * FD_TILE, reach = g.gap + 1;
    for (int i = tid; i < FD_TILE + 2 * reach; i += FD_THREADS) {
        const int b = t0 - reach + i;
        unsigned char hot = 0;
        if (b >= 0 && b < g.nbins) {
            const int x = max(g.mean[b] - g.fmean[b] - g.thr, g.max[b] - g.fmax[b] - g.thr_peak);
            const int d = b > g.dc_bin ? b - g.dc_bin : g.dc_bin - b;
            hot = (x >= 0 && d > g.dc_guard) ? 1 : 0;
            if (i >= reach && i < reach + FD_TILE) g.x[b] = x;
        }
        s_hot[i] = hot;
    }
    __syncthreads();
    const int k = t0 + tid;
    if (k >= g.nbins) return;
    const unsigned char *p = s_hot + reach + tid;
    int closed = p[0];
    if (!closed) {
        int l = 0, r = 0;  // the distances of the nearest hot bins, 0 = none within reach
        for (int d = 1; d <= reach; ++d) {
            if (!l && p[-d]) l = d;
            if (!r && p[d]) r = d;
        }
        closed = (l && r && l + r - 1 <= g.gap) ? 1 : 0;
    }
    g.mask[k] = static_cast<unsigned char>(p[0] | (closed << 1));
}

// ---- the runs -----------------------------------------------------------------------------------------------------------

struct FindRunsArgs {
    const int *mean, *fmean, *max, *fmax;  // [nbins]
    const unsigned char *mask;             // [nbins]
    long long *list;                       // [capacity][8]
    long long capacity;
    unsigned long long *counts;            // [2]: kept runs; all runs
    int nbins, min_hot;
};

__global__ __launch_bounds__(FD_THREADS) void k_find_runs(FindRunsArgs g)
{
    const int lo = blockIdx.x * FD_THREADS + threadIdx.x;
    if (lo >= g.nbins || !(g.mask[lo] & 2) || (lo > 0 && (g.mask[lo - 1] & 2))) return;
    int hot = 0, peak = lo, e_peak = g.mean[lo] - g.fmean[lo], over = g.max[lo] - g.fmax[lo], k = lo;
    long long sw = 0, swk = 0;
    for (; k < g.nbins; ++k) {
        const unsigned char m = g.mask[k];
        if (!(m & 2)) break;
        hot += m & 1;
        const int e = g.mean[k] - g.fmean[k];
        if (e > e_peak) e_peak = e, peak = k;
        const long long w = e > 0 ? e : 0;
        sw += w;
        swk += w * (k - lo);
        over = max(over, g.max[k] - g.fmax[k]);
    }
    atomicAdd(g.counts + 1, 1ULL);
    if (hot < g.min_hot) return;
    const unsigned long long at = atomicAdd(g.counts, 1ULL);
    if (at >= static_cast<unsigned long long>(g.capacity)) return;
    long long *rec = g.list + FD_RECORD * at;
    rec[0] = lo, rec[1] = k - 1, rec[2] = hot, rec[3] = peak, rec[4] = e_peak, rec[5] = sw, rec[6] = swk, rec[7] = over;
}

// ---- the activity -------------------------------------------------------------------------------------------------------

struct FindActArgs {
    const int *slice;       // [S][nbins]
    const int *fmean;       // [nbins]
    const long long *list;  // [J][8]
    unsigned char *on;      // [J][S]
    long long J, F;
    int nbins, T, S, thr_act;
};

__global__ __launch_bounds__(FD_THREADS) void k_find_activity(FindActArgs g)
{
    const int lane = threadIdx.x % kWave;
    const long long job = static_cast<long long>(blockIdx.x) * FD_WAVES + threadIdx.x / kWave;  // (wave-uniform)
    if (job >= g.J * g.S) return;
    const long long j = job / g.S;
    const int s = static_cast<int>(job % g.S);
    const long long lo = g.list[FD_RECORD * j], hi = g.list[FD_RECORD * j + 1];
    if (lo < 0 || hi >= g.nbins || lo > hi) {  // (not a run of this plane: nothing is read)
        if (lane == 0) g.on[job] = 0;
        return;
    }
    const long long left = g.F - static_cast<long long>(s) * g.T, Ts = left < g.T ? left : g.T;
    const int *row = g.slice + static_cast<long long>(s) * g.nbins;
    long long total = 0;
    for (long long k = lo + lane; k <= hi; k += kWave) total += row[k] - Ts * g.fmean[k];
    total = wave_sum(total);
    if (lane == 0) g.on[job] = total >= Ts * (hi - lo + 1) * g.thr_act ? 1 : 0;
}

static_assert((FD_TILE + 2 * IQA_FIND_MAX_HALF) * 2 <= 64 * 1024, "a floor tile and its neighbours must fit the default LDS allowance");
static_assert(static_cast<long long>(IQA_FIND_MAX_SLICE_FRAMES) * FD_C_MAX < (1LL << 31), "a slice sum stays inside int32");
static_assert(FD_C_MAX <= 32767 && FD_C_MIN >= -32768, "the planes fit the floor kernel's halfwords");
static_assert(2LL * IQA_FIND_MAX_HALF * 65536 < (1LL << 31), "the rank's product is formed in int64 all the same");

}  // namespace iqa

using namespace iqa;

constexpr int FD_MAX_BINS = 1 << 24;

extern "C" int iqa_find_accumulate(const void *rows_dev, int32_t n_frames, int32_t nbins, int64_t first_frame, int32_t slice_frames,
                                   int32_t n_slices, void *sum_dev, void *max_dev, void *slice_dev, void *c_out_dev, void *stream)
{
    if (n_frames < 0 || nbins < 0 || first_frame < 0) return fail_inval("negative length or position");
    if (nbins > FD_MAX_BINS) return fail_inval("nbins out of range");
    if (slice_frames < 1 || slice_frames > IQA_FIND_MAX_SLICE_FRAMES) return fail_inval("slice_frames must be 1 .. IQA_FIND_MAX_SLICE_FRAMES");
    if (n_slices < 1) return fail_inval("n_slices must be at least 1");
    if (first_frame > static_cast<int64_t>(n_slices) * slice_frames - n_frames) return fail_inval("frames reach past the last slice");
    if (n_frames == 0 || nbins == 0) return IQA_OK;
    if (!rows_dev || !sum_dev || !max_dev || !slice_dev) return fail_inval("NULL device pointer");
    FindAccArgs g;
    g.rows = static_cast<const float *>(rows_dev);
    g.sum = static_cast<long long *>(sum_dev);
    g.max = static_cast<int *>(max_dev);
    g.slice = static_cast<int *>(slice_dev);
    g.c_out = static_cast<short *>(c_out_dev);
    g.first = first_frame;
    g.n_frames = n_frames;
    g.nbins = nbins;
    g.T = slice_frames;
    hipLaunchKernelGGL(k_find_accumulate, grid1d(nbins, FD_THREADS), dim3(FD_THREADS), 0, as_stream(stream), g);
    return check_launch("k_find_accumulate");
}

extern "C" int iqa_find_mean(const void *sum_dev, int32_t nbins, int64_t frames, void *mean_out_dev, void *stream)
{
    if (nbins < 0) return fail_inval("negative length");
    if (nbins > FD_MAX_BINS) return fail_inval("nbins out of range");
    if (frames < 1) return fail_inval("frames must be at least 1");
    if (nbins == 0) return IQA_OK;
    if (!sum_dev || !mean_out_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_find_mean, grid1d(nbins, FD_THREADS), dim3(FD_THREADS), 0, as_stream(stream),
                       static_cast<const long long *>(sum_dev), static_cast<int>(nbins), static_cast<long long>(frames),
                       static_cast<int *>(mean_out_dev));
    return check_launch("k_find_mean");
}

extern "C" int iqa_find_floor(const void *plane_dev, int32_t nbins, int32_t half, int32_t num, int32_t den, void *floor_out_dev,
                              void *stream)
{
    if (nbins < 0) return fail_inval("negative length");
    if (nbins > FD_MAX_BINS) return fail_inval("nbins out of range");
    if (half < 0 || half > IQA_FIND_MAX_HALF) return fail_inval("half must be 0 .. IQA_FIND_MAX_HALF");
    if (den < 1 || den > 65536 || num < 0 || num > den) return fail_inval("the rank fraction needs 0 <= num <= den, 1 <= den <= 65536");
    if (nbins == 0) return IQA_OK;
    if (!plane_dev || !floor_out_dev) return fail_inval("NULL device pointer");
    const int h = half < nbins ? half : nbins;  // (a window wider than the plane is the plane: less to stage, the same values)
    hipLaunchKernelGGL(k_find_floor, grid1d(nbins, FD_TILE), dim3(FD_THREADS), static_cast<size_t>(FD_TILE + 2 * h) * sizeof(short),
                       as_stream(stream), static_cast<const int *>(plane_dev), static_cast<int>(nbins), h, static_cast<int>(num),
                       static_cast<int>(den), static_cast<int *>(floor_out_dev));
    return check_launch("k_find_floor");
}

extern "C" int iqa_find_mask(const void *mean_dev, const void *fmean_dev, const void *max_dev, const void *fmax_dev, int32_t nbins,
                             int32_t thr, int32_t thr_peak, int32_t gap, int32_t dc_bin, int32_t dc_guard, void *x_out_dev,
                             void *mask_out_dev, void *stream)
{
    if (nbins < 0) return fail_inval("negative length");
    if (nbins > FD_MAX_BINS) return fail_inval("nbins out of range");
    if (gap < 0 || gap > IQA_FIND_MAX_GAP) return fail_inval("gap must be 0 .. IQA_FIND_MAX_GAP");
    if (thr <= -(1 << 20) || thr >= (1 << 20) || thr_peak <= -(1 << 20) || thr_peak >= (1 << 20)) return fail_inval("a threshold must stay inside +-2^20");
    if (dc_bin < 0 || dc_bin > FD_MAX_BINS) return fail_inval("dc_bin out of range");
    if (nbins == 0) return IQA_OK;
    if (!mean_dev || !fmean_dev || !max_dev || !fmax_dev || !x_out_dev || !mask_out_dev) return fail_inval("NULL device pointer");
    FindMaskArgs g;
    g.mean = static_cast<const int *>(mean_dev);
    g.fmean = static_cast<const int *>(fmean_dev);
    g.max = static_cast<const int *>(max_dev);
    g.fmax = static_cast<const int *>(fmax_dev);
    g.x = static_cast<int *>(x_out_dev);
    g.mask = static_cast<unsigned char *>(mask_out_dev);
    g.nbins = nbins;
    g.thr = thr;
    g.thr_peak = thr_peak;
    g.gap = gap;
    g.dc_bin = dc_bin;
    g.dc_guard = dc_guard < 0 ? -1 : dc_guard;
    hipLaunchKernelGGL(k_find_mask, grid1d(nbins, FD_TILE), dim3(FD_THREADS), 0, as_stream(stream), g);
    return check_launch("k_find_mask");
}

extern "C" int iqa_find_runs(const void *mean_dev, const void *fmean_dev, const void *max_dev, const void *fmax_dev, const void *mask_dev,
                             int32_t nbins, int32_t min_hot, void *list_dev, int64_t capacity, void *counts_dev, void *stream)
{
    if (nbins < 0 || capacity < 0) return fail_inval("negative length");
    if (nbins > FD_MAX_BINS) return fail_inval("nbins out of range");
    if (min_hot < 1) return fail_inval("min_hot must be at least 1");
    if (!counts_dev) return fail_inval("NULL device pointer");
    if (nbins > 0 && (!mean_dev || !fmean_dev || !max_dev || !fmax_dev || !mask_dev || (capacity > 0 && !list_dev))) return fail_inval("NULL device pointer");
    if (hipMemsetAsync(counts_dev, 0, 2 * sizeof(long long), as_stream(stream)) != hipSuccess) {  // (behind every check)
        set_error("clearing the run counts failed");
        return IQA_EHIP;
    }
    if (nbins == 0) return IQA_OK;
    FindRunsArgs g;
    g.mean = static_cast<const int *>(mean_dev);
    g.fmean = static_cast<const int *>(fmean_dev);
    g.max = static_cast<const int *>(max_dev);
    g.fmax = static_cast<const int *>(fmax_dev);
    g.mask = static_cast<const unsigned char *>(mask_dev);
    g.list = static_cast<long long *>(list_dev);
    g.capacity = capacity;
    g.counts = static_cast<unsigned long long *>(counts_dev);
    g.nbins = nbins;
    g.min_hot = min_hot;
    hipLaunchKernelGGL(k_find_runs, grid1d(nbins, FD_THREADS), dim3(FD_THREADS), 0, as_stream(stream), g);
    return check_launch("k_find_runs");
}

extern "C" int iqa_find_activity(const void *slice_dev, const void *fmean_dev, const void *list_dev, int64_t n_runs, int32_t nbins,
                                 int64_t frames, int32_t slice_frames, int32_t n_slices, int32_t thr_act, void *on_out_dev, void *stream)
{
    if (n_runs < 0 || nbins < 0) return fail_inval("negative length");
    if (nbins > FD_MAX_BINS || n_runs > FD_MAX_BINS) return fail_inval("length out of range");
    if (slice_frames < 1 || slice_frames > IQA_FIND_MAX_SLICE_FRAMES) return fail_inval("slice_frames must be 1 .. IQA_FIND_MAX_SLICE_FRAMES");
    if (n_slices < 1 || n_slices > (1 << 20)) return fail_inval("n_slices must be 1 .. 2^20");
    if (frames > static_cast<int64_t>(n_slices) * slice_frames || frames <= static_cast<int64_t>(n_slices - 1) * slice_frames)
        return fail_inval("n_slices must be ceil(frames / slice_frames)");
    if (thr_act <= -(1 << 20) || thr_act >= (1 << 20)) return fail_inval("a threshold must stay inside +-2^20");
    if (n_runs * n_slices > (1LL << 31)) return fail_inval("n_runs n_slices out of range");
    if (n_runs == 0 || nbins == 0) return IQA_OK;
    if (!slice_dev || !fmean_dev || !list_dev || !on_out_dev) return fail_inval("NULL device pointer");
    FindActArgs g;
    g.slice = static_cast<const int *>(slice_dev);
    g.fmean = static_cast<const int *>(fmean_dev);
    g.list = static_cast<const long long *>(list_dev);
    g.on = static_cast<unsigned char *>(on_out_dev);
    g.J = n_runs;
    g.F = frames;
    g.nbins = nbins;
    g.T = slice_frames;
    g.S = n_slices;
    g.thr_act = thr_act;
    hipLaunchKernelGGL(k_find_activity, grid1d(n_runs * n_slices, FD_WAVES), dim3(FD_THREADS), 0, as_stream(stream), g);
    return check_launch("k_find_activity");
}
