// squelch.hip -- the reference's audio post-processing (automatic squelch) as one segmented launch sequence.
//
// Replaces reference src/iq_to_audio/squelch.py:20-255 (apply_squelch and its helpers).  One call processes a
// batch of files ("segments") of different lengths, channel counts, sample rates and windows.  Every per-sample
// array lives in the workspace at the segment's tile-aligned `base`, so a workgroup (one SQ_TILE of samples) never
// straddles two files; per-tile partials go through a per-segment scan, then the tile applies its carry.
//
//   moving averages  -> float64 prefix sums of the channel-mean magnitude (exact windows, any w)
//   np.percentile    -> exact radix select (11/11/10 bits) of the two neighbouring order statistics, numpy's _lerp
//   minimum.accumulate -> segmented min-scan
//   _dilate_mask     -> int32 window counts from a prefix count, with the reference's int8 wrap
//   _smooth_gain     -> integer triangular window sums from prefix sums of d[p] and p*d[p]
//   _apply_trim      -> per-segment atomic min/max of the active index, bounds on the device
//
// Nothing is read back inside the sequence: order statistics and bounds are consumed from device memory.
#include "common.h"

#include <climits>

// numpy evaluates the float32 parts of the chain one rounded operation at a time
#pragma clang fp contract(off)

namespace iqa {
namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_ITEMS = 8;
constexpr int SQ_TILE = SQ_THREADS * SQ_ITEMS;
static_assert(SQ_TILE == IQA_SQ_TILE, "tile size");
constexpr int SQ_BINS = 2048;
constexpr int SQ_QUERIES = 6;  // 0,1: noise floor; 2,3: 5th percentile; 4,5: 95th percentile (prev / next index)

struct SelState {
    unsigned key[SQ_QUERIES];
    int rank[SQ_QUERIES];
    float value[SQ_QUERIES];
    float thr32, lo32, hi32, low, span;
    int any_above, first, last;
};

struct Work {
    float *mag;  // channel-mean magnitude, later the gain
    double *pre;  // inclusive prefix of mag, later (as long long) the prefix of p * dilated[p]
    float *env, *rel, *thr;
    unsigned char *mask, *dil;
    int *cm, *cd;
    long long *ta, *tb, *tc, *td;  // per-tile partials / carries (8 bytes each; reinterpreted per pass)
    unsigned *hist;  // [seg][query][bin]
    SelState *sel;
};

inline long long align_up(long long v) { return (v + 255) & ~255LL; }

// byte offsets of the workspace arrays, in declaration order of Work
void layout(long long np, int nseg, long long off[13], long long *total)
{
    const long long nt = np / SQ_TILE;
    const long long sizes[13] = {4 * np, 8 * np, 4 * np, 4 * np, 4 * np, np, np, 4 * np, 4 * np,
                                 8 * nt * 4, 0, 4LL * nseg * SQ_QUERIES * SQ_BINS, (long long)sizeof(SelState) * nseg};
    long long o = 0;
    for (int k = 0; k < 13; ++k) {
        off[k] = o;
        o += align_up(sizes[k]);
    }
    *total = o;
}

Work carve(void *ws, long long np, int nseg)
{
    long long off[13], total;
    layout(np, nseg, off, &total);
    char *b = static_cast<char *>(ws);
    const long long nt = np / SQ_TILE;
    Work w;
    w.mag = reinterpret_cast<float *>(b + off[0]);
    w.pre = reinterpret_cast<double *>(b + off[1]);
    w.env = reinterpret_cast<float *>(b + off[2]);
    w.rel = reinterpret_cast<float *>(b + off[3]);
    w.thr = reinterpret_cast<float *>(b + off[4]);
    w.mask = reinterpret_cast<unsigned char *>(b + off[5]);
    w.dil = reinterpret_cast<unsigned char *>(b + off[6]);
    w.cm = reinterpret_cast<int *>(b + off[7]);
    w.cd = reinterpret_cast<int *>(b + off[8]);
    w.ta = reinterpret_cast<long long *>(b + off[9]);
    w.tb = w.ta + nt;
    w.tc = w.tb + nt;
    w.td = w.tc + nt;
    w.hist = reinterpret_cast<unsigned *>(b + off[11]);
    w.sel = reinterpret_cast<SelState *>(b + off[12]);
    return w;
}

// ---------------------------------------------------------------------------------------------------------------
// helpers

__device__ __forceinline__ int seg_of_tile(const iqa_squelch_seg *segs, int nseg, long long tile)
{
    int lo = 0, hi = nseg - 1;  // last segment whose first tile <= tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].base / SQ_TILE <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct SumOp {
    template <class T> __device__ static T op(T a, T b) { return a + b; }
};
struct MinOp {
    __device__ static float op(float a, float b) { return fminf(a, b); }
};

// exclusive block scan of one value per thread (256 threads); *total gets the block's total
template <class T, class Op>
__device__ T block_exclusive(T v, T identity, T *total)
{
    __shared__ T wtot[SQ_THREADS / kWave];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    T inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T u = __shfl_up(inc, o, kWave);
        if (lane >= o) inc = Op::op(u, inc);
    }
    if (lane == kWave - 1) wtot[wid] = inc;
    __syncthreads();
    T before = identity, all = identity;
#pragma unroll
    for (int k = 0; k < SQ_THREADS / kWave; ++k) {
        if (k < wid) before = Op::op(before, wtot[k]);
        all = Op::op(all, wtot[k]);
    }
    T ex = __shfl_up(inc, 1, kWave);
    if (lane == 0) ex = identity;
    __syncthreads();  // wtot may be reused by the caller's next scan
    *total = all;
    return Op::op(before, ex);
}

__device__ __forceinline__ float dbfs(float x)  // ref: squelch.py _dbfs
{
    const double v = fmax(static_cast<double>(x), 1e-10);
    return static_cast<float>(fmax(-160.0, 20.0 * log10(v)));
}

__device__ __forceinline__ unsigned f2key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// numpy 2.2 _lerp in float32 (function_base: a + (b-a)*t, or b - (b-a)*(1-t) where t >= 0.5)
__device__ __forceinline__ float np_lerp(float a, float b, float t)
{
    const float d = b - a;
    if (t >= 0.5f) return b - d * (1.0f - t);
    return a + d * t;
}

// ---------------------------------------------------------------------------------------------------------------
// kernels

__global__ __launch_bounds__(SQ_THREADS) void k_sq_init(const iqa_squelch_seg *segs, Work w)
{
    const int s = blockIdx.x;
    unsigned *h = w.hist + static_cast<long long>(s) * SQ_QUERIES * SQ_BINS;
    for (int k = threadIdx.x; k < SQ_QUERIES * SQ_BINS; k += SQ_THREADS) h[k] = 0;
    if (threadIdx.x == 0) {
        SelState &st = w.sel[s];
        for (int q = 0; q < SQ_QUERIES; ++q) {
            st.key[q] = 0;
            st.rank[q] = static_cast<int>(segs[s].q_index[q]);
            st.value[q] = 0.0f;
        }
        st.any_above = 0;
        st.first = INT_MAX;
        st.last = -1;
    }
}

// mean |x| over channels (float64 -> float32) and the tile's float64 sum.  ref: squelch.py _envelope
__global__ __launch_bounds__(SQ_THREADS) void k_sq_magnitude(const iqa_squelch_seg *segs, int nseg, const float *in, Work w)
{
    const long long t = blockIdx.x;
    const iqa_squelch_seg &sg = segs[seg_of_tile(segs, nseg, t)];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS;
    const int C = sg.channels;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) {
        const long long i = i0 + j;
        float m = 0.0f;
        if (i >= 0 && i < sg.n) {
            const float *x = in + sg.in_off + i * C;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += static_cast<double>(fabsf(x[c]));
            m = static_cast<float>(s / C);
        }
        w.mag[t * SQ_TILE + threadIdx.x * SQ_ITEMS + j] = m;
        acc += m;
    }
    double tot;
    block_exclusive<double, SumOp>(acc, 0.0, &tot);
    if (threadIdx.x == 0) reinterpret_cast<double *>(w.ta)[t] = tot;
}

// per-segment exclusive scan of per-tile partials (one workgroup per segment, up to two arrays: blockIdx.y)
template <class T, class Op>
__global__ __launch_bounds__(SQ_THREADS) void k_sq_tile_scan(const iqa_squelch_seg *segs, const T *in0, T *out0,
                                                              const T *in1, T *out1, T identity)
{
    const iqa_squelch_seg &sg = segs[blockIdx.x];
    const T *in = blockIdx.y ? in1 : in0;
    T *out = blockIdx.y ? out1 : out0;
    const long long t0 = sg.base / SQ_TILE, nt = (sg.n + SQ_TILE - 1) / SQ_TILE;
    T carry = identity;
    for (long long k = 0; k < nt; k += SQ_THREADS) {
        const long long idx = k + threadIdx.x;
        const T v = idx < nt ? in[t0 + idx] : identity;
        T tot;
        const T ex = block_exclusive<T, Op>(v, identity, &tot);
        if (idx < nt) out[t0 + idx] = Op::op(carry, ex);
        carry = Op::op(carry, tot);
    }
}

// inclusive float64 prefix of the magnitude
__global__ __launch_bounds__(SQ_THREADS) void k_sq_prefix(Work w)
{
    const long long t = blockIdx.x, e0 = t * SQ_TILE + threadIdx.x * SQ_ITEMS;
    double v[SQ_ITEMS], s = 0.0;
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) {
        s += static_cast<double>(w.mag[e0 + j]);
        v[j] = s;
    }
    double tot;
    const double ex = block_exclusive<double, SumOp>(s, 0.0, &tot) + reinterpret_cast<const double *>(w.tb)[t];
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) w.pre[e0 + j] = ex + v[j];
}

// box average of w taps centred as np.convolve(mode="same"): sum a[i - w//2 .. i - w//2 + w - 1] / w, zero outside
__device__ __forceinline__ float box(const double *pre, const float *mag, long long i, long long n, int win)
{
    if (win == 1) return mag[i];
    long long lo = i - win / 2, hi = lo + win;  // [lo, hi)
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    const double s = (hi > 0 ? pre[hi - 1] : 0.0) - (lo > 0 ? pre[lo - 1] : 0.0);
    return static_cast<float>(s / win);
}

// envelope dB (and for "transient" its short/long difference and mask); per-tile min of the envelope dB
__global__ __launch_bounds__(SQ_THREADS) void k_sq_envelope(const iqa_squelch_seg *segs, int nseg, int method,
                                                             float tmargin, Work w)
{
    const long long t = blockIdx.x;
    const iqa_squelch_seg &sg = segs[seg_of_tile(segs, nseg, t)];
    const long long b = sg.base, n = sg.n;
    const long long i0 = t * SQ_TILE - b + threadIdx.x * SQ_ITEMS;
    const double *pre = w.pre + b;
    const float *mag = w.mag + b;
    float mn = INFINITY;
    for (int j = 0; j < SQ_ITEMS; ++j) {
        const long long i = i0 + j;
        if (i >= n) break;
        const float db = dbfs(box(pre, mag, i, n, sg.window));
        w.env[b + i] = db;
        mn = fminf(mn, db);
        if (method == IQA_SQ_TRANSIENT) {  // ref: squelch.py _transient_mask
            const float es = box(pre, mag, i, n, sg.short_window);
            const float el = box(pre, mag, i, n, sg.long_window);
            const float diff = dbfs(es) - dbfs(el + 1e-10f);
            w.rel[b + i] = diff;
            w.thr[b + i] = tmargin;
            w.mask[b + i] = diff >= tmargin;
        }
    }
    float tot;
    block_exclusive<float, MinOp>(mn, INFINITY, &tot);
    if (threadIdx.x == 0) reinterpret_cast<float *>(w.tc)[t] = tot;
}

// one radix-select pass: histogram of the `shift` digit of the values whose higher digits equal the query's prefix
__global__ __launch_bounds__(SQ_THREADS) void k_sq_select_hist(const iqa_squelch_seg *segs, int nseg, const float *vals,
                                                                Work w, int q0, int nq, int shift)
{
    __shared__ unsigned lh[4 * SQ_BINS];
    for (int k = threadIdx.x; k < nq * SQ_BINS; k += SQ_THREADS) lh[k] = 0;
    const long long t = blockIdx.x;
    const int s = seg_of_tile(segs, nseg, t);
    const iqa_squelch_seg &sg = segs[s];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS;
    // digits: bits 21..31, 10..20, 0..9; the digits above `shift` are already fixed by the query's prefix
    const unsigned hi_mask = shift == 21 ? 0u : shift == 10 ? 0xFFE00000u : 0xFFFFFC00u;
    const unsigned bin_mask = shift == 0 ? (SQ_BINS / 2 - 1) : (SQ_BINS - 1);
    unsigned keys[SQ_ITEMS];
    int cnt = 0;
    for (int j = 0; j < SQ_ITEMS; ++j) {
        if (i0 + j < sg.n) keys[cnt++] = f2key(vals[sg.base + i0 + j]);
    }
    __syncthreads();
    for (int q = 0; q < nq; ++q) {
        const unsigned prefix = w.sel[s].key[q0 + q];
        unsigned run_bin = 0, run = 0;  // consecutive samples mostly share a digit: one LDS atomic per run
        for (int j = 0; j < cnt; ++j) {
            if ((keys[j] & hi_mask) != prefix) continue;
            const unsigned bin = (keys[j] >> shift) & bin_mask;
            if (run && bin != run_bin) {
                atomicAdd(&lh[q * SQ_BINS + run_bin], run);
                run = 0;
            }
            run_bin = bin;
            ++run;
        }
        if (run) atomicAdd(&lh[q * SQ_BINS + run_bin], run);
    }
    __syncthreads();
    unsigned *gh = w.hist + static_cast<long long>(s) * SQ_QUERIES * SQ_BINS;
    for (int k = threadIdx.x; k < nq * SQ_BINS; k += SQ_THREADS) {
        if (lh[k]) atomicAdd(&gh[q0 * SQ_BINS + k], lh[k]);
    }
}

// pick the digit that holds the query's rank; clear the histogram for the next pass
__global__ __launch_bounds__(SQ_THREADS) void k_sq_select_pick(Work w, int q0, int shift)
{
    const int s = blockIdx.x, q = q0 + blockIdx.y;
    unsigned *h = w.hist + (static_cast<long long>(s) * SQ_QUERIES + q) * SQ_BINS;
    SelState &st = w.sel[s];
    unsigned c[SQ_BINS / SQ_THREADS], sum = 0;
#pragma unroll
    for (int j = 0; j < SQ_BINS / SQ_THREADS; ++j) {
        c[j] = h[threadIdx.x * (SQ_BINS / SQ_THREADS) + j];
        sum += c[j];
    }
    const int rank = st.rank[q];
    unsigned tot;
    unsigned before = block_exclusive<unsigned, SumOp>(sum, 0u, &tot);
    if (static_cast<unsigned>(rank) >= before && static_cast<unsigned>(rank) < before + sum) {
#pragma unroll
        for (int j = 0; j < SQ_BINS / SQ_THREADS; ++j) {
            if (static_cast<unsigned>(rank) < before + c[j]) {
                const unsigned bin = threadIdx.x * (SQ_BINS / SQ_THREADS) + j;
                st.key[q] |= bin << shift;
                st.rank[q] = rank - static_cast<int>(before);
                if (shift == 0) st.value[q] = key2f(st.key[q]);
                break;
            }
            before += c[j];
        }
    }
#pragma unroll
    for (int j = 0; j < SQ_BINS / SQ_THREADS; ++j) h[threadIdx.x * (SQ_BINS / SQ_THREADS) + j] = 0;
}

// noise floor (percentile or manual) and threshold.  ref: squelch.py resolve_noise_floor, apply_squelch
__global__ void k_sq_floor(const iqa_squelch_seg *segs, int nseg, int auto_floor, double margin, Work w, iqa_squelch_result *res)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    SelState &st = w.sel[s];
    const double floor_db = auto_floor ? static_cast<double>(np_lerp(st.value[0], st.value[1], segs[s].q_gamma[0]))
                                       : segs[s].manual_floor_db;
    const double thr = floor_db + margin;
    st.thr32 = static_cast<float>(thr);
    st.lo32 = static_cast<float>(thr - 6.0);
    st.hi32 = static_cast<float>(thr + 6.0);
    res[s].noise_floor_db = floor_db;
    res[s].threshold_db = thr;
}

__device__ __forceinline__ void tile_count(long long cnt, long long t, long long *dst)
{
    long long tot;
    block_exclusive<long long, SumOp>(cnt, 0LL, &tot);
    if (threadIdx.x == 0) dst[t] = tot;
}

// static mask (envelope >= threshold).  ref: squelch.py _static_mask
__global__ __launch_bounds__(SQ_THREADS) void k_sq_mask_static(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const long long t = blockIdx.x;
    const int s = seg_of_tile(segs, nseg, t);
    const iqa_squelch_seg &sg = segs[s];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS;
    const float thr = w.sel[s].thr32;
    long long cnt = 0;
    for (int j = 0; j < SQ_ITEMS && i0 + j < sg.n; ++j) {
        const long long e = sg.base + i0 + j;
        const bool m = w.env[e] >= thr;
        w.mask[e] = m;
        w.thr[e] = thr;
        cnt += m;
    }
    tile_count(cnt, t, w.ta);
}

// per-tile mask counts of the transient mask (made by k_sq_envelope)
__global__ __launch_bounds__(SQ_THREADS) void k_sq_mask_count(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const long long t = blockIdx.x;
    const iqa_squelch_seg &sg = segs[seg_of_tile(segs, nseg, t)];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS;
    long long cnt = 0;
    for (int j = 0; j < SQ_ITEMS && i0 + j < sg.n; ++j) cnt += w.mask[sg.base + i0 + j];
    tile_count(cnt, t, w.ta);
}

// relative = envelope - minimum.accumulate(envelope); any(envelope >= threshold).  ref: squelch.py _adaptive_mask
__global__ __launch_bounds__(SQ_THREADS) void k_sq_relative(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const long long t = blockIdx.x;
    const int s = seg_of_tile(segs, nseg, t);
    const iqa_squelch_seg &sg = segs[s];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS;
    const float thr = w.sel[s].thr32;
    float v[SQ_ITEMS], run = INFINITY;
    int above = 0;
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) {
        v[j] = i0 + j < sg.n ? w.env[sg.base + i0 + j] : INFINITY;
        run = fminf(run, v[j]);
        above |= v[j] >= thr && i0 + j < sg.n;
    }
    float tot;
    float base = fminf(block_exclusive<float, MinOp>(run, INFINITY, &tot), reinterpret_cast<const float *>(w.td)[t]);
    if (__syncthreads_or(above) && threadIdx.x == 0) atomicOr(&w.sel[s].any_above, 1);
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) {
        base = fminf(base, v[j]);
        if (i0 + j < sg.n) w.rel[sg.base + i0 + j] = v[j] - base;
    }
}

// 5th / 95th percentile span of `relative`.  ref: squelch.py _percentile_difference
__global__ void k_sq_span(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    SelState &st = w.sel[s];
    st.low = np_lerp(st.value[2], st.value[3], segs[s].q_gamma[1]);
    const float high = np_lerp(st.value[4], st.value[5], segs[s].q_gamma[2]);
    const float d = high - st.low;
    st.span = 1e-6f > d ? 1e-6f : d;  // max(high - low, 1e-6)
}

// adaptive mask: envelope >= clip(thr + 6 (1 - score), thr - 6, thr + 6), all-false when nothing is above thr
__global__ __launch_bounds__(SQ_THREADS) void k_sq_mask_adaptive(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const long long t = blockIdx.x;
    const int s = seg_of_tile(segs, nseg, t);
    const iqa_squelch_seg &sg = segs[s];
    const SelState &st = w.sel[s];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS;
    long long cnt = 0;
    for (int j = 0; j < SQ_ITEMS && i0 + j < sg.n; ++j) {
        const long long e = sg.base + i0 + j;
        float at = st.thr32;
        bool m = false;
        if (st.any_above) {
            const float score = (w.rel[e] - st.low) / st.span;
            at = fminf(fmaxf(st.thr32 + 6.0f * (1.0f - score), st.lo32), st.hi32);
            m = w.env[e] >= at;
        }
        w.thr[e] = at;
        w.mask[e] = m;
        cnt += m;
    }
    tile_count(cnt, t, w.ta);
}

// inclusive int32 prefix of a 0/1 array; with `px`, also the int64 prefix of i * flag[i]
__global__ __launch_bounds__(SQ_THREADS) void k_sq_count_prefix(const iqa_squelch_seg *segs, int nseg, const unsigned char *flag,
                                                                  const long long *carry, int *cnt_out,
                                                                  const long long *carry_x, long long *px_out)
{
    const long long t = blockIdx.x;
    const iqa_squelch_seg &sg = segs[seg_of_tile(segs, nseg, t)];
    const long long e0 = t * SQ_TILE + threadIdx.x * SQ_ITEMS, i0 = e0 - sg.base;
    int c[SQ_ITEMS], s = 0;
    long long x[SQ_ITEMS], sx = 0;
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) {
        const int f = i0 + j < sg.n ? flag[e0 + j] : 0;
        s += f;
        sx += f ? i0 + j : 0;
        c[j] = s;
        x[j] = sx;
    }
    long long tot;
    const long long ex = block_exclusive<long long, SumOp>(static_cast<long long>(s), 0LL, &tot) + carry[t];
#pragma unroll
    for (int j = 0; j < SQ_ITEMS; ++j) cnt_out[e0 + j] = static_cast<int>(ex + c[j]);
    if (px_out) {
        const long long exx = block_exclusive<long long, SumOp>(sx, 0LL, &tot) + carry_x[t];
#pragma unroll
        for (int j = 0; j < SQ_ITEMS; ++j) px_out[e0 + j] = exx + x[j];
    }
}

// ref: squelch.py _dilate_mask -- np.convolve of int8 arrays accumulates in int8, so a window count c sets the
// sample only when (int8)(c mod 256) > 0; reproduced on purpose
__device__ __forceinline__ bool int8_positive(int c) { return static_cast<signed char>(c & 0xFF) > 0; }

__global__ __launch_bounds__(SQ_THREADS) void k_sq_dilate(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const long long t = blockIdx.x;
    const iqa_squelch_seg &sg = segs[seg_of_tile(segs, nseg, t)];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS, n = sg.n, h = sg.hold;
    const int *cm = w.cm + sg.base;
    long long cnt = 0, sx = 0;
    for (int j = 0; j < SQ_ITEMS && i0 + j < n; ++j) {
        const long long i = i0 + j;
        bool d = w.mask[sg.base + i];
        if (h > 0) {
            const int before = i - h - 1 >= 0 ? cm[i - h - 1] : 0;
            const int tail = cm[i] - before;  // mask count in [i - h, i]
            const long long last = i + h < n - 1 ? i + h : n - 1;
            const int head = cm[last] - (i > 0 ? cm[i - 1] : 0);  // mask count in [i, i + h]
            d = d || int8_positive(tail) || int8_positive(head);
        }
        w.dil[sg.base + i] = d;
        cnt += d;
        sx += d ? i : 0;
    }
    tile_count(cnt, t, w.ta);
    tile_count(sx, t, w.tc);
}

// ref: squelch.py _smooth_gain -- its fade kernel [0, 1/f, .., (f-1)/f, 1, 1, (f-1)/f, .., 1/f] (two ones: the ramp's
// last value and the explicit 1) applied by np.convolve(mode="same") to the edge-padded mask (np.pad mode="edge")
// weighs sample p by (f + 1 - (i - p)) / f for p in [i - f, i - 1] and by (f - (p - i)) / f for p in [i, i + f];
// then clip to [0, 1].  Exact in integers.  Active span (gain > 1e-3) for _apply_trim.
__global__ __launch_bounds__(SQ_THREADS) void k_sq_gain(const iqa_squelch_seg *segs, int nseg, Work w)
{
    const long long t = blockIdx.x;
    const int s = seg_of_tile(segs, nseg, t);
    const iqa_squelch_seg &sg = segs[s];
    const long long i0 = t * SQ_TILE - sg.base + threadIdx.x * SQ_ITEMS, n = sg.n, f = sg.fade;
    const int *cd = w.cd + sg.base;
    const long long *px = reinterpret_cast<const long long *>(w.pre) + sg.base;
    const unsigned char *dil = w.dil + sg.base;
    int first = INT_MAX, last = -1;
    for (int j = 0; j < SQ_ITEMS && i0 + j < n; ++j) {
        const long long i = i0 + j;
        float g;
        if (f <= 0) {
            g = dil[i];
        } else {
            auto C = [&](long long k) -> long long { return k >= 0 ? cd[k] : 0; };
            auto X = [&](long long k) -> long long { return k >= 0 ? px[k] : 0; };
            const long long a = i - f > 0 ? i - f : 0;  // left: p in [a, i - 1], weight f + 1 - i + p
            long long W = (f + 1 - i) * (C(i - 1) - C(a - 1)) + (X(i - 1) - X(a - 1));
            const long long b = i + f < n - 1 ? i + f : n - 1;  // right: p in [i, b], weight f + i - p
            W += (f + i) * (C(b) - C(i - 1)) - (X(b) - X(i - 1));
            if (i - f < 0) W += dil[0] * ((f - i) * (f - i + 1) / 2);  // p in [i - f, -1] repeat d[0]
            if (i + f > n - 1) W += dil[n - 1] * ((f + i - n) * (f + i - n + 1) / 2);  // p in [n, i + f] repeat d[n - 1]
            g = fminf(static_cast<float>(static_cast<double>(W) / static_cast<double>(f)), 1.0f);
        }
        w.mag[sg.base + i] = g;
        if (g > 1e-3f) {
            first = first < i ? first : static_cast<int>(i);
            last = static_cast<int>(i);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        first = min(first, __shfl_xor(first, o, kWave));
        last = max(last, __shfl_xor(last, o, kWave));
    }
    if (threadIdx.x % kWave == 0 && last >= 0) {
        atomicMin(&w.sel[s].first, first);
        atomicMax(&w.sel[s].last, last);
    }
}

// output bounds.  ref: squelch.py _apply_trim (and the untrimmed copy)
__global__ void k_sq_bounds(const iqa_squelch_seg *segs, int nseg, int trim, Work w, iqa_squelch_result *res)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const iqa_squelch_seg &sg = segs[s];
    long long start = 0, stop = sg.n;
    if (trim) {
        const SelState &st = w.sel[s];
        if (st.last < 0) {
            stop = 0;
        } else {
            start = st.first - static_cast<long long>(sg.lead);
            start = start < 0 ? 0 : start;
            stop = st.last + static_cast<long long>(sg.trail) + 1;
            stop = stop > sg.n ? sg.n : stop;
        }
    }
    res[s].start = start;
    res[s].stop = stop;
}

// out[(i - start) * C + c] = x[i * C + c] * gain[i] for i in [start, stop), float32 or PCM16 (rint(double(y)*32767), saturated)
template <bool PCM16>
__global__ __launch_bounds__(SQ_THREADS) void k_sq_output(const iqa_squelch_seg *segs, int nseg, const float *in, void *out,
                                                           Work w, const iqa_squelch_result *res)
{
    const long long t = blockIdx.x;
    const int s = seg_of_tile(segs, nseg, t);
    const iqa_squelch_seg &sg = segs[s];
    const long long start = res[s].start, stop = res[s].stop;
    const int C = sg.channels;
    for (int j = 0; j < SQ_ITEMS; ++j) {
        const long long i = t * SQ_TILE - sg.base + j * SQ_THREADS + threadIdx.x;  // coalesced
        if (i < start || i >= stop) continue;
        const float g = w.mag[sg.base + i];
        const float *x = in + sg.in_off + i * C;
        const long long o = sg.in_off + (i - start) * C;
        for (int c = 0; c < C; ++c) {
            const float y = x[c] * g;
            if constexpr (PCM16) {
                const double r = rint(static_cast<double>(y) * 32767.0);  // iqio.encode_iq_slice's WAV rule
                static_cast<short *>(out)[o + c] = static_cast<short>(fmin(fmax(r, -32768.0), 32767.0));
            } else {
                static_cast<float *>(out)[o + c] = y;
            }
        }
    }
}

long long padded_samples(const iqa_squelch_seg *segs, int nseg)
{
    const iqa_squelch_seg &l = segs[nseg - 1];
    return l.base + (l.n + SQ_TILE - 1) / SQ_TILE * SQ_TILE;
}

}  // namespace
}  // namespace iqa

using namespace iqa;

extern "C" int64_t iqa_squelch_workspace_bytes(int64_t padded, int32_t n_segs)
{
    if (padded <= 0 || padded % SQ_TILE || n_segs <= 0) return -1;
    long long off[13], total;
    layout(padded, n_segs, off, &total);
    return total;
}

extern "C" int64_t iqa_squelch_stage_offset(int64_t padded, int32_t n_segs, int32_t stage)
{
    if (padded <= 0 || padded % SQ_TILE || n_segs <= 0) return -1;
    long long off[13], total;
    layout(padded, n_segs, off, &total);
    switch (stage) {
        case IQA_SQ_STAGE_ENVELOPE_DB: return off[2];
        case IQA_SQ_STAGE_LEVEL: return off[3];
        case IQA_SQ_STAGE_THRESHOLD: return off[4];
        case IQA_SQ_STAGE_MASK: return off[5];
        case IQA_SQ_STAGE_DILATED: return off[6];
        case IQA_SQ_STAGE_GAIN: return off[0];
        default: return -1;
    }
}

extern "C" int iqa_squelch(const iqa_squelch_params *p, const iqa_squelch_seg *segs, int32_t n_segs, const void *segs_dev,
                           const void *in_dev, void *out_dev, void *result_dev, void *ws_dev, int64_t ws_bytes, void *stream)
{
    if (!p || !segs || n_segs <= 0) return fail_inval("params / segments");
    if (p->method < IQA_SQ_ADAPTIVE || p->method > IQA_SQ_TRANSIENT) return fail_inval("method");
    if (!segs_dev || !in_dev || !out_dev || !result_dev || !ws_dev) return fail_inval("null device pointer");
    long long next_base = 0;
    for (int s = 0; s < n_segs; ++s) {
        const iqa_squelch_seg &g = segs[s];
        if (g.channels < 1) return fail_inval("channels < 1");
        if (g.window < 1 || g.short_window < 1 || g.long_window < 1) return fail_inval("window < 1");
        const long long need = p->method == IQA_SQ_TRANSIENT ? (g.window > g.long_window ? g.window : g.long_window) : g.window;
        if (g.n < need || g.n < 1 || g.n >= INT_MAX) {
            set_error("invalid argument: segment %d has %lld frames, fewer than its %lld-sample window (or too many)", s,
                      static_cast<long long>(g.n), need);
            return IQA_EINVAL;
        }
        if (g.base % SQ_TILE || g.base < next_base) return fail_inval("segment base not tile-aligned and ascending");
        if (g.in_off < 0 || g.fade < 0 || g.lead < 0 || g.trail < 0) return fail_inval("negative offset / fade / lead / trail");
        for (int q = 0; q < SQ_QUERIES; ++q)
            if (g.q_index[q] < 0 || g.q_index[q] >= g.n) return fail_inval("percentile index outside [0, n)");
        next_base = g.base + (g.n + SQ_TILE - 1) / SQ_TILE * SQ_TILE;
    }
    const long long np = padded_samples(segs, n_segs), nt = np / SQ_TILE;
    if (ws_bytes < iqa_squelch_workspace_bytes(np, n_segs)) return fail_inval("workspace too small");

    hipStream_t st = as_stream(stream);
    const auto *sd = static_cast<const iqa_squelch_seg *>(segs_dev);
    const float *in = static_cast<const float *>(in_dev);
    auto *res = static_cast<iqa_squelch_result *>(result_dev);
    const Work w = carve(ws_dev, np, n_segs);
    const dim3 tiles(static_cast<unsigned>(nt)), blk(SQ_THREADS);
    const unsigned seg_blocks = (n_segs + 63) / 64;
    const float tmargin = static_cast<float>(p->transient_margin_db);

    k_sq_init<<<n_segs, blk, 0, st>>>(sd, w);
    k_sq_magnitude<<<tiles, blk, 0, st>>>(sd, n_segs, in, w);
    k_sq_tile_scan<double, SumOp><<<dim3(n_segs, 1), blk, 0, st>>>(sd, reinterpret_cast<double *>(w.ta),
                                                                   reinterpret_cast<double *>(w.tb), nullptr, nullptr, 0.0);
    k_sq_prefix<<<tiles, blk, 0, st>>>(w);
    k_sq_envelope<<<tiles, blk, 0, st>>>(sd, n_segs, p->method, tmargin, w);
    if (p->auto_floor) {
        for (int shift : {21, 10, 0}) {
            k_sq_select_hist<<<tiles, blk, 0, st>>>(sd, n_segs, w.env, w, 0, 2, shift);
            k_sq_select_pick<<<dim3(n_segs, 2), blk, 0, st>>>(w, 0, shift);
        }
    }
    k_sq_floor<<<seg_blocks, 64, 0, st>>>(sd, n_segs, p->auto_floor, p->margin_db, w, res);
    if (p->method == IQA_SQ_ADAPTIVE) {
        k_sq_tile_scan<float, MinOp><<<dim3(n_segs, 1), blk, 0, st>>>(sd, reinterpret_cast<float *>(w.tc),
                                                                      reinterpret_cast<float *>(w.td), nullptr, nullptr, INFINITY);
        k_sq_relative<<<tiles, blk, 0, st>>>(sd, n_segs, w);
        for (int shift : {21, 10, 0}) {
            k_sq_select_hist<<<tiles, blk, 0, st>>>(sd, n_segs, w.rel, w, 2, 4, shift);
            k_sq_select_pick<<<dim3(n_segs, 4), blk, 0, st>>>(w, 2, shift);
        }
        k_sq_span<<<seg_blocks, 64, 0, st>>>(sd, n_segs, w);
        k_sq_mask_adaptive<<<tiles, blk, 0, st>>>(sd, n_segs, w);
    } else if (p->method == IQA_SQ_STATIC) {
        k_sq_mask_static<<<tiles, blk, 0, st>>>(sd, n_segs, w);
    } else {
        k_sq_mask_count<<<tiles, blk, 0, st>>>(sd, n_segs, w);
    }
    k_sq_tile_scan<long long, SumOp><<<dim3(n_segs, 1), blk, 0, st>>>(sd, w.ta, w.tb, nullptr, nullptr, 0LL);
    k_sq_count_prefix<<<tiles, blk, 0, st>>>(sd, n_segs, w.mask, w.tb, w.cm, nullptr, nullptr);
    k_sq_dilate<<<tiles, blk, 0, st>>>(sd, n_segs, w);
    k_sq_tile_scan<long long, SumOp><<<dim3(n_segs, 2), blk, 0, st>>>(sd, w.ta, w.tb, w.tc, w.td, 0LL);
    k_sq_count_prefix<<<tiles, blk, 0, st>>>(sd, n_segs, w.dil, w.tb, w.cd, w.td, reinterpret_cast<long long *>(w.pre));
    k_sq_gain<<<tiles, blk, 0, st>>>(sd, n_segs, w);
    k_sq_bounds<<<seg_blocks, 64, 0, st>>>(sd, n_segs, p->trim, w, res);
    if (p->out_pcm16)
        k_sq_output<true><<<tiles, blk, 0, st>>>(sd, n_segs, in, out_dev, w, res);
    else
        k_sq_output<false><<<tiles, blk, 0, st>>>(sd, n_segs, in, out_dev, w, res);
    return check_launch("k_sq_* (squelch chain)");
}
