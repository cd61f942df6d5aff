// demod_fused.hip -- the demodulator's scan engine: whole demodulator + AudioWriter.write for a block of
// channel samples in three launches (reduce -> carry -> apply), the pluggable stage API on the same passes,
// and the source stages (discriminator, envelope, real part).
//
// Replaces, for one block of decimated samples z (reference src/iq_to_audio/):
//   decoder.process(z)            processing.py:1128
//     nfm: QuadratureDemod + DeemphasisFilter      decoders/nfm.py:17-24, 48-62
//     am : abs + DCBlocker                         decoders/am.py:28, decoders/common.py:16-30
//     ssb: real + DCBlocker [+ _apply_agc]         decoders/ssb.py:42-45, 65-80
//   audio_writer.write(audio)     processing.py:1147 -> :440-456 (pre-clip peak, clip +-0.99)
//   stats rms_dbfs per chunk      decoders/nfm.py:88-89 (sum of squares per reference chunk)
//
// The three IIR stages are per-sample Python/C loops in the reference.  Each is a first-order affine
// recurrence s[n] = a[n]*s[n-1] + b[n]; affine maps compose associatively, so they run here as a block
// scan in float64.  The AGC's "gain restarts at 1.0 on every process() call" becomes a segmented scan:
// at a restart index the element's map is the constant a+b.
//
// The source stage (discriminator / envelope / real part) is evaluated on the fly inside the
// scan passes, and the sink (peak, clip, per-chunk sum of squares) inside the apply pass, so z is
// read twice and the audio written once: 20 B per channel sample instead of ~52.
// SSB with AGC needs two dependent recurrences and therefore two scans (DC blocker to a float
// scratch, then the segmented AGC scan with the sink).
//
// The stage API (iqa_deemphasis, iqa_dc_block, iqa_agc) runs one recurrence from a float input to the
// unclipped output on the same passes, and the stand-alone source stages (iqa_quadrature, iqa_envelope,
// iqa_real_part) evaluate the same source formulas: a block through the stages gives the audio of the
// fused path before its clip.
#include "common.h"

namespace iqa {

constexpr int SC_THREADS = 256;
constexpr int SC_ITEMS = 8;
constexpr int SC_TILE = SC_THREADS * SC_ITEMS;  // 2048 elements per block

struct Aff {  // s -> A*s + B
    double A, B;
};
// apply `l` first, then `r`
__device__ __forceinline__ Aff then(const Aff &l, const Aff &r) { return Aff{r.A * l.A, fma(r.A, l.B, r.B)}; }

// inclusive ordered wave scan; returns the inclusive prefix for this lane
__device__ __forceinline__ Aff wave_inclusive(Aff v, int lane)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double la = __shfl_up(v.A, o, kWave);
        const double lb = __shfl_up(v.B, o, kWave);
        if (lane >= o) v = then(Aff{la, lb}, v);
    }
    return v;
}

// first index in sorted `arr[0..n)` that is >= v
__device__ __forceinline__ long long lower_bound_ll(const long long *arr, long long n, long long v)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (arr[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

enum FOp { F_DEEMPH = 0, F_DC = 1, F_AGC = 2 };
enum FSrc { S_F32 = 0, S_QUAD = 1, S_ENV = 2, S_REAL = 3 };
enum FSink { K_PLAIN = 0, K_CLIP = 1 };

struct FusedArgs {
    const float2 *z;     // S_QUAD / S_ENV / S_REAL
    const float *x;      // S_F32
    float *y;
    long long n;
    double p0, p1;       // DEEMPH: alpha, 1-alpha | DC: radius (f32-rounded) | AGC: target (f32), decay (f32)
    const float2 *prev;  // S_QUAD: previous complex sample
    const double *st;    // DEEMPH: {y_last} | DC: {x_last, y_last}
    const long long *segs;  // chunk starts (AGC restarts and statistics segments), segs[0] == 0
    long long n_segs;
    unsigned int *peak_bits;
    double *sumsq;
    Aff *agg;
    double *carry;
    double *fin;
    int nblocks;
    int z_aligned, y_aligned;  // z / y are 16-byte aligned: the vector load / store paths may be used
    int fresh;  // the decoder has seen nothing: prev = 1 + 0j, filter states 0 (the caller's state block is not read), and the
                // carry pass clears the peak and the per-chunk sums -- iqa_demodulate_from_reset, no reset copy in front
};

// the source stage's value at a sample zc with predecessor zp (only the discriminator reads zp)
template <int SRC>
__device__ __forceinline__ float src_value(float2 zc, float2 zp)
{
    if constexpr (SRC == S_QUAD) {
        const float re = zc.x * zp.x + zc.y * zp.y;  // z * conj(z_prev), float32 as numpy forms it
        const float im = zc.y * zp.x - zc.x * zp.y;
        return atan2f(im, re);
    } else if constexpr (SRC == S_ENV) {
        return np_abs_c64(zc.x, zc.y);  // numpy's float32 value, bit for bit (common.h)
    } else {
        return zc.x;
    }
}

// ---- the source stages on their own (iqa_quadrature, iqa_envelope, iqa_real_part) -------------

__global__ void k_quadrature(const float2 *z, long long n, const float2 *prev, float *out)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = src_value<S_QUAD>(z[i], (i == 0) ? prev[0] : z[i - 1]);
}

// a launch of its own behind k_quadrature, whose element 0 still reads the old prev
__global__ void k_store_last(const float2 *z, long long n, float2 *prev)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) prev[0] = z[n - 1];
}

__global__ void k_envelope(const float2 *z, long long n, float *out)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src_value<S_ENV>(z[i], z[i]);
}

__global__ void k_real(const float2 *z, long long n, float *out)
{
    const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src_value<S_REAL>(z[i], z[i]);
}

// ---- the scan engine ---------------------------------------------------------------------------

// u[base-1 .. base+7] -> x[0..7] plus x_before (only DC needs u[base-1])
template <int OP, int SRC>
__device__ __forceinline__ void load_u(const FusedArgs &a, long long base, float (&u)[SC_ITEMS], float &u_before)
{
    u_before = 0.f;
    if constexpr (SRC == S_F32) {
#pragma unroll
        for (int i = 0; i < SC_ITEMS; ++i) u[i] = (base + i < a.n) ? a.x[base + i] : 0.f;
        if constexpr (OP == F_DC) {
            if (base == 0) u_before = a.fresh ? 0.f : static_cast<float>(a.st[0]);
            else if (base - 1 < a.n) u_before = a.x[base - 1];
        }
    } else {
        float2 zz[SC_ITEMS + 2];  // z[base-2 .. base+7]
        static_assert(SC_ITEMS == 8, "the vector path below moves 8 float2 = 4 x 16 bytes per thread");
        // Whole-wave fast path (every tile but the last): a thread's eight samples are 64 contiguous, 16-byte
        // aligned bytes -> four 16-byte loads; the two samples in front of them are the previous lane's last two
        // (one shuffle each) except for lane 0.  Scalar float2 loads at a 64-byte lane stride cost 2.5x the
        // load instructions and touch every line five times.
        const int lane = threadIdx.x & 63;
        const long long wave_base = base - static_cast<long long>(lane) * SC_ITEMS;
        if (a.z_aligned && wave_base + 64 * SC_ITEMS <= a.n) {
            const float4 *p = reinterpret_cast<const float4 *>(a.z + base);
            const float4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
            zz[2] = make_float2(q0.x, q0.y);
            zz[3] = make_float2(q0.z, q0.w);
            zz[4] = make_float2(q1.x, q1.y);
            zz[5] = make_float2(q1.z, q1.w);
            zz[6] = make_float2(q2.x, q2.y);
            zz[7] = make_float2(q2.z, q2.w);
            zz[8] = make_float2(q3.x, q3.y);
            zz[9] = make_float2(q3.z, q3.w);
            float2 e0 = make_float2(0.f, 0.f), e1 = make_float2(0.f, 0.f);
            if (lane == 0 && base >= 2) {
                e0 = a.z[base - 2];
                e1 = a.z[base - 1];
            }
            zz[0] = make_float2(__shfl_up(q3.x, 1, kWave), __shfl_up(q3.y, 1, kWave));
            zz[1] = make_float2(__shfl_up(q3.z, 1, kWave), __shfl_up(q3.w, 1, kWave));
            if (lane == 0) {
                zz[0] = e0;
                zz[1] = e1;
            }
        } else {
#pragma unroll
            for (int i = 0; i < SC_ITEMS + 2; ++i) {
                const long long k = base - 2 + i;
                zz[i] = (k >= 0 && k < a.n) ? a.z[k] : make_float2(0.f, 0.f);
            }
        }
        if constexpr (SRC == S_QUAD) {
            if (base == 0) zz[1] = a.fresh ? make_float2(1.f, 0.f) : a.prev[0];  // z[-1]
        }
#pragma unroll
        for (int i = 0; i < SC_ITEMS; ++i) u[i] = (base + i < a.n) ? src_value<SRC>(zz[i + 2], zz[i + 1]) : 0.f;
        if constexpr (OP == F_DC) {
            // DC blocker's x[n-1]: u[base-1] from z (ENV/REAL never need z[base-2]); carried state at 0
            if (base == 0) u_before = a.fresh ? 0.f : static_cast<float>(a.st[0]);
            else u_before = src_value<SRC>(zz[1], zz[0]);
        }
    }
}

template <int OP>
__device__ __forceinline__ Aff fmap(const FusedArgs &a, long long idx, float x, float x_prev, bool maybe_reset)
{
    if constexpr (OP == F_DEEMPH) {
        return Aff{a.p0, a.p1 * static_cast<double>(x)};
    } else if constexpr (OP == F_DC) {
        return Aff{a.p0, static_cast<double>(x - x_prev)};
    } else {
        const float mag = fabsf(x);
        Aff m{1.0, 0.0};
        if (mag > 1e-6f) {
            const float desired = static_cast<float>(a.p0) / mag;
            m = Aff{1.0 - a.p1, a.p1 * static_cast<double>(desired)};
        }
        if (maybe_reset) {
            bool rst = (idx == 0);
            if (!rst && a.segs != nullptr && a.n_segs > 0) {
                const long long lo = lower_bound_ll(a.segs, a.n_segs, idx);
                rst = lo < a.n_segs && a.segs[lo] == idx;
            }
            if (rst) m = Aff{0.0, m.A + m.B};
        }
        return m;
    }
}

__device__ __forceinline__ bool block_has_restart(const FusedArgs &a, long long lo_i, long long hi_i)
{
    if (lo_i == 0) return true;
    if (a.segs == nullptr || a.n_segs <= 0) return false;
    const long long lo = lower_bound_ll(a.segs, a.n_segs, lo_i);
    return lo < a.n_segs && a.segs[lo] < hi_i;
}

// ---- the sink of the one-launch form ----------------------------------------------------------------------------
// (k_fused_apply below carries the same steps inline: moving it onto these helpers took its NFM instance from 80 to 111
// registers and the AGC's from 90 to 120 -- six and five resident waves per SIMD to four -- so it is left as it was)

// The segment (reference chunk) of the first and of the last of a block's samples, counted by the whole block in ONE
// round of loads (a two-thread binary search in front of the first barrier cost eight dependent global loads per block).
// `seg_first`: this thread's share of the chunk starts, a.segs[tid], loaded by the caller in front of its tile's loads;
// s_seg[0..1] hold -1 (behind a barrier).  The counts are complete behind the block's next barrier.
template <int THREADS>
__device__ __forceinline__ void sink_count_segments(const FusedArgs &a, long long seg_first, long long first, long long last,
                                                    long long *s_seg)
{
    const int tid = threadIdx.x, lane = tid & 63;
    int c0 = (tid < a.n_segs) && seg_first <= first, c1 = (tid < a.n_segs) && seg_first <= last;
    for (long long kk = tid + THREADS; kk < a.n_segs; kk += THREADS) {
        const long long st = a.segs[kk];
        c0 += st <= first;
        c1 += st <= last;
    }
    c0 = static_cast<int>(wave_sum(static_cast<float>(c0)));
    c1 = static_cast<int>(wave_sum(static_cast<float>(c1)));
    if (lane == 0 && (c0 | c1)) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&s_seg[0]), static_cast<unsigned long long>(c0));
        atomicAdd(reinterpret_cast<unsigned long long *>(&s_seg[1]), static_cast<unsigned long long>(c1));
    }
}

// A block's samples lie inside one reference chunk (`uniform`) or, a chunk being >= 40 k samples, straddle exactly one
// boundary (`simple`): the squares go to a low and a high running sum split at that boundary, reduced over the block, two
// atomics per block at most.  Only blocks with several boundaries (chunks shorter than a block's range) take the general
// per-thread path with its own look-ups.
struct SinkPlan {
    bool stats, uniform, simple, general;
    long long seg0, seg1, bnd;  // bnd: first index of the high part
    int sub;                    // this block's sub-slot of a chunk's sums
};
__device__ __forceinline__ SinkPlan sink_plan(const FusedArgs &a, bool stats, const long long *s_seg)
{
    SinkPlan p;
    p.stats = stats;
    p.seg0 = stats ? s_seg[0] : -1;
    p.seg1 = stats ? s_seg[1] : -1;
    p.uniform = stats && (p.seg0 == p.seg1);
    p.simple = stats && (p.seg1 == p.seg0 + 1);
    p.general = stats && !p.uniform && !p.simple;
    p.bnd = a.n;
    if (p.simple) p.bnd = a.segs[p.seg1];
    p.sub = blockIdx.x & (IQA_SUMSQ_SLOTS - 1);
    return p;
}

struct SinkAcc {
    float pk = 0.f;
    double run = 0.0, run_hi = 0.0;
    long long seg = 0;  // general path: the segment `run` belongs to
};

// one pre-clip value v at index idx: peak, sums; returns the value to store
template <int SINK>
__device__ __forceinline__ float sink_item(const FusedArgs &a, const SinkPlan &p, SinkAcc &k, float v, long long idx)
{
    if constexpr (SINK != K_CLIP) return v;
    k.pk = fmaxf(k.pk, fabsf(v));
    if (p.stats) {
        const double vv = static_cast<double>(v) * static_cast<double>(v);
        double run = k.run, run_hi = k.run_hi;  // (values, not members: the two sums must stay in registers)
        long long seg = k.seg;
        if (p.general) {
            while (seg + 1 < a.n_segs && a.segs[seg + 1] <= idx) {
                if (run != 0.0) atomicAdd(&a.sumsq[seg * IQA_SUMSQ_SLOTS + p.sub], run);
                run = 0.0;
                ++seg;
            }
            run += vv;
        } else {
            const bool low = idx < p.bnd;
            run += low ? vv : 0.0;
            run_hi += low ? 0.0 : vv;
        }
        k.run = run;
        k.run_hi = run_hi;
        k.seg = seg;
    }
    return fminf(fmaxf(v, -0.99f), 0.99f);
}

// general path: what a thread holds goes out (at the end of its run of consecutive samples)
__device__ __forceinline__ void sink_flush_general(const FusedArgs &a, const SinkPlan &p, SinkAcc &k)
{
    if (p.general && k.run != 0.0) atomicAdd(&a.sumsq[k.seg * IQA_SUMSQ_SLOTS + p.sub], k.run);
    if (p.general) k.run = 0.0;
}

// the block's peak and sums: wave reductions, one barrier, at most three atomics by thread 0
template <int WAVES>
__device__ __forceinline__ void sink_finish(const FusedArgs &a, const SinkPlan &p, SinkAcc &k, float *s_pk, double *s_sq)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    sink_flush_general(a, p, k);
    const float pk = wave_max(k.pk);
    const double wlo = (p.stats && !p.general) ? wave_sum(k.run) : 0.0;
    const double whi = p.simple ? wave_sum(k.run_hi) : 0.0;
    if (lane == 0) {
        s_pk[wave] = pk;
        s_sq[wave] = wlo;
        s_sq[WAVES + wave] = whi;
    }
    __syncthreads();
    if (tid == 0) {
        float m = s_pk[0];
        double lo = s_sq[0], hi = s_sq[WAVES];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            m = fmaxf(m, s_pk[w]);
            lo += s_sq[w];
            hi += s_sq[WAVES + w];
        }
        if (a.peak_bits != nullptr) {
            // thousands of atomics on one word serialise in L2 (~11 ns each): skip the ones that cannot
            // raise the running maximum (a stale read only costs a redundant atomic, never a wrong result)
            const unsigned int mb = __float_as_uint(m);
            if (mb > __hip_atomic_load(a.peak_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.peak_bits, mb);
        }
        if (p.stats && !p.general) atomicAdd(&a.sumsq[p.seg0 * IQA_SUMSQ_SLOTS + p.sub], lo);
        if (p.simple) atomicAdd(&a.sumsq[p.seg1 * IQA_SUMSQ_SLOTS + p.sub], hi);
    }
}

// a thread's eight values to y[base ..], those with index in [lo, hi): 32 contiguous, aligned bytes as two 16-byte stores
__device__ __forceinline__ void store_items(const FusedArgs &a, long long base, long long lo, long long hi, const float (&vout)[SC_ITEMS])
{
    if (a.y_aligned && base >= lo && base + SC_ITEMS <= hi) {
        float4 *yp = reinterpret_cast<float4 *>(a.y + base);
        yp[0] = make_float4(vout[0], vout[1], vout[2], vout[3]);
        yp[1] = make_float4(vout[4], vout[5], vout[6], vout[7]);
    } else {
#pragma unroll
        for (int i = 0; i < SC_ITEMS; ++i)
            if (base + i >= lo && base + i < hi) a.y[base + i] = vout[i];
    }
}

template <int OP, int SRC>
__global__ __launch_bounds__(SC_THREADS) void k_fused_reduce(FusedArgs a)
{
    __shared__ Aff s_w[SC_THREADS / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long blk0 = static_cast<long long>(blockIdx.x) * SC_TILE;
    const long long base = blk0 + static_cast<long long>(tid) * SC_ITEMS;
    const bool mr = (OP == F_AGC) && block_has_restart(a, blk0, blk0 + SC_TILE);
    float u[SC_ITEMS], ub;
    load_u<OP, SRC>(a, base, u, ub);
    Aff t{1.0, 0.0};
#pragma unroll
    for (int i = 0; i < SC_ITEMS; ++i)
        if (base + i < a.n) t = then(t, fmap<OP>(a, base + i, u[i], i ? u[i - 1] : ub, mr));
    const Aff inc = wave_inclusive(t, lane);
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    if (tid == 0) {
        Aff tot = s_w[0];
#pragma unroll
        for (int w = 1; w < SC_THREADS / kWave; ++w) tot = then(tot, s_w[w]);
        a.agg[blockIdx.x] = tot;
    }
}

// Carry pass: exclusive scan of the per-tile maps.  One block of 1024 threads: a thread composes its run of
// consecutive tiles, a wave scan and a 16-entry table in LDS give it the state in front of its run, and it walks
// the run once more to store the carries (a single wave walking thousands of tiles serially cost 30 us).
constexpr int FC_THREADS = 1024;
template <int OP>
__global__ __launch_bounds__(FC_THREADS) void k_fused_carry(FusedArgs a)
{
    __shared__ Aff s_w[FC_THREADS / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s0;
    if constexpr (OP == F_DEEMPH) s0 = a.fresh ? 0.0 : a.st[0];
    else if constexpr (OP == F_DC) s0 = a.fresh ? 0.0 : a.st[1];
    else s0 = 1.0;
    const int per = (a.nblocks + FC_THREADS - 1) / FC_THREADS;
    const int b0 = tid * per;
    Aff t{1.0, 0.0};
    for (int i = 0; i < per; ++i)
        if (b0 + i < a.nblocks) t = then(t, a.agg[b0 + i]);
    const Aff inc = wave_inclusive(t, lane);
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    Aff pre{1.0, 0.0};
    for (int w = 0; w < wave; ++w) pre = then(pre, s_w[w]);
    Aff exl{__shfl_up(inc.A, 1, kWave), __shfl_up(inc.B, 1, kWave)};
    if (lane == 0) exl = Aff{1.0, 0.0};
    const Aff ex = then(pre, exl);
    double s = fma(ex.A, s0, ex.B);  // state in front of this thread's run
    for (int i = 0; i < per; ++i) {
        const int b = b0 + i;
        if (b < a.nblocks) {
            a.carry[b] = s;
            const Aff v = a.agg[b];
            s = fma(v.A, s, v.B);
        }
    }
    if (tid == FC_THREADS - 1) a.fin[0] = s;  // runs past the end are identity maps: the last thread holds the total
    // Snapshot of the incoming state for the apply pass (fin[1] = prev, fin[2] = st[0]): its last block hands the
    // outgoing state to the next call while its first block may not have read the incoming one yet.
    if (a.fresh) {  // (the apply pass -- the only writer of these -- runs behind this kernel)
        if (tid == 0 && a.peak_bits != nullptr) a.peak_bits[0] = 0u;
        if (a.sumsq != nullptr)
            for (long long i = tid; i < a.n_segs * IQA_SUMSQ_SLOTS; i += FC_THREADS) a.sumsq[i] = 0.0;
    }
    if (tid == 0) {
        if (a.prev != nullptr) reinterpret_cast<float2 *>(a.fin + 1)[0] = a.fresh ? make_float2(1.f, 0.f) : a.prev[0];
        if (a.st != nullptr) a.fin[2] = a.fresh ? 0.0 : a.st[0];
    }
}

// `a.prev` / `a.st` point at the carry pass's snapshot; prev_out / st_out at the caller's state block (written by
// the last block: the streaming state for the next call, OP != F_AGC)
template <int OP, int SRC, int SINK>
__global__ __launch_bounds__(SC_THREADS) void k_fused_apply(FusedArgs a, float2 *prev_out, double *st_out)
{
    __shared__ Aff s_w[SC_THREADS / kWave];
    __shared__ float s_pk[SC_THREADS / kWave];
    __shared__ double s_sq[2 * (SC_THREADS / kWave)];  // low | high part of a tile that straddles a chunk boundary
    __shared__ long long s_seg[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long blk0 = static_cast<long long>(blockIdx.x) * SC_TILE;
    const long long base = blk0 + static_cast<long long>(tid) * SC_ITEMS;
    const bool mr = (OP == F_AGC) && block_has_restart(a, blk0, blk0 + SC_TILE);
    const bool stats = (SINK == K_CLIP) && a.sumsq != nullptr && a.n_segs > 0;
    // Issued first, consumed late: the state in front of this tile, and the segment (reference chunk) of the tile's
    // first and last element, counted by the whole block in ONE round of loads (a two-thread binary search in front
    // of the first barrier cost eight dependent global loads per block: two thirds of this kernel's time was waiting).
    const double carry_in = a.carry[blockIdx.x];
    // this thread's share of the chunk starts (one round of loads, issued in front of the tile's own loads)
    long long seg_first = 0;
    if (stats && tid < a.n_segs) seg_first = a.segs[tid];
    if (stats && tid < 2) s_seg[tid] = -1;
    float u[SC_ITEMS], ub;
    load_u<OP, SRC>(a, base, u, ub);
    // The maps of the AGC (a division and a restart look-up each) are kept for the second walk; those of the two
    // linear filters are one multiply / one subtract and are formed again there: 16 doubles fewer to hold, which is what
    // decides between five and eight resident waves per SIMD for a kernel that lives two or three rounds of blocks.
    constexpr bool KEEP = (OP == F_AGC);
    Aff m[KEEP ? SC_ITEMS : 1];
    Aff t{1.0, 0.0};
#pragma unroll
    for (int i = 0; i < SC_ITEMS; ++i) {
        const Aff mi = (base + i < a.n) ? fmap<OP>(a, base + i, u[i], i ? u[i - 1] : ub, mr) : Aff{1.0, 0.0};
        if constexpr (KEEP) m[i] = mi;
        t = then(t, mi);
    }
    if (stats) {
        __syncthreads();  // s_seg initialised
        const long long first = blk0, last = min(blk0 + SC_TILE, a.n) - 1;
        int c0 = (tid < a.n_segs) && seg_first <= first, c1 = (tid < a.n_segs) && seg_first <= last;
        for (long long kk = tid + SC_THREADS; kk < a.n_segs; kk += SC_THREADS) {
            const long long st = a.segs[kk];
            c0 += st <= first;
            c1 += st <= last;
        }
        c0 = static_cast<int>(wave_sum(static_cast<float>(c0)));
        c1 = static_cast<int>(wave_sum(static_cast<float>(c1)));
        if (lane == 0 && (c0 | c1)) {
            atomicAdd(reinterpret_cast<unsigned long long *>(&s_seg[0]), static_cast<unsigned long long>(c0));
            atomicAdd(reinterpret_cast<unsigned long long *>(&s_seg[1]), static_cast<unsigned long long>(c1));
        }
    }
    const Aff inc = wave_inclusive(t, lane);
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    const double ea = __shfl_up(inc.A, 1, kWave), eb = __shfl_up(inc.B, 1, kWave);
    Aff ex = (lane == 0) ? Aff{1.0, 0.0} : Aff{ea, eb};
    Aff wpre{1.0, 0.0};
    for (int w = 0; w < wave; ++w) wpre = then(wpre, s_w[w]);
    ex = then(wpre, ex);
    double s = fma(ex.A, carry_in, ex.B);

    // A tile (2048 samples) lies inside one reference chunk (`uniform`) or, a chunk being >= 40 k samples, straddles
    // exactly one boundary (`simple`): the squares go to a low and a high running sum split at that boundary, reduced
    // over the block, two atomics per block at most.  Only tiles with several boundaries (chunks shorter than a tile)
    // take the general per-thread path with its own look-ups.
    const long long seg0 = stats ? s_seg[0] : -1, seg1 = stats ? s_seg[1] : -1;
    const bool uniform = stats && (seg0 == seg1);
    const bool simple = stats && (seg1 == seg0 + 1);
    const bool general = stats && !uniform && !simple;
    long long bnd = a.n;  // first index of the high part
    if (simple) bnd = a.segs[seg1];
    long long seg = seg0;
    if (general && base < a.n) seg = lower_bound_ll(a.segs, a.n_segs, base + 1) - 1;
    float pk = 0.f;
    double run = 0.0, run_hi = 0.0;
    float vout[SC_ITEMS];
#pragma unroll
    for (int i = 0; i < SC_ITEMS; ++i) {
        const long long idx = base + i;
        Aff mi;
        if constexpr (KEEP) mi = m[i];
        else mi = (idx < a.n) ? fmap<OP>(a, idx, u[i], i ? u[i - 1] : ub, mr) : Aff{1.0, 0.0};
        s = fma(mi.A, s, mi.B);
        vout[i] = 0.f;
        if (idx < a.n) {
            const float v = (OP == F_AGC) ? u[i] * static_cast<float>(s) : static_cast<float>(s);
            if constexpr (SINK == K_CLIP) {
                pk = fmaxf(pk, fabsf(v));
                vout[i] = fminf(fmaxf(v, -0.99f), 0.99f);
                if (stats) {
                    const double vv = static_cast<double>(v) * static_cast<double>(v);
                    if (general) {
                        while (seg + 1 < a.n_segs && a.segs[seg + 1] <= idx) {
                            if (run != 0.0) atomicAdd(&a.sumsq[seg * IQA_SUMSQ_SLOTS + (blockIdx.x & (IQA_SUMSQ_SLOTS - 1))], run);
                            run = 0.0;
                            ++seg;
                        }
                        run += vv;
                    } else {
                        run += idx < bnd ? vv : 0.0;
                        run_hi += idx < bnd ? 0.0 : vv;
                    }
                }
            } else {
                vout[i] = v;
            }
        }
    }
    if constexpr (SINK == K_CLIP) {
        if (general && run != 0.0) atomicAdd(&a.sumsq[seg * IQA_SUMSQ_SLOTS + (blockIdx.x & (IQA_SUMSQ_SLOTS - 1))], run);
        pk = wave_max(pk);
        const double wlo = (stats && !general) ? wave_sum(run) : 0.0;
        const double whi = simple ? wave_sum(run_hi) : 0.0;
        if (lane == 0) {
            s_pk[wave] = pk;
            s_sq[wave] = wlo;
            s_sq[4 + wave] = whi;
        }
        __syncthreads();
        if (tid == 0) {
            if (a.peak_bits != nullptr) {
                // thousands of atomics on one word serialise in L2 (~11 ns each): skip the ones that cannot
                // raise the running maximum (a stale read only costs a redundant atomic, never a wrong result)
                const unsigned int m = __float_as_uint(fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3])));
                if (m > __hip_atomic_load(a.peak_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.peak_bits, m);
            }
            const int sub = blockIdx.x & (IQA_SUMSQ_SLOTS - 1);
            if (stats && !general) atomicAdd(&a.sumsq[seg0 * IQA_SUMSQ_SLOTS + sub], s_sq[0] + s_sq[1] + s_sq[2] + s_sq[3]);
            if (simple) atomicAdd(&a.sumsq[seg1 * IQA_SUMSQ_SLOTS + sub], s_sq[4] + s_sq[5] + s_sq[6] + s_sq[7]);
        }
    }
    if (OP != F_AGC && blockIdx.x == a.nblocks - 1 && tid == 0) {  // hand the streaming state to the next call
        if constexpr (SRC == S_QUAD) prev_out[0] = a.z[a.n - 1];
        if constexpr (OP == F_DEEMPH) {
            st_out[0] = a.fin[0];
        } else if constexpr (OP == F_DC) {
            float last;
            if constexpr (SRC == S_F32) last = a.x[a.n - 1];
            else last = src_value<SRC>(a.z[a.n - 1], make_float2(0.f, 0.f));
            st_out[0] = static_cast<double>(last);
            st_out[1] = a.fin[0];
        }
    }
    // the audio goes out last: nothing waits for these stores (a barrier behind them would)
    if (a.y_aligned && base + SC_ITEMS <= a.n) {  // 32 contiguous, aligned bytes per thread: two 16-byte stores
        float4 *yp = reinterpret_cast<float4 *>(a.y + base);
        yp[0] = make_float4(vout[0], vout[1], vout[2], vout[3]);
        yp[1] = make_float4(vout[4], vout[5], vout[6], vout[7]);
    } else {
#pragma unroll
        for (int i = 0; i < SC_ITEMS; ++i)
            if (base + i < a.n) a.y[base + i] = vout[i];
    }
}

// ---- the one-launch form of the de-emphasis scan ----------------------------------------------------------
//
// The de-emphasis pole forgets: alpha^W <= 2^-64 after W samples (W from scan_window below, a multiple of 512).  A
// workgroup therefore needs no state from its predecessors: it covers FW_SPAN consecutive positions, the first W of
// them a warm-up from state 0 (computed, not stored, not in the peak or the sums), the other FW_SPAN - W its own.
// The state it ignores is a y of this call, |y| <= S, so its first own sample is off by at most 2^-64 S: 2^-17 of the
// floor term 64 * 2^-53 * S / (1 - alpha) that the scan's own roundings are allowed.  Block 0 starts at index 0 from
// the carried state (the exact chain), and is the only block that reads the caller's state block; it also writes the
// outgoing state, from a warm-up of its own over the last W samples where the call has more than one block.  So no
// block waits for another: no flags, no counters, nothing kept in the workspace.
// A block runs its span in FW_ROUNDS rounds of FW_THREADS * SC_ITEMS positions, handing the state from round to round.
// 256 x 8 x 4 by measurement at config 2 (n = 5 769 231, W = 1536): 41 us against 44 for 512 x 8 x 2, 43 for
// 512 x 8 x 4, 52 for 256 x 8 x 8, 60 for 1024 x 8 x 1 and 84 for 1024 x 8 x 2 -- 867 workgroups of four waves at 91 registers
// are all resident at once (five waves per SIMD), and a longer span only adds serial rounds.
constexpr int FW_THREADS = 256;
constexpr int FW_ROUNDS = 4;
constexpr int FW_WAVES = FW_THREADS / kWave;
constexpr long long FW_ROUND = static_cast<long long>(FW_THREADS) * SC_ITEMS;
constexpr long long FW_SPAN = FW_ROUND * FW_ROUNDS;

// 0 and the window W where the one-launch form is used for this pole, 1 where the three launches are kept (no pole in
// (0, 1), or a W above half a span: a long time constant, a high channel rate).  Depends on alpha alone.
static int scan_window(double alpha, long long *window)
{
    if (!(alpha > 0.0 && alpha < 1.0)) return 1;
    const double need = 64.0 * log(2.0) / -log(alpha);  // alpha^need = 2^-64
    if (!(need < static_cast<double>(FW_SPAN))) return 1;
    long long w = 512 * static_cast<long long>(ceil(need / 512.0));
    if (w < 512) w = 512;
    while (w > 512 && pow(alpha, static_cast<double>(w - 512)) <= 0x1p-64) w -= 512;  // (the logarithms' rounding)
    while (pow(alpha, static_cast<double>(w)) > 0x1p-64) w += 512;
    if (2 * w > FW_SPAN) return 1;
    *window = w;
    return 0;
}

// One round: the source values u of positions [base, base + 8) and the state in front of `base`, given the state
// `s_run` in front of the round; `s_run` becomes the state behind the round.  Positions at or above `end` are identity
// maps.  `skip0`: the value at index 0 is taken as 0 (a warm-up that begins at index 0 in a block other than block 0,
// which does not read the carried prev).  One barrier; `s_w` is this round's table (the caller alternates two).
template <int SRC>
__device__ __forceinline__ double windowed_round(const FusedArgs &a, long long base, long long end, bool skip0, Aff *s_w,
                                                 double &s_run, float (&u)[SC_ITEMS])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ub;
    load_u<F_DEEMPH, SRC>(a, base, u, ub);
    if (skip0 && base == 0) u[0] = 0.f;
    Aff t{1.0, 0.0};
#pragma unroll
    for (int i = 0; i < SC_ITEMS; ++i)
        if (base + i < end) t = then(t, fmap<F_DEEMPH>(a, base + i, u[i], 0.f, false));
    const Aff inc = wave_inclusive(t, lane);
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    const double ea = __shfl_up(inc.A, 1, kWave), eb = __shfl_up(inc.B, 1, kWave);
    Aff ex = (lane == 0) ? Aff{1.0, 0.0} : Aff{ea, eb};
    Aff acc{1.0, 0.0}, wpre{1.0, 0.0};
#pragma unroll
    for (int w = 0; w < FW_WAVES; ++w) {
        if (w == wave) wpre = acc;
        acc = then(acc, s_w[w]);
    }
    ex = then(wpre, ex);
    const double s = fma(ex.A, s_run, ex.B);
    s_run = fma(acc.A, s_run, acc.B);  // the same operations in every thread: one value for the whole block
    return s;
}

// clears the peak and the per-chunk sums in front of a windowed launch (iqa_demodulate_from_reset); with `state`, also
// writes the state block of a decoder that has seen nothing (iqa_demod_reset)
__global__ __launch_bounds__(FC_THREADS) void k_fused_clear(float *state, unsigned int *peak_bits, double *sumsq, long long n_sums)
{
    if (state != nullptr && threadIdx.x < 8) state[threadIdx.x] = threadIdx.x ? 0.f : 1.f;  // prev = 1 + 0j, filter states 0
    if (threadIdx.x == 0 && peak_bits != nullptr) peak_bits[0] = 0u;
    if (sumsq != nullptr)
        for (long long i = threadIdx.x; i < n_sums; i += FC_THREADS) sumsq[i] = 0.0;
}

template <int SRC, int SINK>
__global__ __launch_bounds__(FW_THREADS) void k_fused_windowed(FusedArgs a, long long window, float2 *prev_out, double *st_out)
{
    __shared__ Aff s_w[2][FW_WAVES];
    __shared__ float s_pk[FW_WAVES];
    __shared__ double s_sq[2 * FW_WAVES];  // low | high part of an own range that straddles a chunk boundary
    __shared__ long long s_seg[2];
    const int tid = threadIdx.x;
    const long long own = FW_SPAN - window;
    const long long own0 = static_cast<long long>(blockIdx.x) * own, own1 = min(own0 + own, a.n);
    const long long start = blockIdx.x ? own0 - window : 0;  // >= 0: window <= own
    const bool skip0 = blockIdx.x != 0;
    const bool stats = (SINK == K_CLIP) && a.sumsq != nullptr && a.n_segs > 0;
    double s_run = (blockIdx.x == 0 && !a.fresh) ? a.st[0] : 0.0;
    long long seg_first = 0;
    if (stats && tid < a.n_segs) seg_first = a.segs[tid];
    if (stats && tid < 2) s_seg[tid] = -1;
    if (stats) {
        __syncthreads();  // s_seg initialised
        sink_count_segments<FW_THREADS>(a, seg_first, own0, own1 - 1, s_seg);
    }
    SinkPlan plan{};
    SinkAcc acc;
    for (int r = 0; r < FW_ROUNDS; ++r) {
        const long long rbase = start + r * FW_ROUND;
        if (rbase >= own1) break;  // (the whole block leaves together)
        const long long base = rbase + static_cast<long long>(tid) * SC_ITEMS;
        float u[SC_ITEMS];
        double s = windowed_round<SRC>(a, base, own1, skip0, s_w[r & 1], s_run, u);
        if (r == 0) plan = sink_plan(a, stats, s_seg);  // behind the round's barrier: the counts are complete
        if (base + SC_ITEMS <= own0 || base >= own1) continue;  // warm-up only, or behind the end: nothing to emit
        acc.seg = plan.seg0;
        if (plan.general) acc.seg = lower_bound_ll(a.segs, a.n_segs, max(base, own0) + 1) - 1;
        float vout[SC_ITEMS];
#pragma unroll
        for (int i = 0; i < SC_ITEMS; ++i) {
            const long long idx = base + i;
            if (idx < own1) {
                const Aff mi = fmap<F_DEEMPH>(a, idx, u[i], 0.f, false);
                s = fma(mi.A, s, mi.B);
            }
            vout[i] = 0.f;
            if (idx >= own0 && idx < own1) vout[i] = sink_item<SINK>(a, plan, acc, static_cast<float>(s), idx);
        }
        sink_flush_general(a, plan, acc);  // (a thread's samples of the next round do not follow these)
        store_items(a, base, own0, own1, vout);
    }
    if constexpr (SINK == K_CLIP) sink_finish<FW_WAVES>(a, plan, acc, s_pk, s_sq);
    if (blockIdx.x != 0) return;
    // Block 0 hands the streaming state to the next call.  Every read of the incoming state (round 0, in front of its
    // barrier) lies behind it.  One block: s_run is the exact chain's state at n - 1.  More: a warm-up over the last
    // `window` samples (from a multiple of 8, so the vector loads stay aligned), rounds of its own.
    if (a.nblocks > 1) {
        // t0 >= 0 (n > own >= window); it is 0 only where window == own and n < window + 8: the warm-up then runs from
        // index 0 from state 0, not from the carried state, which costs alpha^(n-1) |state| <= 2^-64 S like any other
        const long long t0 = (a.n - window) & ~7LL;
        s_run = 0.0;
        __syncthreads();  // the last round's table has been read
        for (int r = 0; t0 + r * FW_ROUND < a.n; ++r) {
            float u[SC_ITEMS];
            windowed_round<SRC>(a, t0 + r * FW_ROUND + static_cast<long long>(tid) * SC_ITEMS, a.n, false, s_w[r & 1], s_run, u);
        }
    }
    if (tid == 0) {
        if constexpr (SRC == S_QUAD) prev_out[0] = a.z[a.n - 1];
        st_out[0] = s_run;
    }
}

template <int OP, int SRC, int SINK>
static int launch_fused(FusedArgs a, float2 *prev_out, double *st_out, void *work, hipStream_t s)
{
    if constexpr (OP == F_DEEMPH) {
        long long window;
        if (scan_window(a.p0, &window) == 0) {
            const long long own = FW_SPAN - window;
            a.nblocks = static_cast<int>((a.n + own - 1) / own);
            if (a.fresh && (a.peak_bits != nullptr || a.sumsq != nullptr))
                hipLaunchKernelGGL(k_fused_clear, dim3(1), dim3(FC_THREADS), 0, s, static_cast<float *>(nullptr), a.peak_bits, a.sumsq,
                                   a.n_segs * IQA_SUMSQ_SLOTS);
            hipLaunchKernelGGL((k_fused_windowed<SRC, SINK>), dim3(a.nblocks), dim3(FW_THREADS), 0, s, a, window, prev_out, st_out);
            return check_launch("windowed demodulator");
        }
    }
    a.nblocks = static_cast<int>((a.n + SC_TILE - 1) / SC_TILE);
    char *w = static_cast<char *>(work);
    a.agg = reinterpret_cast<Aff *>(w);
    a.carry = reinterpret_cast<double *>(w + sizeof(Aff) * a.nblocks);
    a.fin = a.carry + a.nblocks;
    hipLaunchKernelGGL((k_fused_reduce<OP, SRC>), dim3(a.nblocks), dim3(SC_THREADS), 0, s, a);
    hipLaunchKernelGGL((k_fused_carry<OP>), dim3(1), dim3(FC_THREADS), 0, s, a);
    FusedArgs b = a;  // the apply pass reads the incoming state from the carry pass's snapshot
    b.prev = reinterpret_cast<const float2 *>(a.fin + 1);
    b.st = a.fin + 2;
    b.fresh = 0;
    hipLaunchKernelGGL((k_fused_apply<OP, SRC, SINK>), dim3(a.nblocks), dim3(SC_THREADS), 0, s, b, prev_out, st_out);
    return check_launch("fused demodulator");
}

}  // namespace iqa

using namespace iqa;

static int demodulate(const iqa_demod_params *p, const void *z_dev, int64_t n, void *state_dev, const void *seg_starts_dev,
                      int64_t n_segs, void *peak_dev, void *sumsq_dev, void *audio_out_dev, void *scratch_dev, void *work_dev,
                      void *stream, int fresh)
{
    if (p == nullptr) return fail_inval("params is NULL");
    if (n < 0 || n_segs < 0) return fail_inval("negative length");
    if (p->mode < IQA_DEMOD_NFM || p->mode > IQA_DEMOD_LSB) return fail_inval("Unsupported demod mode");
    if (n == 0) return IQA_OK;
    if (!z_dev || !state_dev || !audio_out_dev || !work_dev) return fail_inval("NULL device pointer");
    if (n_segs > 0 && !seg_starts_dev) return fail_inval("seg_starts is NULL");
    hipStream_t s = as_stream(stream);
    // state block: [0] float2 prev (8 B) | [8] double y_last | [16] double x_last, y_last
    char *st = static_cast<char *>(state_dev);
    FusedArgs a{};
    a.fresh = fresh;
    a.z = static_cast<const float2 *>(z_dev);
    a.n = n;
    a.segs = static_cast<const long long *>(seg_starts_dev);
    a.n_segs = n_segs;
    a.peak_bits = static_cast<unsigned int *>(peak_dev);
    a.sumsq = static_cast<double *>(sumsq_dev);
    a.y = static_cast<float *>(audio_out_dev);
    a.z_aligned = (reinterpret_cast<uintptr_t>(z_dev) & 15) == 0;
    a.y_aligned = (reinterpret_cast<uintptr_t>(audio_out_dev) & 15) == 0;
    a.prev = reinterpret_cast<const float2 *>(st);
    if (p->mode == IQA_DEMOD_NFM) {
        a.p0 = p->deemph_alpha;
        a.p1 = 1.0 - p->deemph_alpha;
        a.st = reinterpret_cast<const double *>(st + 8);
        return launch_fused<F_DEEMPH, S_QUAD, K_CLIP>(a, reinterpret_cast<float2 *>(st), reinterpret_cast<double *>(st + 8),
                                                      work_dev, s);
    }
    if (!(p->dc_radius > 0.0 && p->dc_radius < 1.0)) return fail_inval("radius must be between 0 and 1");
    a.p0 = static_cast<double>(static_cast<float>(p->dc_radius));
    a.st = reinterpret_cast<const double *>(st + 16);
    double *dc_out = reinterpret_cast<double *>(st + 16);
    if (p->mode == IQA_DEMOD_AM) return launch_fused<F_DC, S_ENV, K_CLIP>(a, nullptr, dc_out, work_dev, s);
    if (!p->agc_enabled) return launch_fused<F_DC, S_REAL, K_CLIP>(a, nullptr, dc_out, work_dev, s);
    // SSB with AGC: DC blocker into scratch, then the segmented AGC scan with the writer sink
    if (!scratch_dev) return fail_inval("SSB with AGC needs a float scratch buffer of n elements");
    FusedArgs d = a;
    d.y = static_cast<float *>(scratch_dev);
    d.y_aligned = (reinterpret_cast<uintptr_t>(scratch_dev) & 15) == 0;
    d.peak_bits = nullptr;
    d.sumsq = nullptr;
    int rc = launch_fused<F_DC, S_REAL, K_PLAIN>(d, nullptr, dc_out, work_dev, s);
    if (rc != IQA_OK) return rc;
    FusedArgs g = a;
    g.z = nullptr;
    g.x = static_cast<const float *>(scratch_dev);
    g.p0 = static_cast<double>(static_cast<float>(p->agc_target));
    g.p1 = static_cast<double>(static_cast<float>(p->agc_decay));
    g.st = nullptr;
    return launch_fused<F_AGC, S_F32, K_CLIP>(g, nullptr, nullptr, work_dev, s);
}

extern "C" int iqa_demodulate(const iqa_demod_params *p, const void *z_dev, int64_t n, void *state_dev,
                              const void *seg_starts_dev, int64_t n_segs, void *peak_dev, void *sumsq_dev,
                              void *audio_out_dev, void *scratch_dev, void *work_dev, void *stream)
{
    return demodulate(p, z_dev, n, state_dev, seg_starts_dev, n_segs, peak_dev, sumsq_dev, audio_out_dev, scratch_dev, work_dev, stream, 0);
}

extern "C" int iqa_demodulate_from_reset(const iqa_demod_params *p, const void *z_dev, int64_t n, void *state_dev,
                                         const void *seg_starts_dev, int64_t n_segs, void *peak_dev, void *sumsq_dev,
                                         void *audio_out_dev, void *scratch_dev, void *work_dev, void *stream)
{
    if (n == 0) return fail_inval("iqa_demodulate_from_reset needs samples (an empty block resets nothing)");
    return demodulate(p, z_dev, n, state_dev, seg_starts_dev, n_segs, peak_dev, sumsq_dev, audio_out_dev, scratch_dev, work_dev, stream, 1);
}

extern "C" int iqa_demod_reset(void *state_dev, void *peak_dev, void *sumsq_dev, int64_t n_sums, void *stream)
{
    if (n_sums < 0) return fail_inval("negative length");
    if (!state_dev) return fail_inval("NULL device pointer");
    if (n_sums > 0 && !sumsq_dev) return fail_inval("sumsq is NULL");
    hipLaunchKernelGGL(k_fused_clear, dim3(1), dim3(FC_THREADS), 0, as_stream(stream), static_cast<float *>(state_dev),
                       static_cast<unsigned int *>(peak_dev), static_cast<double *>(sumsq_dev), (long long)n_sums);
    return check_launch("k_fused_clear");
}

extern "C" int iqa_scan_window(double alpha, int64_t *window, int64_t *span)
{
    long long w = 0;
    if (scan_window(alpha, &w) != 0) return 1;
    if (window != nullptr) *window = w;
    if (span != nullptr) *span = FW_SPAN;
    return 0;
}

extern "C" int64_t iqa_scan_workspace_bytes(int64_t n)
{
    const int64_t nb = (n + SC_TILE - 1) / SC_TILE;
    return nb * (sizeof(Aff) + sizeof(double)) + 64;
}

// ---- the stage API: one recurrence, float input, unclipped output -------------------------------

static FusedArgs stage_args(const void *x_dev, int64_t n, void *y_dev)
{
    FusedArgs a{};
    a.x = static_cast<const float *>(x_dev);
    a.y = static_cast<float *>(y_dev);
    a.n = n;
    a.y_aligned = (reinterpret_cast<uintptr_t>(y_dev) & 15) == 0;
    return a;
}

extern "C" int iqa_deemphasis(const void *x_dev, int64_t n, double alpha, void *state_dev, void *y_dev,
                              void *work_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!x_dev || !state_dev || !y_dev || !work_dev) return fail_inval("NULL device pointer");
    FusedArgs a = stage_args(x_dev, n, y_dev);
    a.p0 = alpha;
    a.p1 = 1.0 - alpha;
    a.st = static_cast<const double *>(state_dev);
    return launch_fused<F_DEEMPH, S_F32, K_PLAIN>(a, nullptr, static_cast<double *>(state_dev), work_dev, as_stream(stream));
}

extern "C" int iqa_dc_block(const void *x_dev, int64_t n, double radius, void *state_dev, void *y_dev,
                            void *work_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (!(radius > 0.0 && radius < 1.0)) return fail_inval("radius must be between 0 and 1");
    if (n == 0) return IQA_OK;
    if (!x_dev || !state_dev || !y_dev || !work_dev) return fail_inval("NULL device pointer");
    FusedArgs a = stage_args(x_dev, n, y_dev);
    a.p0 = static_cast<double>(static_cast<float>(radius));  // the reference's in-loop r is float32
    a.st = static_cast<const double *>(state_dev);
    return launch_fused<F_DC, S_F32, K_PLAIN>(a, nullptr, static_cast<double *>(state_dev), work_dev, as_stream(stream));
}

extern "C" int iqa_agc(const void *x_dev, int64_t n, double target, double decay, const void *reset_starts_dev,
                       int64_t n_resets, void *y_dev, void *work_dev, void *stream)
{
    if (n < 0 || n_resets < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!x_dev || !y_dev || !work_dev) return fail_inval("NULL device pointer");
    FusedArgs a = stage_args(x_dev, n, y_dev);
    a.p0 = static_cast<double>(static_cast<float>(target));
    a.p1 = static_cast<double>(static_cast<float>(decay));
    a.segs = static_cast<const long long *>(reset_starts_dev);  // the restarts (element 0 always restarts)
    a.n_segs = n_resets;
    return launch_fused<F_AGC, S_F32, K_PLAIN>(a, nullptr, nullptr, work_dev, as_stream(stream));
}

// ---- the source stages -----------------------------------------------------------------------------

extern "C" int iqa_quadrature(const void *z_dev, int64_t n, void *prev_dev, void *out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!z_dev || !prev_dev || !out_dev) return fail_inval("NULL device pointer");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_quadrature, grid1d(n, 256), dim3(256), 0, s, static_cast<const float2 *>(z_dev), (long long)n,
                       static_cast<const float2 *>(prev_dev), static_cast<float *>(out_dev));
    hipLaunchKernelGGL(k_store_last, dim3(1), dim3(1), 0, s, static_cast<const float2 *>(z_dev), (long long)n,
                       static_cast<float2 *>(prev_dev));
    return check_launch("k_quadrature");
}

extern "C" int iqa_envelope(const void *z_dev, int64_t n, void *out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!z_dev || !out_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_envelope, grid1d(n, 256), dim3(256), 0, as_stream(stream), static_cast<const float2 *>(z_dev),
                       (long long)n, static_cast<float *>(out_dev));
    return check_launch("k_envelope");
}

extern "C" int iqa_real_part(const void *z_dev, int64_t n, void *out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!z_dev || !out_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_real, grid1d(n, 256), dim3(256), 0, as_stream(stream), static_cast<const float2 *>(z_dev),
                       (long long)n, static_cast<float *>(out_dev));
    return check_launch("k_real");
}
