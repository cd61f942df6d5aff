// adsb.hip -- ADS-B / Mode S squitters (1090 MHz pulse position modulation) beside the AM demodulator (DESIGN.md section
// 17), for gfx950.  k_adsb_quantise runs per block; k_adsb_search once per run, on the run's stored q plane.
//
// Specification (fs the channel rate, e = |z|, all indices absolute; sps = fs / 1e6, h = floor(sps / 2),
// o[k] = rint(k sps / 2) for k < 240, span = o[239] + h):
//   q[n]   = 65535 unless e[n] 65536 < 65535, else rint(e[n] 65536)      (uint16, half-even; integers from here on)
//   C_k(p) = sum_{j<h} q[p + o[k] + j]                                    (int32; p is a position iff p + span <= N)
//   P      = C0 + C2 + C7 + C9; p passes the preamble rule iff C0 > C1, C2 > C1, C2 > C3, C7 > C6, C7 > C8, C9 > C8,
//            C9 > C10 and 6 C_j < P for j = 4, 5, 11, 12, 13, 14
//   b_i    = (C_{16+2i} > C_{17+2i}), i < 112; DF = b_0 .. b_4; nbits = 112 for DF >= 16, else 56
//   kept iff p passes, DF is 11, 17 or 18 and the first nbits bits leave no remainder under 0x1FFF409.
//
// k_adsb_search: a workgroup owns AD_TILE consecutive positions.  It stages q[tile .. tile + AD_TILE + span) as halfwords
// in LDS (zero behind the stream: no position reads there), then the chip sum w[i] = sum_{j<h} q[i + j] of every staged
// sample as one int32 plane, so that a chip is ONE LDS read at any rate: C_k(p) = w[p + o[k]].  o[k] is read from global
// memory at a wave-uniform index (a scalar load); for a fixed chip consecutive lanes read consecutive words of w:
// conflict-free.  Pass 1 tests the preamble rule at every position (15 reads) and appends the passing ones to a list in
// LDS through one LDS counter; pass 2 walks that list densely, one passing position per lane (224 reads, the check, the
// record), so that a wave is not dragged through the slice by the few lanes that passed.
#include "common.h"

namespace iqa {

constexpr int AD_THREADS = 256;
constexpr int AD_TILE = IQA_ADSB_TILE;
constexpr int AD_PER_THREAD = AD_TILE / AD_THREADS;
constexpr int AD_MAX_H = IQA_ADSB_MAX_SPS / 2;
constexpr unsigned AD_GENERATOR = 0x1FFF409u;

// ---- the quantiser ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(AD_THREADS) void k_adsb_quantise(const float *__restrict__ e, long long n, unsigned short *__restrict__ q)
{
    const long long stride = static_cast<long long>(gridDim.x) * AD_THREADS;
    for (long long i = static_cast<long long>(blockIdx.x) * AD_THREADS + threadIdx.x; i < n; i += stride) {
        const float x = e[i] * 65536.0f;  // exact, or +inf
        // (NaN fails the comparison and gives 65535; fmaxf keeps a negative value, outside the precondition, at 0)
        q[i] = x < 65535.0f ? static_cast<unsigned short>(static_cast<int>(rintf(fmaxf(x, 0.0f)))) : static_cast<unsigned short>(65535);
    }
}

// ---- the search ---------------------------------------------------------------------------------------------------------

struct AdsbSearchArgs {
    const unsigned short *q;     // [n]
    const int *o;                // [240]
    unsigned char *flags;        // [npos] or NULL
    long long *list;             // [capacity][3]: position, nbits, P
    unsigned char *slots;        // [capacity][IQA_ADSB_SLOT_BYTES]
    long long capacity;
    unsigned long long *counts;  // [2]: kept frames; positions that passed the preamble rule
    long long n, npos;           // npos = n - span + 1
    int h, span;
};

constexpr size_t ad_lds_bytes(int span, int h)
{
    // w: int32[AD_TILE + span - h]; the list: uint16[AD_TILE]; q: uint16[AD_TILE + span], rounded up to whole words
    return static_cast<size_t>(AD_TILE + span - h) * 4 + static_cast<size_t>(AD_TILE) * 2 + static_cast<size_t>((AD_TILE + span + 1) / 2 * 2) * 2;
}

__global__ __launch_bounds__(AD_THREADS) void k_adsb_search(AdsbSearchArgs g)
{
    extern __shared__ int s_ad[];
    __shared__ int s_count;
    const int tid = threadIdx.x, h = g.h, span = g.span;
    const int nw = AD_TILE + span - h;  // the largest index read is AD_TILE - 1 + o[239] <= AD_TILE - 1 + span - h
    const int nq = AD_TILE + span;      // w[nw - 1] reads q up to nw - 1 + h - 1 = nq - 2
    int *s_w = s_ad;
    unsigned short *s_list = reinterpret_cast<unsigned short *>(s_w + nw);
    unsigned short *s_q = s_list + AD_TILE;
    const int *__restrict__ o = g.o;
    const long long t0 = static_cast<long long>(blockIdx.x) * AD_TILE;  // (< npos: the grid covers npos)
    if (tid == 0) s_count = 0;
    for (int j = tid; j < nq; j += AD_THREADS) {
        const long long a = t0 + j;
        s_q[j] = a < g.n ? g.q[a] : static_cast<unsigned short>(0);
    }
    __syncthreads();
    for (int i = tid; i < nw; i += AD_THREADS) {
        int sum = 0;
        for (int j = 0; j < h; ++j) sum += s_q[i + j];
        s_w[i] = sum;
    }
    __syncthreads();
    const long long left = g.npos - t0;
    const int live = left < AD_TILE ? static_cast<int>(left) : AD_TILE;
    // pass 1: the preamble rule at every position of the tile
#pragma unroll 2
    for (int r = 0; r < AD_PER_THREAD; ++r) {
        const int i = tid + r * AD_THREADS;
        if (i >= live) continue;
        int c[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) c[k] = s_w[i + o[k]];
        const int P = c[0] + c[2] + c[7] + c[9];
        bool pass = c[0] > c[1] && c[2] > c[1] && c[2] > c[3] && c[7] > c[6] && c[7] > c[8] && c[9] > c[8] && c[9] > c[10];
        pass = pass && 6 * c[4] < P && 6 * c[5] < P && 6 * c[11] < P && 6 * c[12] < P && 6 * c[13] < P && 6 * c[14] < P;
        if (g.flags) g.flags[t0 + i] = pass ? 1 : 0;
        if (pass) s_list[atomicAdd(&s_count, 1)] = static_cast<unsigned short>(i);  // (at most AD_TILE entries: one per position)
    }
    __syncthreads();
    const int count = s_count;
    if (count == 0) return;
    if (tid == 0) atomicAdd(g.counts + 1, static_cast<unsigned long long>(count));
    // pass 2: the passing positions, one per lane
    for (int idx = tid; idx < count; idx += AD_THREADS) {
        const int i = s_list[idx];
        unsigned w[4];
        unsigned reg = 0, reg56 = 0;
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
            const int nb = wd < 3 ? 32 : 16;
            unsigned acc = 0;
#pragma unroll 4
            for (int bb = 0; bb < nb; ++bb) {
                const int k = 16 + 2 * (32 * wd + bb);
                const unsigned bit = s_w[i + o[k]] > s_w[i + o[k + 1]] ? 1u : 0u;
                acc = (acc << 1) | bit;
                reg = (reg << 1) | bit;
                if (reg & 0x1000000u) reg ^= AD_GENERATOR;
                if (wd == 1 && bb == 23) reg56 = reg;  // behind bit 55
            }
            w[wd] = acc << (32 - nb);
        }
        const unsigned df = w[0] >> 27;
        const bool is_long = df >= 16;
        if (!(df == 11 || df == 17 || df == 18) || (is_long ? reg : reg56) != 0) continue;
        const unsigned long long at = atomicAdd(g.counts, 1ULL);
        if (at >= static_cast<unsigned long long>(g.capacity)) continue;
        if (!is_long) w[1] &= 0xFFFFFF00u, w[2] = 0, w[3] = 0;
        long long *e3 = g.list + 3 * at;
        e3[0] = t0 + i;
        e3[1] = is_long ? 112 : 56;
        e3[2] = s_w[i + o[0]] + s_w[i + o[2]] + s_w[i + o[7]] + s_w[i + o[9]];
        unsigned char *slot = g.slots + at * IQA_ADSB_SLOT_BYTES;
#pragma unroll
        for (int k = 0; k < IQA_ADSB_SLOT_BYTES; ++k) slot[k] = static_cast<unsigned char>(w[k >> 2] >> (24 - 8 * (k & 3)));
    }
}

static_assert(AD_TILE % AD_THREADS == 0 && AD_TILE <= 65536, "a tile is whole passes of the workgroup; list entries are uint16");
static_assert(ad_lds_bytes(IQA_ADSB_MAX_SPAN, 1) <= 64 * 1024, "the search's images must fit the default LDS allowance");
static_assert(6LL * AD_MAX_H * 65535 < (1LL << 31), "6 C_j and P stay inside int32");
static_assert(IQA_ADSB_MAX_SPAN >= IQA_ADSB_CHIPS * AD_MAX_H, "the longest span fits");

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_adsb_quantise(const void *e_dev, int64_t n, void *q_out_dev, void *stream)
{
    if (n < 0) return fail_inval("negative length");
    if (n == 0) return IQA_OK;
    if (!e_dev || !q_out_dev) return fail_inval("NULL device pointer");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    const int64_t blocks = (n + AD_THREADS * 8 - 1) / (AD_THREADS * 8);
    hipLaunchKernelGGL(k_adsb_quantise, dim3(static_cast<unsigned>(blocks < 65536 ? blocks : 65536)), dim3(AD_THREADS), 0, as_stream(stream),
                       static_cast<const float *>(e_dev), static_cast<long long>(n), static_cast<unsigned short *>(q_out_dev));
    return check_launch("k_adsb_quantise");
}

extern "C" int iqa_adsb_search(const void *q_dev, int64_t n, const void *offsets_dev, const int32_t *offsets_host, int32_t h, int32_t span,
                               void *flags_out_dev, void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream)
{
    if (n < 0 || capacity < 0) return fail_inval("negative length");
    if (!counts_dev) return fail_inval("NULL device pointer");
    if (!offsets_host) return fail_inval("NULL offset table");
    if (h < 1 || h > AD_MAX_H) return fail_inval("h must be 1 .. IQA_ADSB_MAX_SPS / 2");
    if (span < 1 || span > IQA_ADSB_MAX_SPAN) return fail_inval("span must be 1 .. IQA_ADSB_MAX_SPAN");
    if (offsets_host[0] != 0) return fail_inval("o[0] must be 0");
    for (int k = 1; k < IQA_ADSB_CHIPS; ++k)
        if (offsets_host[k] < offsets_host[k - 1]) return fail_inval("the offsets must ascend");
    if (static_cast<int64_t>(offsets_host[IQA_ADSB_CHIPS - 1]) + h > span) return fail_inval("o[239] + h must be <= span");
    if (n > (1LL << 40)) return fail_inval("length out of range");
    if (n >= span && (!q_dev || !offsets_dev || (capacity > 0 && (!list_dev || !slots_dev)))) return fail_inval("NULL device pointer");
    if (hipMemsetAsync(counts_dev, 0, 2 * sizeof(long long), as_stream(stream)) != hipSuccess) {  // (behind every check)
        set_error("clearing the frame counts failed");
        return IQA_EHIP;
    }
    if (n < span) return IQA_OK;
    AdsbSearchArgs g;
    g.q = static_cast<const unsigned short *>(q_dev);
    g.o = static_cast<const int *>(offsets_dev);
    g.flags = static_cast<unsigned char *>(flags_out_dev);
    g.list = static_cast<long long *>(list_dev);
    g.slots = static_cast<unsigned char *>(slots_dev);
    g.capacity = capacity;
    g.counts = static_cast<unsigned long long *>(counts_dev);
    g.n = n;
    g.npos = n - span + 1;
    g.h = h;
    g.span = span;
    hipLaunchKernelGGL(k_adsb_search, grid1d(g.npos, AD_TILE), dim3(AD_THREADS), ad_lds_bytes(span, h), as_stream(stream), g);
    return check_launch("k_adsb_search");
}
