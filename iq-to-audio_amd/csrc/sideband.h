// sideband.h -- what the side decoders' kernels share (afsk.hip, acars.hip, ais.hip, pocsag.hip), for
// gfx950: one tile layout, the register-window FIR on it, the sampling instant, the CRC step, the HDLC walk, the frame
// emission and the host checks of the frame entry points.
//
// The tile.  A workgroup of SB_THREADS = 256 threads owns SB_TILE = 2048 consecutive samples, a thread SB_RUN = 8
// consecutive ones.  It quantises them and ``front`` values in front of them into LDS (sb_stage); image index i lives at
// word sb_pad(i) = i + i / 8.  Lanes are 8 samples apart, so a fixed tap of consecutive lanes is 9 words apart:
// conflict-free on the 32 banks a ds_read_b32 half-wave sees.
//
// The front.  A FIR of W taps stages front = H = sb_front(W) = W - 1 rounded up to 8 values.  Tap 0 reads the thread's own
// 8 values; taps 1 .. W - 1 go in groups of 8, zero-padded to H, each group reading the 8 values in front of the register
// window (sb_fir_run8).  Every staged value is used, nothing in front of the image is touched, and a W that is a multiple
// of 8 plus 1 costs no group of its own.
#pragma once

#include "common.h"

namespace iqa {

constexpr int SB_THREADS = 256;
constexpr int SB_RUN = 8;                       // consecutive outputs of a thread, and the tap group
constexpr int SB_TILE = SB_THREADS * SB_RUN;    // 2048

__host__ __device__ constexpr int sb_pad(int i) { return i + (i >> 3); }
__host__ __device__ constexpr int sb_round8(int v) { return (v + SB_RUN - 1) / SB_RUN * SB_RUN; }
__host__ __device__ constexpr int sb_front(int W) { return sb_round8(W - 1); }  // H of a FIR of W taps
// LDS words of sb_fir_run8<NF>: the tap tables and the image
__host__ __device__ constexpr int sb_fir_words(int NF, int W) { return NF * sb_front(W) + sb_pad(sb_front(W) + SB_TILE) + 1; }

// acc += a b for |a|, |b| < 2^23 (the low 32 bits of the 24-bit product; the operands are sign-extended from bit 23, which is
// why iqa_hotpath.h makes |t| < 2^23 a precondition of iqa_afsk_correlate).  Written out: from ``acc += __mul24(a, b)`` the
// compiler makes 256 separate products per tap group and adds them three at a time, 1.5 instructions and a live register
// per multiply-add.
__device__ __forceinline__ void sb_mad24(int &acc, int a, int b)
{
    asm("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}

// ---- staging ----------------------------------------------------------------------------------------------------------------

struct SbScale {  // rint(x k), half-even
    float k;
    __device__ int operator()(float x) const { return __float2int_rn(x * k); }
};
struct SbLdexp {  // rint(x 2^sh), half-even
    int sh;
    __device__ int operator()(float x) const { return __float2int_rn(ldexpf(x, sh)); }
};

// s[sb_pad(i)] = the value at absolute index a = A - front + i, i = 0 .. front + SB_TILE - 1: quant(x[a]) for 0 <= a < n,
// hist[hist_len + a] for -hist_len <= a < 0 (hist == NULL: zeros), zero elsewhere.  plane != NULL also receives the
// quantised values of image indices i >= plane_from.  The caller places the barrier.
template <class Quant>
__device__ __forceinline__ void sb_stage(int *s, int front, long long A, long long n, const float *__restrict__ x, Quant quant,
                                         const int *__restrict__ hist, int hist_len, int *__restrict__ plane, int plane_from)
{
    for (int i = threadIdx.x; i < front + SB_TILE; i += SB_THREADS) {
        const long long a = A - front + i;
        int v = 0;
        if (a < 0) {
            if (hist && a >= -hist_len) v = hist[hist_len + a];
        } else if (a < n) {
            v = quant(x[a]);
            if (plane && i >= plane_from) plane[a] = v;
        }
        s[sb_pad(i)] = v;
    }
}

// ---- the register-window FIR ------------------------------------------------------------------------------------------------

// s_taps[j][f] = table f's tap 1 + j, j = 0 .. H - 1, zero for 1 + j >= W; ``taps`` is [NF][W] in global memory.
template <int NF>
__device__ __forceinline__ void sb_stage_taps(int *s_taps, const short *__restrict__ taps, int W, int H)
{
    for (int j = threadIdx.x; j < H; j += SB_THREADS)
#pragma unroll
        for (int f = 0; f < NF; ++f) s_taps[j * NF + f] = (1 + j < W) ? taps[f * W + 1 + j] : 0;
}

// acc[f][r] = sum_{k < W} tap_f[k] x[first + r - k] for r = 0 .. 7 and NF interleaved tables: tap0[f] = tap_f[0], s_taps as
// sb_stage_taps leaves it (16-byte aligned), x the padded image, ``first`` the image index (unpadded) of the thread's first
// output, first >= H.  Per group of 8 taps: 8 more x into a register window of 16, 2 NF int4 of taps read at a wave-uniform
// address (a broadcast), 8 x 8 x NF 24-bit multiply-adds (|x| < 2^23 and |tap| < 2^23; the sums wrap in int32).
template <int NF>
__device__ __forceinline__ void sb_fir_run8(const int4 *s_taps, const int *s_x, int first, int H, const int (&tap0)[NF], int (&acc)[NF][SB_RUN])
{
    // w[j] = x at image index first - kb - 8 + j, j = 0 .. 15: output r, tap 1 + kb + kk reads index first + r - 1 - kb - kk = w[7 + r - kk]
    int w[2 * SB_RUN];
#pragma unroll
    for (int j = 0; j < SB_RUN; ++j) {
        w[SB_RUN + j] = s_x[sb_pad(first + j)];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            acc[f][j] = 0;
            sb_mad24(acc[f][j], tap0[f], w[SB_RUN + j]);
        }
    }
    for (int kb = 0; kb < H; kb += SB_RUN) {
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j) w[j] = s_x[sb_pad(first - kb - SB_RUN + j)];  // (first - kb - 8 >= H - (H - 8) - 8 = 0)
        int tp[SB_RUN * NF];
#pragma unroll
        for (int q = 0; q < 2 * NF; ++q) {
            const int4 t = s_taps[kb * NF / 4 + q];
            tp[4 * q] = t.x, tp[4 * q + 1] = t.y, tp[4 * q + 2] = t.z, tp[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int kk = 0; kk < SB_RUN; ++kk)
#pragma unroll
            for (int r = 0; r < SB_RUN; ++r)
#pragma unroll
                for (int f = 0; f < NF; ++f) sb_mad24(acc[f][r], tp[kk * NF + f], w[SB_RUN - 1 + r - kk]);
#pragma unroll
        for (int j = 0; j < SB_RUN; ++j) w[SB_RUN + j] = w[j];
    }
}

// The flags of outputs a0 .. a0 + 7 (a0 a multiple of 8) that lie below n: one 8-byte store where the run is whole and the
// plane is 8-byte aligned, byte stores otherwise.
__device__ __forceinline__ void sb_store_flags8(unsigned char *plane, long long a0, long long n, const unsigned char (&flag)[SB_RUN])
{
    if (a0 + SB_RUN <= n && (reinterpret_cast<uintptr_t>(plane) & 7u) == 0) {
        unsigned long long packed = 0;
#pragma unroll
        for (int r = 0; r < SB_RUN; ++r) packed |= static_cast<unsigned long long>(flag[r]) << (8 * r);
        *reinterpret_cast<unsigned long long *>(plane + a0) = packed;
        return;
    }
#pragma unroll
    for (int r = 0; r < SB_RUN; ++r)
        if (a0 + r < n) plane[a0 + r] = flag[r];
}

// ---- symbols and frames -----------------------------------------------------------------------------------------------------

// The instant of symbol i of phase p behind a detector of ``front`` taps: one float64 product, one rint (half-even).
__device__ __forceinline__ long long sb_instant(int front, double step, long long i, int p)
{
    return front - 1 + static_cast<long long>(rint(static_cast<double>(8 * i + p) * step));
}

// One byte into a reflected CRC-16 register, polynomial 0x8408 (X.25 / KERMIT: the caller sets the start value and the
// final inversion).
__device__ __forceinline__ unsigned sb_crc16_step(unsigned reg, unsigned byte)
{
    reg ^= byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) reg = (reg & 1u) ? (reg >> 1) ^ 0x8408u : reg >> 1;
    return reg;
}

// The HDLC walk from bit s of nb: bytes LSB first, a zero after five ones dropped, a sixth one ends the walk (a closing flag
// iff the next bit is 0 and 6 bits of the current byte are collected).  -1 for an abort / more than MAX_BYTES bytes / the
// end of the stream, else the byte count.  crc_ok: the CRC-16/X.25 of all but the last two bytes equals them (low byte
// first): three registers one byte apart.  out != NULL also stores the bytes.
// The bit source: ``bit(j)`` is called once per j, ascending from s, and may carry state; ``ahead(j)`` gives bit j behind
// bit(j - 1) and leaves the source as it is.
template <int MAX_BYTES, class Source>
__device__ int sb_hdlc_walk(Source src, long long s, long long nb, unsigned char *out, bool &crc_ok)
{
    unsigned cur = 0, c0 = 0xFFFFu, c1 = 0xFFFFu, c2 = 0xFFFFu, last = 0, last2 = 0;  // c0: over all bytes; c2: all but two
    int have = 0, ones = 0, nbytes = 0;
    crc_ok = false;
    for (long long j = s; j < nb; ++j) {
        const unsigned bit = src.bit(j);
        if (bit) {
            if (++ones == 6) {
                if (!(j + 1 < nb && src.ahead(j + 1) == 0 && have == 6)) return -1;
                crc_ok = nbytes >= 2 && ((c2 ^ 0xFFFFu) & 0xFFFFu) == (last2 | (last << 8));
                return nbytes;
            }
        } else {
            const bool stuffed = ones == 5;
            ones = 0;
            if (stuffed) continue;
        }
        cur |= bit << have;
        if (++have == 8) {
            if (nbytes == MAX_BYTES) return -1;
            if (out) out[nbytes] = static_cast<unsigned char>(cur);
            ++nbytes;
            c2 = c1, c1 = c0, c0 = sb_crc16_step(c0, cur);
            last2 = last, last = cur;
            cur = 0, have = 0;
        }
    }
    return -1;
}

// What a frame kernel reads: T the element of the symbol plane.
template <class T, int PHASES>
struct SbFrameArgs {
    const T *plane;             // [variants][n]
    long long n;
    long long count_of[PHASES]; // symbols of phase p that exist
    long long *list;            // [capacity][4]: key, s, start instant, nbytes
    unsigned char *slots;       // [capacity][slot bytes]
    long long capacity;
    unsigned long long *counts; // [2]: kept frames; candidates
    double step;                // sps / 8
    int front;                  // the detector's taps (sb_instant)
};

// One candidate: counted in counts[1]; where it is kept it takes a place from counts[0], and where that lies below the
// capacity its list entry (key, s, instant, nbytes) is written and its slot handed back (else NULL).
template <class T, int PHASES>
__device__ __forceinline__ unsigned char *sb_emit(const SbFrameArgs<T, PHASES> &g, bool kept, int slot_bytes, int key, long long s, int p, int nbytes)
{
    atomicAdd(g.counts + 1, 1ULL);
    if (!kept) return nullptr;
    const unsigned long long at = atomicAdd(g.counts, 1ULL);
    if (at >= static_cast<unsigned long long>(g.capacity)) return nullptr;
    long long *e4 = g.list + 4 * at;
    e4[0] = key;
    e4[1] = s;
    e4[2] = sb_instant(g.front, g.step, s, p);
    e4[3] = nbytes;
    return g.slots + at * slot_bytes;
}

// ---- host side of the frame entry points ------------------------------------------------------------------------------------

// dst = count_of where every entry is 0 .. limit (else false, and the caller names the limit in its error).
template <int PHASES>
inline bool sb_copy_counts(const int64_t *count_of, int64_t limit, long long (&dst)[PHASES])
{
    for (int p = 0; p < PHASES; ++p) {
        if (count_of[p] < 0 || count_of[p] > limit) return false;
        dst[p] = count_of[p];
    }
    return true;
}

inline int sb_clear_counts(void *counts_dev, void *stream)
{
    if (hipMemsetAsync(counts_dev, 0, 2 * sizeof(long long), as_stream(stream)) != hipSuccess) {
        set_error("clearing the frame counts failed");
        return IQA_EHIP;
    }
    return IQA_OK;
}

// What the checks leave to fill in.
template <class T, int PHASES>
inline void sb_fill_frames(SbFrameArgs<T, PHASES> &g, const void *plane_dev, int64_t n, void *list_dev, void *slots_dev, int64_t capacity,
                           void *counts_dev, double step, int front)
{
    g.plane = static_cast<const T *>(plane_dev);
    g.n = n;
    g.list = static_cast<long long *>(list_dev);
    g.slots = static_cast<unsigned char *>(slots_dev);
    g.capacity = capacity;
    g.counts = static_cast<unsigned long long *>(counts_dev);
    g.step = step;
    g.front = front;
}

// A thread per position s = 0 .. n (a frame may open behind the last symbol's flag) and a row per variant.
inline dim3 sb_frames_grid(int64_t n, int variants)
{
    dim3 grid = grid1d(n + 1, SB_THREADS);
    grid.y = variants;
    return grid;
}

}  // namespace iqa
