// protocol.h -- what the kernels of the second pass's protocol layers share (ident.hip, flex.hip, dmr.hip, p25.hip, ysf.hip, nxdn.hip;
// DESIGN.md section 27), for gfx950: the bits of a word record, the sync word's levels, the Golay code over 0xC75, the workgroup minimum,
// the slicing of a four-level symbol against the levels of its sync word, and the host checks of the entry points.
//
// Words and codes.  A record is u32 words with the first sent bit the MSB of word 0 (pl_bit).  A 24-symbol sync word is 48 bits,
// symbol 0 on top, a dibit 01 = +3, 11 = -3: pl_sync_positive names a symbol's sign, pl_sync_ups counts the +3 (the balance that
// turns the sums over the sync symbols into the DC and the outer level).  pl_golay is the systematic encoder of the (23,12) code
// over 0xC75 with an even parity bit, shortened to data_bits; pl_golay_distance holds a table of its codewords to the code's
// distance at compile time.
//
// Workgroup.  pl_block_min: the minimum over keys (distance << k | value) that every thread has put into LDS.
//
// Slicing.  A hit row begins (m, s): m where sync symbol 0 ends on the integrator plane of section 25, s the sign of its
// correlation (pl_hit).  An instant m + o[i] is read only where it lies in [0, n) (pl_read).  pl_dibit slices d, a symbol less
// the DC, against the outer level amp, both at the layer's common scale; pl_pack_dibits packs sixteen of them into a word.
//
// Host.  pl_check_lengths and pl_copy_offsets are the prologue of the entry points: the limits of one stored stream and of one
// call, and the offset table o[i] = rint(i sps) that is passed by value to the kernels.
#pragma once

#include "common.h"

namespace iqa {

constexpr int64_t PL_MAX_N = 1LL << 30;       // samples of one stored stream: positions stay far inside int64, rows inside 2^31
constexpr int64_t PL_MAX_K = 1LL << 20;       // hits, frames or bursts of one call: at most 55 workgroups each inside the grid's 2^31
constexpr long long PL_V_MAX = 64LL * 65534;  // |v| of the integrator plane
constexpr unsigned PL_GOLAY_POLY = 0xC75u;

// ---- words and codes ----------------------------------------------------------------------------------------------------------

// bit b of a record, the first sent bit the MSB of word 0
__device__ inline unsigned pl_bit(const unsigned *w, int b) { return (w[b >> 5] >> (31 - (b & 31))) & 1u; }

__host__ __device__ constexpr unsigned pl_popcount(unsigned x)
{
    unsigned c = 0;
    for (; x; x &= x - 1) ++c;
    return c;
}

__host__ __device__ constexpr unsigned pl_parity(unsigned x)
{
    x ^= x >> 16;
    x ^= x >> 8;
    x ^= x >> 4;
    x ^= x >> 2;
    x ^= x >> 1;
    return x & 1u;
}

// whether symbol i (0 .. 23) of a sync word is a positive level: the dibits 01 (+3) and 00 (+1) have a clear first bit
__host__ __device__ constexpr bool pl_sync_positive(unsigned long long word, int i) { return ((word >> (2 * (23 - i) + 1)) & 1ull) == 0; }

// the +3 symbols of a sync word, or -1 where it holds an inner level (only 01 and 11 may occur)
constexpr int pl_sync_ups(unsigned long long word)
{
    int up = 0;
    for (int i = 0; i < 24; ++i) {
        if (((word >> (2 * (23 - i))) & 1ull) == 0) return -1;
        up += pl_sync_positive(word, i) ? 1 : 0;
    }
    return up;
}

// the codeword of a data_bits-bit value (at most 12): data << 12 | (data x^11 mod 0xC75) << 1 | even parity
__host__ __device__ constexpr unsigned pl_golay(unsigned data, int data_bits)
{
    unsigned r = data << 11;
    for (int i = data_bits + 10; i >= 11; --i)
        if ((r >> i) & 1u) r ^= PL_GOLAY_POLY << (i - 11);
    const unsigned cw = (data << 12) | ((r & 0x7FFu) << 1);
    return cw | pl_parity(cw);
}
static_assert(pl_golay(0x29, 8) == pl_golay(0x29, 12), "a shortened value has the codeword of the full code");

// The smallest weight of a nonzero codeword of a table (t.word(d), d < count), or 0 where the table is not linear.  Every word is
// held to the sum of the word of its lowest set bit and the word of the rest, so the table is linear, a difference of two
// codewords is a codeword, and the smallest nonzero weight is the smallest distance between two of them.
template <class Table>
constexpr unsigned pl_golay_distance(const Table &t, unsigned count)
{
    unsigned best = 32;
    for (unsigned d = 1; d < count; ++d) {
        if (t.word(d) != (t.word(d & (d - 1)) ^ t.word(d & (0u - d)))) return 0;
        const unsigned w = pl_popcount(t.word(d));
        if (w < best) best = w;
    }
    return t.word(0) == 0 ? best : 0;
}

// ---- workgroup ----------------------------------------------------------------------------------------------------------------

// the minimum of s_key[0 .. threads) over the workgroup (threads a power of two); every thread has written its entry
__device__ inline unsigned pl_block_min(unsigned *s_key, int tid, int threads)
{
    __syncthreads();
    for (int w = threads / 2; w >= 1; w >>= 1) {
        if (tid < w && s_key[tid + w] < s_key[tid]) s_key[tid] = s_key[tid + w];
        __syncthreads();
    }
    const unsigned key = s_key[0];
    __syncthreads();  // (the next round overwrites s_key only behind every read of it)
    return key;
}

// ---- slicing ------------------------------------------------------------------------------------------------------------------

struct PlHit {
    long long m, s;  // where sync symbol 0 ends; +-1
};
__device__ __forceinline__ PlHit pl_hit(const long long *row) { return {row[0], row[1] < 0 ? -1LL : 1LL}; }

// plane[at] where the instant lies in [0, n), else 0: nothing outside the plane is read
__device__ __forceinline__ int pl_read(const int *__restrict__ plane, long long n, long long at, bool &inside)
{
    inside = at >= 0 && at < n;
    return inside ? plane[at] : 0;
}

// the dibit of a symbol at d from the DC with the outer level amp: its first bit (d < 0), its second (3 |d| >= 2 amp)
__device__ __forceinline__ unsigned pl_dibit(long long d, long long amp)
{
    const long long mag = d < 0 ? -d : d;
    return (d < 0 ? 2u : 0u) | (3 * mag >= 2 * amp ? 1u : 0u);
}

// word ``lane`` of the dibits in s_two, sixteen to a word, the first the top two bits
__device__ __forceinline__ unsigned pl_pack_dibits(const unsigned char *s_two, int lane)
{
    unsigned word = 0;
    for (int k = 0; k < 16; ++k) word |= static_cast<unsigned>(s_two[16 * lane + k]) << (30 - 2 * k);
    return word;
}

// ---- host side of the entry points --------------------------------------------------------------------------------------------

// The lengths of a call: n samples of the plane and K items (``count`` the letter of the argument); 0 for the one that an entry
// point does not take.
inline int pl_check_lengths(int64_t n, int64_t K, char count = 'K')
{
    if (n < 0 || K < 0) return fail_inval("negative length");
    if (n > PL_MAX_N) return fail_inval("n must not exceed 2^30");
    if (K > PL_MAX_K) {
        set_error("invalid argument: %c must not exceed 2^20", count);
        return IQA_EINVAL;
    }
    return IQA_OK;
}

// dst = the table ``name`` of N offsets with o[0] at index ``lead``: o[0] = 0, strictly ascending, no step above the longest
// symbol plus the one sample that rounding adds.
inline int pl_copy_offsets(const int32_t *offsets, int N, int lead, const char *name, int *dst)
{
    if (!offsets) return fail_inval("NULL offsets");
    if (offsets[lead] != 0) {
        set_error("invalid argument: %s[%d] (o[0]) must be 0", name, lead);
        return IQA_EINVAL;
    }
    for (int i = 0; i < N; ++i) {
        const char *must = nullptr;
        if (i && offsets[i] <= offsets[i - 1]) must = "ascend";
        else if (i && offsets[i] - offsets[i - 1] > IQA_IDENT_MAX_SPS + 1) must = "not step by more than IQA_IDENT_MAX_SPS + 1";
        if (must) {
            set_error("invalid argument: %s must %s", name, must);
            return IQA_EINVAL;
        }
        dst[i] = offsets[i];
    }
    return IQA_OK;
}

}  // namespace iqa
