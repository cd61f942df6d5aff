// dmr.hip -- the bursts of DMR channels behind their sync words (--find-dmr), for gfx950: the levels and
// the 288 sliced bits of every kept sync hit, and the TACT, the slot type and the BPTC(196,96) payload of every sliced burst.
//
// Specification (plane the integrator plane v of section 25 at 4800 symbols/s, n samples; a hit (m, s, kind): m where sync
// symbol 0 ends, s the sign of its correlation, kind 0 bs voice, 1 bs data, 2 ms voice, 3 ms data; o[i] = rint(i sps),
// i = -66 .. 77, at index 66 + i; sgn_i the sign of symbol i of the bs or ms voice word):
//   k_dmr_slice, per hit:
//     the burst is valid iff every instant m + o[i], i = -54 .. 77, lies in [0, n); the CACH iff the kind is a bs one and every
//     instant of i = -66 .. -55 does
//     x_i = v[m + o[i]], i = 0 .. 23; Sigma = sum x_i, A = s sum sgn_i x_i                        (int64; 0 for a cut burst)
//     a read symbol: d = 24 v[instant] - Sigma; its first bit (d < 0), its second (3 |d| >= 2 A)
//     bits: u32[9], the 24 CACH bits then the 264 burst bits, the first sent bit the MSB of word 0; a cut burst's bits are 0, and
//     so are the CACH bits that are not read; levels: Sigma, A, flags (bit 0 burst valid, bit 1 CACH valid)
//   k_dmr_decode, per burst of 288 bits and its kind:
//     TACT (bs kinds): CACH bits {0, 4, 8, 12, 14, 18, 22} = AT, TC, LCSS1, LCSS0, P0, P1, P2, Hamming(7,4); status 0 clean, 1
//     one bit restored, 4 not sent; the nibble AT TC LCSS1 LCSS0
//     slot type (data kinds): burst bits 98 .. 107 and 156 .. 165, Golay(20,8): data << 12 | (data x^11 mod 0xC75) << 1 | even
//     parity; the nearest of the 256 codewords (ties cannot occur at a distance of 3 or less); status 0 clean, 1 corrected
//     (distance 1 .. 3), 2 refused (the raw top byte kept), 4 not sent
//     BPTC (data kinds, slot type not refused): raw = burst bits 0 .. 97, 166 .. 263; D[k] = raw[181 k mod 196]; 13 rows of 15 at
//     D[1 + 15 r + c]; up to five rounds of all columns (Hamming(13,9); the syndromes 1001 and 1101 name no bit), then rows
//     0 .. 8 (Hamming(15,11)); a round without a flip is the last; status 0 clean, 1 corrected, 2 failed, 4 not sent
//     info: D[4 .. 11], D[16 .. 26], D[31 .. 41], ..., D[121 .. 131], the first bit the MSB of word 0
//   rec: int32[8] = TACT status, TACT nibble, slot-type status, distance, byte, BPTC status, flips, rounds
//
// k_dmr_slice is one wave per hit: its lanes gather the 144 instants (three strided reads at the most), the levels are
// reduced across the wave, nine lanes pack the words.  k_dmr_decode is a workgroup of 256 per burst: a codeword of the slot
// type to a thread with a minimum over (distance, value), then the de-interleaved bits in LDS and a thread per column and per
// row under block-uniform barriers.  The sync word's signs, the Golay encoder, the minimum, the dibit rule, the packing and the
// host prologue are protocol.h's.  Plain C++ stores, no inline assembly, no atomics, no mutable statics.
#include "protocol.h"

namespace iqa {

constexpr int DM_WAVE = 64;
constexpr int DM_THREADS = 256;
constexpr int DM_OFFSETS = IQA_DMR_OFFSETS;  // 144: o[-66] .. o[77]
constexpr int DM_LEAD = 66;                  // o[i] sits at index 66 + i
constexpr int DM_CACH = 12;                  // CACH symbols, indices 0 .. 11
constexpr int DM_WORDS = IQA_DMR_WORDS;      // 9 words of 32 bits: 24 + 264
constexpr int DM_REC = IQA_DMR_RECORD;       // 8
constexpr int DM_ROUNDS = 5;
constexpr unsigned long long DM_BS_VOICE = 0x755FD7DF75F7ull, DM_MS_VOICE = 0x7F7D5DD57DFDull;

static_assert(24 * PL_V_MAX * 2 < (1LL << 40), "24 y - Sigma and 3 |d| stay far inside int64");
static_assert(DM_OFFSETS == 2 * DM_WAVE + 16 && 2 * DM_OFFSETS == 32 * DM_WORDS, "144 symbols: three passes of a wave, nine words");

struct DmrOffsets {
    int o[DM_OFFSETS];
};

static_assert(pl_sync_ups(DM_BS_VOICE) == 12 && pl_sync_ups(DM_MS_VOICE) == 12, "both sync words hold twelve +3 and twelve -3: Sigma / 24 is the DC");

// the slot type's codewords of the 8-bit values
struct DmrGolay {
    unsigned cw[256];
    constexpr unsigned word(unsigned d) const { return cw[d]; }
};

constexpr DmrGolay dm_golay_table()
{
    DmrGolay t{};
    for (unsigned d = 0; d < 256; ++d) t.cw[d] = pl_golay(d, 8);
    return t;
}

constexpr DmrGolay DM_GOLAY_HOST = dm_golay_table();
static_assert(DM_GOLAY_HOST.cw[1] == 0x18EBu && DM_GOLAY_HOST.cw[2] == 0x293Eu && DM_GOLAY_HOST.cw[4] == 0x4A97u, "the slot type's codewords of 1, 2 and 4");
static_assert(pl_golay_distance(DM_GOLAY_HOST, 256) == 8, "the 256 codewords lie 8 apart at the least: a word within 3 of one is within 3 of no other");
__device__ const DmrGolay DM_GOLAY = dm_golay_table();

// The parity checks as masks over a word whose bit j is d_j; check e covers the bits of its equation and its parity bit.
enum DmrCode { DM_H7 = 0, DM_H13 = 1, DM_H15 = 2 };
__host__ __device__ constexpr int dm_checks(int code) { return code == DM_H7 ? 3 : 4; }
__host__ __device__ constexpr int dm_length(int code) { return code == DM_H7 ? 7 : code == DM_H13 ? 13 : 15; }
__host__ __device__ constexpr unsigned dm_check(int code, int e)
{
    switch (4 * code + e) {
    case 0: return 0x17u;  // the TACT, d0 .. d3 = AT, TC, LCSS1, LCSS0: P0 = d0^d1^d2
    case 1: return 0x2Eu;  // P1 = d1^d2^d3
    case 2: return 0x4Bu;  // P2 = d0^d1^d3
    case 4: return 0x026Bu;  // a column: d9 = d0^d1^d3^d5^d6
    case 5: return 0x04D7u;  // d10 = d0^d1^d2^d4^d6^d7
    case 6: return 0x09AFu;  // d11 = d0^d1^d2^d3^d5^d7^d8
    case 7: return 0x1135u;  // d12 = d0^d2^d4^d5^d8
    case 8: return 0x09AFu;  // a row: d11 = d0^d1^d2^d3^d5^d7^d8
    case 9: return 0x135Eu;  // d12 = d1^d2^d3^d4^d6^d8^d9
    case 10: return 0x26BCu;  // d13 = d2^d3^d4^d5^d7^d9^d10
    case 11: return 0x44D7u;  // d14 = d0^d1^d2^d4^d6^d7^d10
    default: return 0;
    }
}

__host__ __device__ constexpr unsigned dm_syndrome(int code, unsigned word)
{
    unsigned syn = 0;
    for (int e = 0; e < dm_checks(code); ++e) syn |= pl_parity(word & dm_check(code, e)) << e;
    return syn;
}

// the position whose column of H is syn, or -1 where no column is
__host__ __device__ constexpr int dm_position(int code, unsigned syn)
{
    for (int j = 0; j < dm_length(code); ++j)
        if (dm_syndrome(code, 1u << j) == syn) return j;
    return -1;
}

constexpr int dm_named(int code)
{
    int named = 0;
    for (unsigned syn = 1; syn < (1u << dm_checks(code)); ++syn) named += dm_position(code, syn) >= 0 ? 1 : 0;
    return named;
}
static_assert(dm_named(DM_H7) == 7 && dm_named(DM_H15) == 15, "every nonzero syndrome of the TACT and of a row names one bit");
static_assert(dm_named(DM_H13) == 13 && dm_position(DM_H13, 0x9u) < 0 && dm_position(DM_H13, 0xBu) < 0,
              "a column's syndromes name 13 bits; (1,0,0,1) and (1,1,0,1) name none");

__global__ __launch_bounds__(DM_WAVE) void k_dmr_slice(const int *__restrict__ plane, long long n, const long long *__restrict__ hits,
                                                       DmrOffsets off, unsigned *__restrict__ bits_out, long long *__restrict__ levels_out)
{
    __shared__ unsigned char s_two[DM_OFFSETS];
    const int lane = threadIdx.x;
    const long long id = blockIdx.x;
    const PlHit hit = pl_hit(hits + 3 * id);
    const int kind = static_cast<int>(hits[3 * id + 2]) & 3;
    const bool bs = kind < 2;
    // the gather: every instant is checked against [0, n) before it is read
    int y[3] = {0, 0, 0};
    bool burst_in = true, cach_in = true;
    for (int p = 0; p < 3; ++p) {
        const int idx = p * DM_WAVE + lane;
        if (idx >= DM_OFFSETS) break;
        bool inside;
        y[p] = pl_read(plane, n, hit.m + off.o[idx], inside);
        if (idx < DM_CACH)
            cach_in = cach_in && inside;
        else
            burst_in = burst_in && inside;
    }
    const bool burst_ok = __all(burst_in), cach_ok = bs && __all(cach_in);
    // the levels: the sync symbols are indices 66 .. 89, all in the second pass (lanes 2 .. 25)
    const int i = lane - (DM_LEAD - DM_WAVE);
    const bool sync = i >= 0 && i < 24;
    long long sigma = sync ? y[1] : 0;
    long long amp = 0;
    if (sync) amp = pl_sync_positive(bs ? DM_BS_VOICE : DM_MS_VOICE, i) ? y[1] : -static_cast<long long>(y[1]);
    sigma = wave_sum(sigma);
    amp = hit.s * wave_sum(amp);
    if (!burst_ok) sigma = amp = 0;
    for (int p = 0; p < 3; ++p) {
        const int idx = p * DM_WAVE + lane;
        if (idx >= DM_OFFSETS) break;
        unsigned two = pl_dibit(24LL * y[p] - sigma, amp);
        if (!burst_ok || (idx < DM_CACH && !cach_ok)) two = 0;
        s_two[idx] = static_cast<unsigned char>(two);
    }
    __syncthreads();
    if (lane < DM_WORDS) bits_out[DM_WORDS * id + lane] = pl_pack_dibits(s_two, lane);
    if (lane == 0) {
        long long *e = levels_out + 3 * id;
        e[0] = sigma;
        e[1] = amp;
        e[2] = (burst_ok ? 1 : 0) | (cach_ok ? 2 : 0);
    }
}

// the index in D of information bit q (0 .. 95)
__device__ inline int dm_info_index(int q) { return q < 8 ? 4 + q : 1 + 15 * (1 + (q - 8) / 11) + (q - 8) % 11; }

__global__ __launch_bounds__(DM_THREADS) void k_dmr_decode(const unsigned *__restrict__ bits, const unsigned char *__restrict__ kinds,
                                                           unsigned *__restrict__ info_out, int *__restrict__ rec_out)
{
    __shared__ unsigned s_w[DM_WORDS];
    __shared__ unsigned s_key[DM_THREADS];
    __shared__ unsigned char s_d[196];
    __shared__ unsigned char s_flag[32];
    const int tid = threadIdx.x;
    const long long id = blockIdx.x;
    const int kind = kinds[id] & 3;
    const bool bs = kind < 2, data = (kind & 1) != 0;  // (block-uniform)
    if (tid < DM_WORDS) s_w[tid] = bits[DM_WORDS * id + tid];
    __syncthreads();
    const unsigned *cach = s_w;
    auto burst = [&](int b) { return pl_bit(s_w, 24 + b); };

    // the TACT: every thread reads the same seven bits
    int tact_status = 4, tact = 0;
    if (bs) {
        constexpr int at[7] = {0, 4, 8, 12, 14, 18, 22};
        unsigned word = 0;
        for (int j = 0; j < 7; ++j) word |= pl_bit(cach, at[j]) << j;
        const unsigned syn = dm_syndrome(DM_H7, word);
        tact_status = syn ? 1 : 0;
        if (syn) word ^= 1u << dm_position(DM_H7, syn);
        tact = static_cast<int>(((word & 1u) << 3) | ((word & 2u) << 1) | ((word & 4u) >> 1) | ((word & 8u) >> 3));
    }

    // the slot type: a codeword to a thread, the minimum over (distance, value)
    int st_status = 4, st_distance = 0, st_byte = 0;
    if (data) {
        unsigned word = 0;
        for (int j = 0; j < 10; ++j) word |= burst(98 + j) << (19 - j) | burst(156 + j) << (9 - j);
        s_key[tid] = (pl_popcount(word ^ DM_GOLAY.cw[tid]) << 8) | static_cast<unsigned>(tid);
        const unsigned key = pl_block_min(s_key, tid, DM_THREADS);
        st_distance = static_cast<int>(key >> 8);
        st_status = st_distance == 0 ? 0 : st_distance <= 3 ? 1 : 2;
        st_byte = st_status == 2 ? static_cast<int>(word >> 12) : static_cast<int>(key & 0xFFu);
    }

    // the payload
    int bptc_status = 4, flips = 0, rounds = 0;
    const bool read = data && st_status != 2;
    if (read) {
        if (tid < 196) {
            const int k = (181 * tid) % 196;
            s_d[tid] = static_cast<unsigned char>(burst(k < 98 ? k : k + 68));
        }
        __syncthreads();
        bool more = true;
        while (more && rounds < DM_ROUNDS) {
            ++rounds;
            if (tid < 32) s_flag[tid] = 0;
            __syncthreads();
            if (tid < 15) {  // column tid: d_r at D[1 + 15 r + tid]
                unsigned word = 0;
                for (int r = 0; r < 13; ++r) word |= static_cast<unsigned>(s_d[1 + 15 * r + tid]) << r;
                const unsigned syn = dm_syndrome(DM_H13, word);
                const int pos = syn ? dm_position(DM_H13, syn) : -1;
                if (pos >= 0) {
                    s_d[1 + 15 * pos + tid] ^= 1;
                    s_flag[tid] = 1;
                }
            }
            __syncthreads();
            if (tid < 9) {  // row tid
                unsigned word = 0;
                for (int c = 0; c < 15; ++c) word |= static_cast<unsigned>(s_d[1 + 15 * tid + c]) << c;
                const unsigned syn = dm_syndrome(DM_H15, word);
                if (syn) {
                    s_d[1 + 15 * tid + dm_position(DM_H15, syn)] ^= 1;
                    s_flag[15 + tid] = 1;
                }
            }
            __syncthreads();
            int flipped = 0;
            for (int j = 0; j < 24; ++j) flipped += s_flag[j];
            flips += flipped;
            more = flipped != 0;
            __syncthreads();  // (s_flag is cleared by the next round only behind every read of it)
        }
        if (tid < 32) s_flag[tid] = 0;
        __syncthreads();
        if (tid < 15) {
            unsigned word = 0;
            for (int r = 0; r < 13; ++r) word |= static_cast<unsigned>(s_d[1 + 15 * r + tid]) << r;
            s_flag[tid] = dm_syndrome(DM_H13, word) ? 1 : 0;
        } else if (tid < 24) {
            unsigned word = 0;
            for (int c = 0; c < 15; ++c) word |= static_cast<unsigned>(s_d[1 + 15 * (tid - 15) + c]) << c;
            s_flag[tid] = dm_syndrome(DM_H15, word) ? 1 : 0;
        }
        __syncthreads();
        int bad = 0;
        for (int j = 0; j < 24; ++j) bad += s_flag[j];
        bptc_status = bad ? 2 : flips ? 1 : 0;
    }
    if (tid < 3) {
        unsigned word = 0;
        if (read)
            for (int k = 0; k < 32; ++k) word |= static_cast<unsigned>(s_d[dm_info_index(32 * tid + k)]) << (31 - k);
        info_out[3 * id + tid] = word;
    }
    if (tid == 0) {
        int *e = rec_out + DM_REC * id;
        e[0] = tact_status;
        e[1] = tact;
        e[2] = st_status;
        e[3] = st_distance;
        e[4] = st_byte;
        e[5] = bptc_status;
        e[6] = flips;
        e[7] = rounds;
    }
}

}  // namespace iqa

using namespace iqa;

extern "C" int iqa_dmr_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_DMR_OFFSETS],
                             void *bits_dev, void *levels_dev, void *stream)
{
    DmrOffsets off;
    if (const int rc = pl_check_lengths(n, K)) return rc;
    if (const int rc = pl_copy_offsets(offsets, DM_OFFSETS, DM_LEAD, "offsets", off.o)) return rc;
    if (n == 0 || K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!plane_dev || !hits_dev || !bits_dev || !levels_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_dmr_slice, dim3(static_cast<unsigned>(K)), dim3(DM_WAVE), 0, as_stream(stream), static_cast<const int *>(plane_dev),
                       (long long)n, static_cast<const long long *>(hits_dev), off, static_cast<unsigned *>(bits_dev),
                       static_cast<long long *>(levels_dev));
    return check_launch("k_dmr_slice");
}

extern "C" int iqa_dmr_decode(const void *bits_dev, const void *kinds_dev, int64_t K, void *info_dev, void *rec_dev, void *stream)
{
    if (const int rc = pl_check_lengths(0, K)) return rc;
    if (K == 0) return IQA_OK;  // (nothing to read: no pointer is touched)
    if (!bits_dev || !kinds_dev || !info_dev || !rec_dev) return fail_inval("NULL device pointer");
    hipLaunchKernelGGL(k_dmr_decode, dim3(static_cast<unsigned>(K)), dim3(DM_THREADS), 0, as_stream(stream),
                       static_cast<const unsigned *>(bits_dev), static_cast<const unsigned char *>(kinds_dev), static_cast<unsigned *>(info_dev),
                       static_cast<int *>(rec_dev));
    return check_launch("k_dmr_decode");
}
