// stream_probe.hip -- what bounds the capture stream of the byte-plane ring kernels (channelize_ring.hip, ring_loader_split)?
// Replays the loader geometry of config 2 (D = 104, k_channelize_mfma_s16_ring_multi_half<7>) and nothing else: 256
// workgroups of twelve waves, each streaming ONE contiguous range of 705 tiles (13 312 bytes = 32 rows x 26 sixteen-byte
// units; 9 384 960 bytes per range, 2.4 GB in all).  Four loader waves (parity cp, half h) take the 1 KiB pieces 2 j + h of
// their parity's tile, hold two rounds of loads in registers, split every int16 into its high and its biased low byte
// (v_perm_b32 / v_xor) and write the two planes at the 16x16x64 kernels' pitch (224 bytes) into 66 560 bytes of LDS; one
// s_barrier per round; the eight multiplying waves only meet the barriers.
//
// Variants (template switches):
//   A  base: as shipped, 16-byte loads of a stream that starts 4 bytes behind a 16-byte boundary (phase 1 of 0..3 dwords)
//   B  phase: A with the stream at 0, 8 and 12 mod 16
//   C1 aligned loads, shift in registers: a lane loads the aligned unit at or below its bytes and takes the leading dwords
//      of the next unit from the lane above (v_mov_b32_dpp wave_shl:1); lane 63's come from ONE extra narrow load per round
//      (lane j of it fetches the head of the unit behind piece j, v_readlane_b32 hands it over as the DPP's old value)
//   C2 aligned loads, no cross-lane traffic: one aligned dwordx4 plus the next unit's leading dwords per lane
//   D  policy: A and C1 with nt loads
//   E  issue shape: E1 = all requests of a round in front of its plane writes, E2 = in two halves around them
//   F  DMA staging: the raw tile by global_load_lds_dwordx4 into a raw area of LDS (3 rounds x 2 tiles beside the planes),
//      the loaders split from there
//   G1 ceiling: all twelve waves load aligned vectors of one in-order sweep, no LDS
//   G2 order: A with the tiles dealt round-robin over the workgroups instead of as 256 ranges
//   R  the same with the multiplying waves' LDS reads beside the stream (AR against A; DR, ER against AR)
// `check` first: the planes C1, C2 and F leave (every workgroup's LDS, and a position-dependent checksum of every plane
// write of the whole run) must be byte for byte those of A at every phase, and A's must be the host's.
//
// Build: hipcc --offload-arch=gfx950 -O3 stream_probe.hip -o stream_probe
//   stream_probe [seconds per figure = 2] [pairs = 5] [row ...]: the check, then every variant against A in alternating pairs (ms per
//     launch by events over `seconds` of back-to-back launches, TB/s of the 2.4 GB, in-kernel clock = s_memtime ticks per
//     100 MHz s_memrealtime tick, median over the workgroups) and the gate: faster than A in every pair and a mean gain above
//     three times the larger spread of either side's figures
//     (`row`: only the rows whose names begin so)
//   stream_probe pmc: A, D, C1, F, G1, AR and DR three times each under their own kernel names, for a counters-only profiler run
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef v4i v4i_u __attribute__((aligned(4)));  // 16 bytes of the capture at a dword boundary
typedef int v2i __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_t;

constexpr int WGS = 256, TILES = 705, UPR = 26, Q = 32 * UPR, TILE_BYTES = 16 * Q, NP = 7, F = 2;
constexpr int PP = 224, SLOT = 64 * PP, PLANES = 4 * SLOT, LDS_A = PLANES + 9216;  // 66 560: planes + the window of sums
constexpr int RAW_OFF = LDS_A, LDS_F = LDS_A + 3 * 2 * TILE_BYTES;
constexpr long long STREAM_BYTES = static_cast<long long>(WGS) * TILES * TILE_BYTES;  // 2 402 549 760
constexpr int SLACK = 4096;
constexpr int SWEEP_ITERS = static_cast<int>(STREAM_BYTES / (WGS * 768 * 16));

struct Args {
    const char *buf;  // 16-byte aligned
    int tiles;        // per workgroup (TILES; the check runs fewer)
    unsigned long long *clk;
    int *sink;
    unsigned char *dump;        // CHECK: every workgroup's planes
    unsigned long long *hash;   // CHECK: one checksum per loader thread
};

__host__ __device__ inline unsigned fill_word(unsigned i)
{
    unsigned x = i * 2654435761u + 0x9E3779B9u;
    x ^= x >> 15;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    return x;
}

__global__ void k_fill(unsigned *w, long long n)
{
    for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n; i += static_cast<long long>(gridDim.x) * blockDim.x)
        w[i] = fill_word(static_cast<unsigned>(i));
}

template <bool NT>
__device__ __forceinline__ v4i load16(const char *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const v4i_u *>(p));
    else return *reinterpret_cast<const v4i_u *>(p);
}

template <bool NT>
__device__ __forceinline__ int load4(const char *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const int *>(p));
    else return *reinterpret_cast<const int *>(p);
}

// lane l <- lane l + 1; lane 63 keeps `old`
__device__ __forceinline__ int from_lane_above(int old, int v)
{
    return __builtin_amdgcn_update_dpp(old, v, 0x130, 0xf, 0xf, false);
}

// the stream's 16 bytes of a lane out of its aligned unit d and the head n of the next one, P dwords into the unit
template <int P>
__device__ __forceinline__ v4i shifted(v4i d, v4i n)
{
    if constexpr (P == 1) return v4i{d.y, d.z, d.w, n.x};
    else if constexpr (P == 2) return v4i{d.z, d.w, n.x, n.y};
    else if constexpr (P == 3) return v4i{d.w, n.x, n.y, n.z};
    else return d;
}

__device__ __forceinline__ void dma16(const void *src, lds_t *dst)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
#else
    (void)src;
    (void)dst;
#endif
}

// SHIFT 0: unaligned 16-byte loads (as shipped); 1: aligned + DPP (C1); 2: aligned + a narrow load per lane (C2); 3: LDS-DMA (F)
// READS: the eight multiplying waves also fetch their tile as ring_main_h16 does (per wave and tile twelve ds_read_b128, lane l
// at row l & 15, unit 4 chunk + (l >> 4), of either plane and data-row half, and the odd step's four ds_read_b64) -- the
// kernel's own "loads and LDS reads alone"
template <int P, int SHIFT, bool NT, int ISSUE, int ORDER, bool CHECK, bool READS = false>
__global__ __launch_bounds__(768, 3) void k_stream(Args a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool SH = (SHIFT == 1 || SHIFT == 2) && P > 0;  // (phase 0 needs no shift and pays for none)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, tiles = a.tiles, rounds = (tiles + 1) >> 1;
    if constexpr (CHECK) {
        for (int i = tid; i < LDS_A / 4; i += 768) reinterpret_cast<int *>(smem)[i] = 0;
    }
    __syncthreads();
    unsigned long long c0 = 0, r0 = 0;
    if (wave < 8) {
        if constexpr (READS) {
            const int cp = (wave >> 2) & 1, r16 = lane & 15, g = lane >> 4;
            const int lane_off = r16 * PP + 16 * g, at = r16 * PP + 32 * 6 + 8 * (g & 1), up = g >> 1;
            int odd[4] = {at + (up ? 0 : 32 * PP), at + 32 * PP + (up ? 0 : 16 * PP), at + (up ? 0 : 16 * PP), at + 16 * PP + (up ? 0 : 32 * PP)};
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(odd[i]));  // (plain ds_read_b64, not paired: as the kernel)
            v4i acc = {0, 0, 0, 0};
            for (int r = 0; r < rounds; ++r) {
                asm volatile("s_barrier" ::: "memory");
                const char *lb = smem + ((r & 1) * 2 + cp) * SLOT, *la = lb + lane_off;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) {
                        acc ^= *reinterpret_cast<const v4i *>(la + 16 * PP * bj + 64 * ch);
                        acc ^= *reinterpret_cast<const v4i *>(la + 32 * PP + 16 * PP * bj + 64 * ch);
                    }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const v2i d = *reinterpret_cast<const v2i *>(lb + odd[i]);
                    acc.x ^= d.x;
                    acc.y ^= d.y;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::"v"(acc) : "memory");  // (read before the barrier that frees the slot)
            }
            if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x5A17C0DE && a.sink != nullptr) a.sink[3] = acc.x;
        } else {
            for (int r = 0; r < rounds; ++r) asm volatile("s_barrier" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");
    } else {
        const int cp = (wave - 8) & 1, half = (wave - 8) >> 1;
        c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
        // the stream: byte 4 P of the buffer; aligned forms address the unit at or below
        const char *base = a.buf + (SH ? 0 : 4 * P);
        auto tile_ptr = [&](int round) {
            const int t = min(2 * round + cp, tiles - 1);
            return base + (ORDER ? static_cast<long long>(t) * WGS + b : static_cast<long long>(b) * tiles + t) * TILE_BYTES;
        };
        constexpr int QC = SH ? Q : Q - 1;  // unit the lanes behind the tile's last fetch: aligned, the one that holds its last 4 P bytes
        int doff[NP], soff[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int q = 64 * (2 * j + half) + lane, row = q / UPR, u = q - row * UPR;
            doff[j] = q < Q ? row * PP + 8 * u : -1;
            soff[j] = 16 * min(q, QC);
        }
        unsigned long long hash = 0;
        if constexpr (SHIFT == 3) {
            // ---- F: LDS-DMA into a raw area, split from there (every wave reads back only the pieces it fetched) ----
            // (pieces 2 j + half, j < 6, and piece 12 in the waves of half 0: a tile is exactly 13 pieces)
            auto request = [&](int round) {
                const char *src = tile_ptr(round) + 16 * lane + 1024 * half;
                char *raw = smem + RAW_OFF + ((round % 3) * 2 + cp) * TILE_BYTES + 1024 * half;
#pragma unroll
                for (int j = 0; j < 6; ++j) dma16(src + 2048 * j, (lds_t *)(raw + 2048 * j));
                if (half == 0) dma16(src + 2048 * 6, (lds_t *)(raw + 2048 * 6));
            };
            auto stage = [&](int round) {
                // this round's DMAs have landed once only the next round's (7 or 6) are outstanding
                if (round == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (half) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
                const char *raw = smem + RAW_OFF + ((round % 3) * 2 + cp) * TILE_BYTES + 16 * lane + 1024 * half;
                char *hi0 = smem + ((round & 1) * 2 + cp) * SLOT;
                v4i d[NP];
#pragma unroll
                for (int j = 0; j < 6; ++j) d[j] = *reinterpret_cast<const v4i *>(raw + 2048 * j);
                d[6] = *reinterpret_cast<const v4i *>(raw + (half ? 0 : 2048 * 6));  // (half 1: read, not written)
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    v2i hi, lo;
                    hi.x = __builtin_amdgcn_perm(d[j].y, d[j].x, 0x07050301);
                    hi.y = __builtin_amdgcn_perm(d[j].w, d[j].z, 0x07050301);
                    lo.x = __builtin_amdgcn_perm(d[j].y, d[j].x, 0x06040200) ^ 0x80808080;
                    lo.y = __builtin_amdgcn_perm(d[j].w, d[j].z, 0x06040200) ^ 0x80808080;
                    if (doff[j] >= 0) {
                        *reinterpret_cast<v2i *>(hi0 + doff[j]) = hi;
                        *reinterpret_cast<v2i *>(hi0 + 32 * PP + doff[j]) = lo;
                        if constexpr (CHECK)
                            hash += (static_cast<unsigned>(hi.x) * 3ull + static_cast<unsigned>(hi.y) * 5ull + static_cast<unsigned>(lo.x) * 7ull + static_cast<unsigned>(lo.y) * 11ull) *
                                    static_cast<unsigned long long>(doff[j] + 1 + 131 * round);
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the raw slot is refilled next)
            };
            request(0);
            stage(0);
            request(1);
            request(2);
            for (int r = 0; r < rounds; ++r) {
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (r + 1 < rounds) stage(r + 1);
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                request(r + 3);  // (beyond the last tile: the last tile again, never staged)
            }
        } else {
            // ---- register-staged loads ----
            int xoff = 0;
            if constexpr (SHIFT == 1 && SH) {
                const int jl = min(lane, NP - 1);
                xoff = 16 * min(64 * (2 * jl + half + 1), QC);
            }
            v4i buf[F][NP];
            int ext[F][3];         // C1: the head of the unit behind piece `lane` (lanes 0..NP-1)
            int nxt[F][NP][SH && SHIFT == 2 ? P : 1];  // C2: the head of the next unit, per lane and piece
            auto request = [&](int round, auto set, int j0, int j1) {
                constexpr int S = decltype(set)::value;
                const char *src = tile_ptr(round);
                if constexpr (SH && SHIFT == 1) {  // (in front of the pieces: loads return in order, the first piece's split needs it)
                    if (j0 == 0 && lane < NP) {
#pragma unroll
                        for (int k = 0; k < P; ++k) ext[S][k] = load4<NT>(src + xoff + 4 * k);
                    }
                }
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    if (j < j0 || j >= j1) continue;
                    buf[S][j] = load16<NT>(src + soff[j]);
                    if constexpr (SH && SHIFT == 2) {
                        const int no = min(soff[j] + 16, 16 * Q);
#pragma unroll
                        for (int k = 0; k < P; ++k) nxt[S][j][k] = load4<NT>(src + no + 4 * k);
                    }
                }
            };
            auto split = [&](auto set, int j, v2i &hi, v2i &lo) {
                constexpr int S = decltype(set)::value;
                v4i d = buf[S][j];
                if constexpr (SH) {
                    v4i n = {0, 0, 0, 0};
                    if constexpr (SHIFT == 1) {
                        if constexpr (P >= 1) n.x = from_lane_above(__builtin_amdgcn_readlane(ext[S][0], j), d.x);
                        if constexpr (P >= 2) n.y = from_lane_above(__builtin_amdgcn_readlane(ext[S][1], j), d.y);
                        if constexpr (P >= 3) n.z = from_lane_above(__builtin_amdgcn_readlane(ext[S][2], j), d.z);
                    } else {
                        if constexpr (P >= 1) n.x = nxt[S][j][0];
                        if constexpr (P >= 2) n.y = nxt[S][j][P >= 2 ? 1 : 0];
                        if constexpr (P >= 3) n.z = nxt[S][j][P >= 3 ? 2 : 0];
                    }
                    d = shifted<P>(d, n);
                }
                hi.x = __builtin_amdgcn_perm(d.y, d.x, 0x07050301);
                hi.y = __builtin_amdgcn_perm(d.w, d.z, 0x07050301);
                lo.x = __builtin_amdgcn_perm(d.y, d.x, 0x06040200) ^ 0x80808080;
                lo.y = __builtin_amdgcn_perm(d.w, d.z, 0x06040200) ^ 0x80808080;
            };
            auto put = [&](int round, int j, v2i hi, v2i lo) {
                char *hi0 = smem + ((round & 1) * 2 + cp) * SLOT;
                if (doff[j] >= 0) {
                    *reinterpret_cast<v2i *>(hi0 + doff[j]) = hi;
                    *reinterpret_cast<v2i *>(hi0 + 32 * PP + doff[j]) = lo;
                    if constexpr (CHECK)
                        hash += (static_cast<unsigned>(hi.x) * 3ull + static_cast<unsigned>(hi.y) * 5ull + static_cast<unsigned>(lo.x) * 7ull + static_cast<unsigned>(lo.y) * 11ull) *
                                static_cast<unsigned long long>(doff[j] + 1 + 131 * round);
                }
            };
            // stage the tile of `round` out of register set S, then request the tile of round `next` into it
            auto turn = [&](int round, int next, bool do_stage, bool do_request, auto set) {
                if constexpr (ISSUE == 0) {
                    if (do_stage) {
#pragma unroll
                        for (int j = 0; j < NP; ++j) {
                            v2i hi, lo;
                            split(set, j, hi, lo);
                            put(round, j, hi, lo);
                        }
                    }
                    if (do_request) request(next, set, 0, NP);
                } else {
                    v2i hi[NP], lo[NP];
#pragma unroll
                    for (int j = 0; j < NP; ++j) split(set, j, hi[j], lo[j]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (do_request) request(next, set, 0, ISSUE == 1 ? NP : 4);
                    __builtin_amdgcn_sched_barrier(0);
                    if (do_stage) {
#pragma unroll
                        for (int j = 0; j < NP; ++j) put(round, j, hi[j], lo[j]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (ISSUE == 2) {
                        if (do_request) request(next, set, 4, NP);
                    }
                }
            };
            using S0 = std::integral_constant<int, 0>;
            using S1 = std::integral_constant<int, 1>;
            request(0, S0{}, 0, NP);
            turn(0, 0, true, false, S0{});
            request(1, S1{}, 0, NP);
            request(2, S0{}, 0, NP);
            // round r stages the tile of round r + 1 (register set (r + 1) % 2) and requests that of round r + 3
            int r = 0;
            for (; r + 2 <= rounds; r += 2) {
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                turn(r + 1, r + 3, r + 1 < rounds, true, S1{});
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                turn(r + 2, r + 4, r + 2 < rounds, true, S0{});
            }
            if (r < rounds) {
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                turn(r + 1, r + 3, r + 1 < rounds, true, S1{});
            }
            // (the loads still in flight: keep them alive)
            int live = 0;
#pragma unroll
            for (int s = 0; s < F; ++s)
#pragma unroll
                for (int j = 0; j < NP; ++j) live ^= buf[s][j].x;
            if (live == 0x5A17C0DE && a.sink != nullptr) a.sink[0] = live;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if constexpr (CHECK) a.hash[b * 256 + (tid - 512)] = hash;
        if (wave == 8 && lane == 0) {
            a.clk[2 * b] = __builtin_amdgcn_s_memtime() - c0;
            a.clk[2 * b + 1] = __builtin_amdgcn_s_memrealtime() - r0;
        }
    }
    __syncthreads();
    if constexpr (CHECK) {
        for (int i = tid; i < PLANES / 4; i += 768) reinterpret_cast<int *>(a.dump)[b * (PLANES / 4) + i] = reinterpret_cast<const int *>(smem)[i];
    } else {
        const int v = reinterpret_cast<const int *>(smem)[tid];
        if (v == 0x5A17C0DE && a.sink != nullptr) a.sink[1] = v;
    }
}

// G1: the box's own read rate for this comparison -- twelve waves per workgroup, aligned 16-byte loads, the whole grid
// sweeping the buffer in order (iteration i: the 3 MiB behind the previous one), eight loads in flight per lane
template <bool NT>
__global__ __launch_bounds__(768, 3) void k_sweep(Args a)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    const char *p = a.buf + (static_cast<long long>(b) * 768 + tid) * 16;
    constexpr long long STEP = static_cast<long long>(WGS) * 768 * 16;
    v4i acc = {0, 0, 0, 0};
    int i = 0;
    for (; i + 8 <= SWEEP_ITERS; i += 8) {
        v4i d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = load16<NT>(p + (i + k) * STEP);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc ^= d[k];
    }
    for (; i < SWEEP_ITERS; ++i) acc ^= load16<NT>(p + i * STEP);
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x5A17C0DE && a.sink != nullptr) a.sink[2] = acc.x;
    if (tid == 0) {
        a.clk[2 * b] = __builtin_amdgcn_s_memtime() - c0;
        a.clk[2 * b + 1] = __builtin_amdgcn_s_memrealtime() - r0;
    }
}

typedef void (*kern_t)(Args);

struct Variant {
    const char *name;
    kern_t fn;
    size_t lds;
    double bytes;
};

struct Figure {
    double ms, ghz;
};

static Figure run(const Variant &v, Args a, double seconds)
{
    hipFuncSetAttribute(reinterpret_cast<const void *>(v.fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    constexpr int BATCH = 8;
    double total_ms = 0, sum_ms = 0;
    int batches = 0;
    float ms = 0;
    bool first = true;
    while (total_ms < seconds * 1e3) {
        hipEventRecord(e0);
        for (int i = 0; i < BATCH; ++i) hipLaunchKernelGGL(v.fn, dim3(WGS), dim3(768), v.lds, 0, a);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) {
            printf("launch of %s failed: %s\n", v.name, hipGetErrorString(hipGetLastError()));
            exit(1);
        }
        hipEventElapsedTime(&ms, e0, e1);
        total_ms += ms;
        if (!first) sum_ms += ms, ++batches;  // (the first batch warms up)
        first = false;
    }
    std::vector<unsigned long long> h(2 * WGS);
    hipMemcpy(h.data(), a.clk, h.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> ghz(WGS);
    for (int i = 0; i < WGS; ++i) ghz[i] = h[2 * i + 1] ? double(h[2 * i]) / double(h[2 * i + 1]) * 0.1 : 0.0;
    std::sort(ghz.begin(), ghz.end());
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return Figure{batches ? sum_ms / (double(BATCH) * batches) : ms / BATCH, ghz[WGS / 2]};
}

// the planes every workgroup is left with and the checksums of all its plane writes
static void run_check(kern_t fn, size_t lds, Args a, int tiles, std::vector<unsigned char> &dump, std::vector<unsigned long long> &hash)
{
    hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    a.tiles = tiles;
    hipMemset(a.dump, 0xEE, static_cast<size_t>(WGS) * PLANES);
    hipMemset(a.hash, 0, WGS * 256 * 8);
    hipLaunchKernelGGL(fn, dim3(WGS), dim3(768), lds, 0, a);
    if (hipDeviceSynchronize() != hipSuccess) {
        printf("check launch failed: %s\n", hipGetErrorString(hipGetLastError()));
        exit(1);
    }
    dump.resize(static_cast<size_t>(WGS) * PLANES);
    hash.resize(WGS * 256);
    hipMemcpy(dump.data(), a.dump, dump.size(), hipMemcpyDeviceToHost);
    hipMemcpy(hash.data(), a.hash, hash.size() * 8, hipMemcpyDeviceToHost);
}

// the planes of workgroup b after a run of `tiles` tiles at phase p, computed on the host
static void host_planes(int b, int tiles, int p, std::vector<unsigned char> &out)
{
    out.assign(PLANES, 0);
    const int rounds = (tiles + 1) >> 1;
    for (int slot = 0; slot < 2; ++slot)
        for (int cp = 0; cp < 2; ++cp) {
            int rr = rounds - 1;
            if ((rr & 1) != slot) --rr;
            if (rr < 0) continue;
            const int t = std::min(2 * rr + cp, tiles - 1);
            const long long start = 4ll * p + (static_cast<long long>(b) * tiles + t) * TILE_BYTES;
            unsigned char *hi0 = out.data() + (slot * 2 + cp) * SLOT;
            for (int row = 0; row < 32; ++row)
                for (int k = 0; k < 8 * UPR; ++k) {
                    const long long byte = start + row * 16ll * UPR + 2 * k;  // int16 k of the row
                    const unsigned w = fill_word(static_cast<unsigned>(byte >> 2));
                    const unsigned short s = static_cast<unsigned short>(w >> (8 * (byte & 3)));
                    hi0[row * PP + k] = static_cast<unsigned char>(s >> 8);
                    hi0[32 * PP + row * PP + k] = static_cast<unsigned char>(s & 0xFF) ^ 0x80;
                }
        }
}

template <int P>
static int check_phase(Args a)
{
    int bad = 0;
    for (int tiles : {9, 12}) {  // an odd count (the clamped last tile) and an even one: either slot holds a last tile
        std::vector<unsigned char> da, dc;
        std::vector<unsigned long long> ha, hc;
        run_check(k_stream<P, 0, false, 0, 0, true>, LDS_A, a, tiles, da, ha);
        std::vector<unsigned char> hp;
        long long host_diff = 0;
        for (int b : {0, 1, 100, 255}) {
            host_planes(b, tiles, P, hp);
            for (int i = 0; i < PLANES; ++i) host_diff += hp[i] != da[static_cast<size_t>(b) * PLANES + i];
        }
        printf("check phase %d, %2d tiles: A against the host's planes (workgroups 0, 1, 100, 255): %lld bytes differ\n", P, tiles, host_diff);
        bad += host_diff != 0;
        auto cmp = [&](const char *name, kern_t fn, size_t lds) {
            run_check(fn, lds, a, tiles, dc, hc);
            long long d = 0, h = 0;
            for (size_t i = 0; i < da.size(); ++i) d += da[i] != dc[i];
            for (size_t i = 0; i < ha.size(); ++i) h += ha[i] != hc[i];
            printf("check phase %d, %2d tiles: %-3s against A: %lld of %zu plane bytes differ, %lld of %zu write checksums differ\n", P, tiles, name, d, da.size(), h, ha.size());
            bad += d != 0 || h != 0;
        };
        cmp("C1", k_stream<P, 1, false, 0, 0, true>, LDS_A);
        cmp("C2", k_stream<P, 2, false, 0, 0, true>, LDS_A);
        cmp("C1n", k_stream<P, 1, true, 0, 0, true>, LDS_A);
        cmp("E1", k_stream<P, 0, false, 1, 0, true>, LDS_A);
        cmp("E2", k_stream<P, 0, false, 2, 0, true>, LDS_A);
        cmp("CE1", k_stream<P, 1, false, 1, 0, true>, LDS_A);
        cmp("F", k_stream<P, 3, false, 0, 0, true>, LDS_F);
    }
    return bad;
}

int main(int argc, char **argv)
{
    const bool pmc = argc > 1 && std::string(argv[1]) == "pmc";
    const double seconds = !pmc && argc > 1 ? atof(argv[1]) : 2.0;
    const int pairs = !pmc && argc > 2 ? atoi(argv[2]) : 5;
    char *buf;
    Args a{};
    if (hipMalloc(&buf, STREAM_BYTES + SLACK) != hipSuccess) {
        printf("cannot allocate %lld bytes\n", STREAM_BYTES + SLACK);
        return 1;
    }
    hipMalloc(&a.clk, 2 * WGS * 8);
    hipMalloc(&a.sink, 64);
    hipMalloc(&a.dump, static_cast<size_t>(WGS) * PLANES);
    hipMalloc(&a.hash, WGS * 256 * 8);
    hipMemset(a.clk, 0, 2 * WGS * 8);
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, reinterpret_cast<unsigned *>(buf), (STREAM_BYTES + SLACK) / 4);
    hipDeviceSynchronize();
    a.buf = buf;
    a.tiles = TILES;

    const Variant A{"A   base, stream at 4 mod 16", k_stream<1, 0, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)};
    const Variant C1{"C1  aligned + DPP shift, 4 mod 16", k_stream<1, 1, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)};
    const Variant D{"D   A with nt loads", k_stream<1, 0, true, 0, 0, false>, LDS_A, double(STREAM_BYTES)};
    const Variant Fv{"F   LDS-DMA staging, 4 mod 16", k_stream<1, 3, false, 0, 0, false>, LDS_F, double(STREAM_BYTES)};
    const Variant G1{"G1  in-order sweep, 12 waves, no LDS", k_sweep<false>, 0, double(SWEEP_ITERS) * WGS * 768 * 16};
    if (pmc) {
        const Variant AR{"AR", k_stream<1, 0, false, 0, 0, false, true>, LDS_A, double(STREAM_BYTES)};
        const Variant DR{"DR", k_stream<1, 0, true, 0, 0, false, true>, LDS_A, double(STREAM_BYTES)};
        for (const Variant *v : {&A, &D, &C1, &Fv, &G1, &AR, &DR}) {
            hipFuncSetAttribute(reinterpret_cast<const void *>(v->fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(v->fn, dim3(WGS), dim3(768), v->lds, 0, a);
            if (hipDeviceSynchronize() != hipSuccess) return 1;
        }
        return 0;
    }

    int bad = check_phase<0>(a) + check_phase<1>(a) + check_phase<2>(a) + check_phase<3>(a);
    printf("check: %s\n\n", bad ? "FAILED" : "every variant writes A's planes at every phase");
    if (bad) return 1;
    a.tiles = TILES;

    const Variant AR{"AR  A, the multiplying waves read their tiles", k_stream<1, 0, false, 0, 0, false, true>, LDS_A, double(STREAM_BYTES)};
    struct Row {
        Variant base, v;
    };
    const std::vector<Row> rows = {
        {A, {"B0  A at 0 mod 16", k_stream<0, 0, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"B2  A at 8 mod 16", k_stream<2, 0, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"B3  A at 12 mod 16", k_stream<3, 0, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, C1},
        {A, {"C2  aligned + dword per lane, 4 mod 16", k_stream<1, 2, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"C1b aligned + DPP shift, 8 mod 16", k_stream<2, 1, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"C1c aligned + DPP shift, 12 mod 16", k_stream<3, 1, false, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, D},
        {A, {"DC  C1 with nt loads", k_stream<1, 1, true, 0, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"E1  A, requests before the plane writes", k_stream<1, 0, false, 1, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"E2  A, requests in halves around them", k_stream<1, 0, false, 2, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"CE1 C1, requests before the plane writes", k_stream<1, 1, false, 1, 0, false>, LDS_A, double(STREAM_BYTES)}},
        {A, Fv},
        {A, G1},
        {A, {"G1n in-order sweep, nt loads", k_sweep<true>, 0, double(SWEEP_ITERS) * WGS * 768 * 16}},
        {A, {"G2  A, tiles dealt round-robin", k_stream<1, 0, false, 0, 1, false>, LDS_A, double(STREAM_BYTES)}},
        {A, {"G2n A, round-robin tiles, nt loads", k_stream<1, 0, true, 0, 1, false>, LDS_A, double(STREAM_BYTES)}},
        {A, AR},
        {AR, {"DR  AR with nt loads", k_stream<1, 0, true, 0, 0, false, true>, LDS_A, double(STREAM_BYTES)}},
        {AR, {"ER  AR, requests in halves around the writes", k_stream<1, 0, false, 2, 0, false, true>, LDS_A, double(STREAM_BYTES)}},
    };
    printf("%.1f s of back-to-back launches per figure, %d alternating pairs against the base (A; the R rows: AR); TB/s of %.4f GB (the sweeps: of their own %.4f GB)\n\n",
           seconds, pairs, STREAM_BYTES * 1e-9, G1.bytes * 1e-9);
    for (const Row &row : rows) {
        const Variant &v = row.v, &base = row.base;
        bool wanted = argc <= 3;
        for (int i = 3; i < argc; ++i) wanted = wanted || strncmp(v.name, argv[i], strlen(argv[i])) == 0;
        if (!wanted) continue;
        std::vector<double> ta, tv;
        double ga = 0, gv = 0;
        for (int p = 0; p < pairs; ++p) {
            const Figure fa = run(base, a, seconds), fv = run(v, a, seconds);
            ta.push_back(fa.ms);
            tv.push_back(fv.ms);
            ga += fa.ghz / pairs;
            gv += fv.ghz / pairs;
        }
        double ma = 0, mv = 0;
        bool every = true;
        printf("%-46s pairs (base, variant) ms:", v.name);
        for (int p = 0; p < pairs; ++p) {
            ma += ta[p] / pairs, mv += tv[p] / pairs;
            every = every && tv[p] < ta[p];
            printf(" (%.4f, %.4f)", ta[p], tv[p]);
        }
        const double sa = *std::max_element(ta.begin(), ta.end()) - *std::min_element(ta.begin(), ta.end());
        const double sv = *std::max_element(tv.begin(), tv.end()) - *std::min_element(tv.begin(), tv.end());
        const double gain = ma - mv, spread = std::max(sa, sv);
        printf("\n    base %.4f ms %.3f TB/s %.3f GHz | variant %.4f ms %.3f TB/s %.3f GHz | gain %+.4f ms (%+.2f %%), spreads %.4f / %.4f, gate %s\n", ma,
               base.bytes / ma * 1e-9, ga, mv, v.bytes / mv * 1e-9, gv, gain, 100.0 * gain / ma, sa, sv,
               every && gain > 3.0 * spread ? "PASSED" : (every ? "faster in every pair, gain within 3 x spread" : "not passed"));
        fflush(stdout);
    }
    return 0;
}
