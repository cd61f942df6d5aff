// kstep_probe.hip -- how busy can the matrix pipe get with the ring kernel's k-step body, two waves per SIMD?
// Isolates the steady state of channelize_ring.hip's inner loop from its round structure (barriers, DMA, scatter):
//   mode 0: 3 x v_mfma_i32_32x32x32_i8 per step, operands constant                       (the pipe's own rate)
//   mode 1: + the byte split (8 v_perm_b32 + 4 v_xor) of a data fragment held in registers
//   mode 2: + the two ds_read_b128 per step from an LDS tile at the padded row pitch (prefetched two steps ahead)
//   mode 3: mode 2 with a workgroup barrier every KS steps (one "tile") -- the round structure without DMA and scatter
//   mode 4: mode 3 + the scatter (16 ds_add_u32 of 256*acc1 + acc2 per tile)
// 256 workgroups x 8 waves (two per SIMD), tap fragments in registers as in the kernel.  Prints MFMAs per SIMD-cycle
// against the pipe's 1 / 32.   Build: hipcc --offload-arch=gfx950 -O3 kstep_probe.hip -o kstep_probe
//   kstep_probe shape [seconds] [pairs]: the 32x32x32 tile body against the 16x16x64 one at the same tile per wave (wall
//     time, in-kernel clock, equal sums) and the bare issue rates of the four int8 forms -- see k_probe_shape
//   kstep_probe fold [seconds] [pairs]: the 16x16x64 body against the same with its odd last k step folded along K
//   kstep_probe zedge [seconds] [pairs]: the folded body against the same with the all-zero high tap bytes of a Kaiser
//     filter's edge rows skipped (light and heavy waves paired per SIMD), and against the pairing alone -- see sh_zedge_wave
//   kstep_probe lds: the LDS access patterns of the bodies, one kernel each, for a counters-only profiler run
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int KS = 13;
constexpr int PITCH = (4 * KS + 1) * 16;  // bytes: 52 units of data + 1 of padding (D = 208)

template <int MODE, int VAR = 0>
__global__ __launch_bounds__(512, 2) void k_probe(const v4i *taps, int *sink, int tiles, unsigned long long *cycles)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    v4i fq[KS][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        fq[ks][0] = taps[(ks * 2 + 0) * 64 + lane];
        fq[ks][1] = taps[(ks * 2 + 1) * 64 + lane];
    }
    for (int i = tid; i < 32 * PITCH / 4 + 1024; i += 512) reinterpret_cast<int *>(smem)[i] = i * 2654435761u;
    int *s_acc = reinterpret_cast<int *>(smem + 32 * PITCH + 1024);
    for (int i = tid; i < 1152; i += 512) s_acc[i] = 0;
    __syncthreads();
    const char *la = smem + (lane & 31) * PITCH + 32 * (lane >> 5);
    const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v16i acc1 = zero16, acc2 = zero16;
    v4i d0 = taps[lane], d1 = taps[64 + lane];
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int t = 0; t < tiles; ++t) {
        if (MODE >= 3) asm volatile("s_barrier" ::: "memory");
        v4i dd[KS][2];
        constexpr int PD = (VAR & 1) ? 4 : 2;
        auto rd = [&](int ks) {
            if constexpr (VAR & 16) {
                typedef int v2i __attribute__((ext_vector_type(2)));
                const v2i a0 = *reinterpret_cast<const v2i *>(la + 64 * ks), a1 = *reinterpret_cast<const v2i *>(la + 64 * ks + 8);
                const v2i b0 = *reinterpret_cast<const v2i *>(la + 64 * ks + 16), b1 = *reinterpret_cast<const v2i *>(la + 64 * ks + 24);
                dd[ks][0] = v4i{a0.x, a0.y, a1.x, a1.y};
                dd[ks][1] = v4i{b0.x, b0.y, b1.x, b1.y};
            } else {
                dd[ks][0] = *reinterpret_cast<const v4i *>(la + 64 * ks);
                dd[ks][1] = (VAR & 8) ? dd[ks][0] : *reinterpret_cast<const v4i *>(la + 64 * ks + 16);
            }
        };
        if (MODE >= 2) {
#pragma unroll
            for (int ks = 0; ks < PD; ++ks) rd(ks);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            v4i hi = d0, lo = d1;
            if (MODE >= 1) {
                const v4i e0 = (MODE >= 2) ? dd[ks][0] : d0, e1 = (MODE >= 2) ? dd[ks][1] : d1;
                hi.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x07050301);
                hi.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x07050301);
                hi.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x07050301);
                hi.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x07050301);
                lo.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x06040200) ^ 0x80808080;
                lo.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x06040200) ^ 0x80808080;
                lo.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x06040200) ^ 0x80808080;
                lo.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x06040200) ^ 0x80808080;
            }
            if (MODE >= 2 && !(VAR & 2) && ks + PD < KS) rd(ks + PD);
            acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], hi, (MODE >= 3 && ks == 0) ? zero16 : acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], lo, (MODE >= 3 && ks == 0) ? zero16 : acc2, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][1], hi, acc2, 0, 0, 0);
            if (MODE >= 2 && (VAR & 2) && ks + PD < KS) rd(ks + PD);
            if (!(VAR & 4)) __builtin_amdgcn_sched_barrier(0);
        }
        if (MODE >= 4) {
            const unsigned p = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(
                s_acc + ((t * 32 + (lane & 31) + 4 * (lane >> 5) + 1) & 511) + (wave & 1) * 32)));
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int comb = (acc1[q] << 8) + acc2[q];
                asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(4 * ((q & 3) + 8 * (q >> 2))));
            }
        } else if (MODE >= 3) {
            asm volatile("" ::"v"(acc1), "v"(acc2));
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    int s = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += acc1[q] + acc2[q];
    if (s == 0x12345678) sink[0] = s;  // keep the accumulators alive
    if (tid == 0) cycles[blockIdx.x] = t1 - t0;
}

template <int MODE, int VAR = 0>
static void run(const v4i *taps, int *sink, unsigned long long *cyc, int tiles)
{
    const size_t lds = 32 * PITCH + 1024 + 1152 * 4 + 4096;
    hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe<MODE, VAR>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_probe<MODE, VAR>), dim3(256), dim3(512), lds, 0, taps, sink, tiles, cyc);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
    }
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h(256);
    hipMemcpy(h.data(), cyc, 256 * 8, hipMemcpyDeviceToHost);
    // 2 waves per SIMD, each 3*KS MFMAs per tile
    const double mfma_per_simd = 2.0 * 3 * KS * tiles;
    const double us = ms * 1e3;
    printf("mode %d var %2d: %8.3f ms for %d tiles per wave; %.1f ns per tile-pair per SIMD; at 32 cycles per MFMA the pipe alone needs %.0f cycles per "
           "tile-pair -> busy %.1f %% if the clock were 2.0 GHz, %.1f %% at 2.4 GHz (s_memtime ticks per block: %llu)\n",
           MODE, VAR, ms, tiles, us * 1e3 / tiles, 2.0 * 3 * KS * 32, 100.0 * mfma_per_simd * 32 / (us * 2000.0), 100.0 * mfma_per_simd * 32 / (us * 2400.0),
           h[0]);
}


// ---- more tap rows per wave: RT row tiles (32 rows each) share every data fragment a wave reads and splits ----------
// WAVES = 8: two waves per SIMD (<= 256 registers each); WAVES = 4: one wave per SIMD (<= 512).
// SYNC = 1: the round structure -- a workgroup barrier in front of every tile and the scatter of the tile's sums (16
// ds_add_u32 per row tile) behind it.  BLK workgroups per CU: BLK = 2 with WAVES = 4 puts two INDEPENDENT barrier domains
// on a CU (each SIMD holds one wave of either), against one domain of 8 waves.
template <int KSX, int RT, int WAVES, int SYNC = 0, int BLK = 1>
__global__ __launch_bounds__(WAVES * 64, BLK) void k_probe_rt(const v4i *taps, int *sink, int tiles, unsigned long long *clk)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PITCHX = (4 * KSX + 1) * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    v4i fq[KSX][RT][2];
#pragma unroll
    for (int ks = 0; ks < KSX; ++ks)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            fq[ks][rt][0] = taps[((ks * 2 + 0) * 2 + rt) * 64 + lane];
            fq[ks][rt][1] = taps[((ks * 2 + 1) * 2 + rt) * 64 + lane];
        }
    for (int i = tid; i < 32 * PITCHX / 4 + 1024; i += WAVES * 64) reinterpret_cast<int *>(smem)[i] = i * 2654435761u;
    __syncthreads();
    const char *la = smem + (lane & 31) * PITCHX + 32 * (lane >> 5);
    const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v16i acc1[RT], acc2[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc1[rt] = acc2[rt] = zero16;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    int *s_win = reinterpret_cast<int *>(smem + 32 * PITCHX + 1024);
    const unsigned win_at = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(s_win + (lane & 31) + 4 * (lane >> 5))));
    if (SYNC == 2 && (blockIdx.x & 256)) {  // the second workgroup of a CU starts half a tile late: out of phase for good
        for (int ks = 0; ks < (KSX * RT * 3) / 2; ++ks) acc1[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[0][0][0], fq[0][0][1], acc1[0], 0, 0, 0);
    }
    for (int t = 0; t < tiles; ++t) {
        if (SYNC) asm volatile("s_barrier" ::: "memory");
        v4i dd[KSX][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            dd[ks][0] = *reinterpret_cast<const v4i *>(la + 64 * ks);
            dd[ks][1] = *reinterpret_cast<const v4i *>(la + 64 * ks + 16);
        }
#pragma unroll
        for (int ks = 0; ks < KSX; ++ks) {
            const v4i e0 = dd[ks][0], e1 = dd[ks][1];
            v4i hi, lo;
            hi.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x07050301);
            hi.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x07050301);
            hi.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x07050301);
            hi.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x07050301);
            lo.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x06040200) ^ 0x80808080;
            lo.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x06040200) ^ 0x80808080;
            lo.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x06040200) ^ 0x80808080;
            lo.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x06040200) ^ 0x80808080;
            if (ks + 2 < KSX) {
                dd[ks + 2][0] = *reinterpret_cast<const v4i *>(la + 64 * (ks + 2));
                dd[ks + 2][1] = *reinterpret_cast<const v4i *>(la + 64 * (ks + 2) + 16);
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                acc1[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][rt][0], hi, acc1[rt], 0, 0, 0);
                acc2[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][rt][0], lo, acc2[rt], 0, 0, 0);
                acc2[rt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][rt][1], hi, acc2[rt], 0, 0, 0);
            }
        }
        if (SYNC) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int comb = (acc1[rt][q] << 8) + acc2[rt][q];
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(win_at), "v"(comb), "n"(4 * ((q & 3) + 8 * (q >> 2)) + 1024 * (rt & 1)));
                }
                acc1[rt] = acc2[rt] = zero16;
            }
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    int s = 0;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int q = 0; q < 16; ++q) s += acc1[rt][q] + acc2[rt][q];
    if (s == 0x12345678) sink[0] = s;
    if (tid == 0 && blockIdx.x == 100) {
        clk[0] = c1 - c0;
        clk[1] = r1 - r0;
    }
}

// ---- the round structure without its bubble ----------------------------------------------------------------------
// One barrier per tile as before, but in the MIDDLE of the tile (it announces the NEXT tile's data and releases the one
// before this one), the fragment prefetch running on across the tile boundary, and two sets of sums: the finished tile's
// 16 adds go out one per k step between the next tile's MFMAs instead of draining the pipe in front of a barrier.
template <int KSX, int WAVES, int OFF = 0>  // OFF bits: 1 no barrier, 2 no scatter, 4 scatter by plain stores, 8 prefetch within the tile only
__global__ __launch_bounds__(WAVES * 64, 1) void k_probe_cont(const v4i *taps, int *sink, int tiles, unsigned long long *clk)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int PITCHX = (4 * KSX + 1) * 16;
    const int tid = threadIdx.x, lane = tid & 63;
    v4i fq[KSX][2];
#pragma unroll
    for (int ks = 0; ks < KSX; ++ks) {
        fq[ks][0] = taps[((ks * 2 + 0) * 2) * 64 + lane];
        fq[ks][1] = taps[((ks * 2 + 1) * 2) * 64 + lane];
    }
    for (int i = tid; i < 32 * PITCHX / 4 + 1024; i += WAVES * 64) reinterpret_cast<int *>(smem)[i] = i * 2654435761u;
    __syncthreads();
    const char *la = smem + (lane & 31) * PITCHX + 32 * (lane >> 5);
    int *s_win = reinterpret_cast<int *>(smem + 32 * PITCHX + 1024);
    const unsigned win_at = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(s_win + (lane & 31) + 4 * (lane >> 5))));
    const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v16i a1[2] = {zero16, zero16}, a2[2] = {zero16, zero16};
    v4i dd[KSX + 2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        dd[ks][0] = *reinterpret_cast<const v4i *>(la + 64 * ks);
        dd[ks][1] = *reinterpret_cast<const v4i *>(la + 64 * ks + 16);
    }
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    auto tile = [&](auto cur_c, bool have_prev) {
        constexpr int CUR = decltype(cur_c)::value, PRV = 1 - CUR;
#pragma unroll
        for (int ks = 0; ks < KSX; ++ks) {
            if (ks == KSX / 2 && !(OFF & 1)) asm volatile("s_barrier" ::: "memory");
            const v4i e0 = dd[ks][0], e1 = dd[ks][1];
            v4i hi, lo;
            hi.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x07050301);
            hi.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x07050301);
            hi.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x07050301);
            hi.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x07050301);
            lo.x = __builtin_amdgcn_perm(e0.y, e0.x, 0x06040200) ^ 0x80808080;
            lo.y = __builtin_amdgcn_perm(e0.w, e0.z, 0x06040200) ^ 0x80808080;
            lo.z = __builtin_amdgcn_perm(e1.y, e1.x, 0x06040200) ^ 0x80808080;
            lo.w = __builtin_amdgcn_perm(e1.w, e1.z, 0x06040200) ^ 0x80808080;
            {  // two steps ahead, across the tile boundary (the barrier of this tile has announced the next one)
                const int nk = (ks + 2) % KSX;
                dd[ks + 2][0] = *reinterpret_cast<const v4i *>(la + 64 * nk);
                dd[ks + 2][1] = *reinterpret_cast<const v4i *>(la + 64 * nk + 16);
            }
            a1[CUR] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], hi, a1[CUR], 0, 0, 0);
            a2[CUR] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], lo, a2[CUR], 0, 0, 0);
            a2[CUR] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][1], hi, a2[CUR], 0, 0, 0);
            // the previous tile's sums leave between this tile's MFMAs: ceil(16 / KSX) adds per k step
            constexpr int PER = (16 + KSX - 1) / KSX;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int q = ks * PER + j;
                if (q < 16 && have_prev && !(OFF & 2)) {
                    const int comb = (a1[PRV][q] << 8) + a2[PRV][q];
                    if (OFF & 4) asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(win_at), "v"(comb), "n"(4 * ((q & 3) + 8 * (q >> 2))));
                    else asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(win_at), "v"(comb), "n"(4 * ((q & 3) + 8 * (q >> 2))));
                }
            }
        }
        // hand the two prefetched fragments to the next tile's steps 0 and 1, and clear the set the next-but-one tile sums into
        dd[0][0] = dd[KSX][0], dd[0][1] = dd[KSX][1], dd[1][0] = dd[KSX + 1][0], dd[1][1] = dd[KSX + 1][1];
        a1[PRV] = zero16, a2[PRV] = zero16;
    };
    for (int t = 0; t < tiles; t += 2) {
        tile(std::integral_constant<int, 0>{}, t > 0);
        tile(std::integral_constant<int, 1>{}, true);
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    int sacc = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc += a1[0][q] + a2[0][q] + a1[1][q] + a2[1][q];
    if (sacc == 0x12345678) sink[0] = sacc;
    if (tid == 0 && blockIdx.x == 100) {
        clk[0] = c1 - c0;
        clk[1] = r1 - r0;
    }
}

template <int KSX, int WAVES, int OFF = 0>
static void run_cont(const v4i *taps, int *sink, int tiles, unsigned long long *clk)
{
    const size_t lds = 32 * ((4 * KSX + 1) * 16) + 4096 + 1024;
    hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe_cont<KSX, WAVES, OFF>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_probe_cont<KSX, WAVES, OFF>), dim3(256), dim3(WAVES * 64), lds, 0, taps, sink, tiles, clk);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
    }
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    const double mfma_per_simd = (WAVES / 4.0) * 3 * KSX * tiles;
    unsigned long long h[2];
    hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
    const double ghz = double(h[0]) / double(h[1]) * 0.1;
    printf("k steps %2d, %d wave(s) per SIMD, mid-tile barrier + prefetch across tiles + interleaved scatter (off bits %d): %8.3f ms; in-kernel clock %.3f GHz -> "
           "matrix pipe busy %.1f %%; %.1f ns per 128 tap rows x 32 data rows per CU\n",
           KSX, WAVES / 4, OFF, ms, ghz, 100.0 * mfma_per_simd * 32 / (ms * 1e6 * ghz), ms * 1e6 / tiles / (WAVES / 4.0));
}

template <int KSX, int RT, int WAVES, int SYNC = 0, int BLK = 1>
static void run_rt(const v4i *taps, int *sink, int tiles, unsigned long long *clk)
{
    const size_t lds = 32 * ((4 * KSX + 1) * 16) + 4096 + 1024;
    hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe_rt<KSX, RT, WAVES, SYNC, BLK>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int rep = 0; rep < 3; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL((k_probe_rt<KSX, RT, WAVES, SYNC, BLK>), dim3(256 * BLK), dim3(WAVES * 64), lds, 0, taps, sink, tiles, clk);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
    }
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    const double mfma_per_simd = BLK * (WAVES / 4.0) * 3 * KSX * RT * tiles;
    unsigned long long h[2];
    hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
    const double ghz = double(h[0]) / double(h[1]) * 0.1;  // in-kernel clock: s_memtime ticks per 100 MHz s_memrealtime tick
    printf("k steps %2d, %d row tile(s) per wave, %d workgroup(s) per CU x %d wave(s) per SIMD%s: %8.3f ms; in-kernel clock %.3f GHz -> matrix pipe busy %.1f %%; "
           "%.1f ns per 128 tap rows x 32 data rows per CU\n",
           KSX, RT, BLK, WAVES / 4, SYNC == 2 ? ", barrier + scatter per tile, second workgroup half a tile late" : SYNC ? ", barrier + scatter per tile" : "", ms, ghz, 100.0 * mfma_per_simd * 32 / (ms * 1e6 * ghz),
           ms * 1e6 / tiles / (BLK * WAVES * RT / 4.0));
}

// ---- the MFMA shape at the same tile per wave: 32 tap rows x 32 data rows, byte planes, 7 k steps, half last step ----
// BODY 0: six v_mfma_i32_32x32x32_i8 steps and one 32x32x16 (plane pitch 15 sixteen-byte units), lane = data row.
// BODY 1: three v_mfma_i32_16x16x64_i8 chunks and one 16x16x32 for the odd last k step (plane pitch 14 units); the two
//         off-diagonal 16x16 blocks of the tile land on the same output positions and share one accumulator.
// BODY 2: BODY 1 with the odd step's twelve 16x16x32, each half against zero taps, folded along K into seven: products
//         that add into the same accumulator are concatenated, 43 matrix instructions per tile instead of 48 (`fold`).
// All read the same logical tile (random bytes) and the same tap fragments (the library's afrag layout, random, zero
// beyond value 208 as the planner pads them); the windows of sums they leave must be equal -- that also checks the tap
// gather and the lane maps.  Twelve waves as in the kernel: eight multiply (two per SIMD), four only join the barriers
// (the loader waves' place).  In-kernel clock: s_memtime ticks per 100 MHz s_memrealtime tick (diagnostic, this probe only).
constexpr int SH_KS = 7, SH_AS = 576;
template <int BODY>
struct ShapeGeo {
    static constexpr int PP = BODY ? 32 * SH_KS : 32 * SH_KS + 16;  // bytes per row of a plane
    static constexpr int SLOT = 64 * PP;
    static constexpr int LDS = 2 * SLOT + 2 * SH_AS * 4;
};

__device__ __forceinline__ unsigned sh_hash(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// ---- `zedge`: BODY 2 with the all-zero high tap bytes of a Kaiser filter's edge rows skipped --------------------------
// The first and last tap rows of a Kaiser design are tiny: with T = 256 q1 + q2 their q1 is zero, and of a row's three
// products only q2 * hi is left.  Config 2's plan has 22 such rows per component, cyclically contiguous (q - 1 = 52..63,
// 0..9); rotated by `rot` = 12 slots (slot s of a component holds tap row (s - rot) mod 64) the first 16-row block of either
// component is free of q1.  A wave of even rt (LIGHT) then runs, per 64-value chunk,
//         Z[bj] = q2_0 . hi_bj                          (block 0: the zero-q1 rows, S2 alone, no S1)
//         S1[bj] = q1_1 . hi_bj      S2[bj] = q1_1 . lo_bj + q2_1 . hi_bj      (block 1, as before)
// eight instructions instead of twelve, and on the folded odd step six instead of seven, from two of the four 8-byte reads:
//         Z[bj] = [0 | q2_0] . [lo_bj ; hi_bj]    S1[bj] = [0 | q1_1] . [lo_bj ; hi_bj]    S2[bj] = [q1_1 | q2_1] . [lo_bj ; hi_bj]
// 30 matrix instructions per tile against 43.  Block 0's rows are two runs (the filter's last rows, then its first), so
// its scatter base differs per lane group (rot a multiple of 4, at most 16) and it shares no positions with block 1: 16
// adds per tile for a light wave, 12 for a heavy one (odd rt: BODY 2's tile, its rows moved by the rotation).
// PAIRING: the waves of parity 1 take rt ^ 1, so that every SIMD (wave index mod 4, read back from HW_ID below) hosts one
// light and one heavy wave.  BODY 3: both; BODY 4: the pairing alone, every wave heavy, rot = 0.
template <bool LIGHT>
__device__ __forceinline__ void sh_zedge_wave(const v4i *afrag, const char *slot, int *s_acc, int rt, int cp, int lane, int tiles, int rot,
                                              unsigned long long (&clk)[4])
{
    constexpr int KS = SH_KS, NC = KS / 2, PP = 32 * SH_KS;
    const int r16 = lane & 15, g = lane >> 4, up = g >> 1;
    const v4i *fa = afrag + rt * 128;
    auto frag = [&](int c, int bi, int pc) { return fa[((2 * c + (g >> 1)) * 8 + pc) * 64 + 16 * bi + r16 + 32 * (g & 1)]; };
    auto last = [&](int bi, int pc) { return reinterpret_cast<const long *>(fa + ((KS - 1) * 8 + pc) * 64 + 16 * bi + r16)[g & 1]; };
    const char *la = slot + r16 * PP + 16 * g;
    const int at = r16 * PP + 32 * (KS - 1) + 8 * (g & 1), lo_pl = 32 * PP, bj1 = 16 * PP;
    const v4i zero4 = {0, 0, 0, 0};
    auto mf64 = [](v4i x, v4i y, v4i z) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(x, y, z, 0, 0, 0); };
    auto mf32 = [](long x, long y, v4i z) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(x, y, z, 0, 0, 0); };
    auto win = [&](int at_pos) {
        return static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(s_acc + (at_pos & 511) + (rt >> 1) * SH_AS)));
    };
    if constexpr (LIGHT) {
        v4i t20[NC], t1[NC][2];  // q2 of tap-row half 0; q1, q2 of half 1
        long tf[3];
        enum { TF_Z_Q20, TF_Z_Q11, TF_Q11_Q21 };
#pragma unroll
        for (int c = 0; c < NC; ++c) t20[c] = frag(c, 0, 1), t1[c][0] = frag(c, 1, 0), t1[c][1] = frag(c, 1, 1);
        {
            const long q20 = last(0, 1), q11 = last(1, 0), q21 = last(1, 1);
            tf[TF_Z_Q20] = up ? q20 : 0;
            tf[TF_Z_Q11] = up ? q11 : 0;
            tf[TF_Q11_Q21] = up ? q21 : q11;
        }
        int odd_off[2] = {at + (up ? 0 : lo_pl), at + bj1 + (up ? 0 : lo_pl)};  // [lo_0 ; hi_0], [lo_1 ; hi_1]
        int vzero = 0;  // (a zero the compiler cannot see through)
        asm volatile("" : "+v"(odd_off[0]), "+v"(odd_off[1]), "+v"(vzero));
        // block 0's rows: slots 4 g .. + 3 are tap rows 64 - rot + 4 g .. of the component while 4 g < rot, 4 g - rot .. behind
        const int base0 = cp * 32 + r16 + 4 * g + (4 * g < rot ? 64 - rot : -rot) + 1, base1 = cp * 32 + r16 + 4 * g + 16 - rot + 1;
        clk[0] = __builtin_amdgcn_s_memtime(), clk[1] = __builtin_amdgcn_s_memrealtime();
        for (int t = 0; t < tiles; ++t) {
            asm volatile("s_barrier" ::: "memory");
            v4i hh[NC][2], ll[NC][2];
            long df[2];
            v4i z[2], a1[2], a2[2];
            auto fetch = [&](int c) {
                if (c < NC) {
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) {
                        hh[c][bj] = *reinterpret_cast<const v4i *>(la + 16 * PP * bj + 64 * c);
                        ll[c][bj] = *reinterpret_cast<const v4i *>(la + 32 * PP + 16 * PP * bj + 64 * c);
                    }
                } else {
                    df[0] = *reinterpret_cast<const long *>(slot + odd_off[0]);
                    df[1] = *reinterpret_cast<const long *>(slot + odd_off[1]);
                }
            };
            fetch(0);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                fetch(c + 1);
                const bool first = c == 0;
                z[0] = mf64(t20[c], hh[c][0], first ? zero4 : z[0]);
                a1[0] = mf64(t1[c][0], hh[c][0], first ? zero4 : a1[0]);
                a2[0] = mf64(t1[c][0], ll[c][0], first ? zero4 : a2[0]);
                z[1] = mf64(t20[c], hh[c][1], first ? zero4 : z[1]);
                a1[1] = mf64(t1[c][0], hh[c][1], first ? zero4 : a1[1]);
                a2[1] = mf64(t1[c][0], ll[c][1], first ? zero4 : a2[1]);
                a2[0] = mf64(t1[c][1], hh[c][0], a2[0]);
                a2[1] = mf64(t1[c][1], hh[c][1], a2[1]);
            }
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                z[bj] = mf32(tf[TF_Z_Q20], df[bj], z[bj]);
                a1[bj] = mf32(tf[TF_Z_Q11], df[bj], a1[bj]);
                a2[bj] = mf32(tf[TF_Q11_Q21], df[bj], a2[bj]);
            }
            const unsigned p0 = win(t * 64 + base0), p1 = win(t * 64 + base1);
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // through a VALU instruction the compiler sees: it places the wait states a matrix result needs in front of
                    // its own instructions, not in front of inline asm (fed directly, these adds sent stale registers)
                    const int comb = z[bj][r] + vzero;
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p0), "v"(comb), "n"(4 * (16 * bj + r)));
                }
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int comb = (a1[bj][r] << 8) + a2[bj][r];
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p1), "v"(comb), "n"(4 * (16 * bj + r)));
                }
        }
    } else {
        v4i tq[NC][2][2];
        long tl[2][2], tf[6];
        enum { TF_Z_Q10, TF_Q10_Q11, TF_Z_Q11, TF_Q10_Q20, TF_Q20_Q21, TF_Q11_Q21 };
        enum { DF_L0_H0, DF_L1_L0, DF_H1_H0, DF_L1_H1 };
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) tq[c][bi][pc] = frag(c, bi, pc);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) tl[bi][pc] = last(bi, pc);
        tf[TF_Z_Q10] = up ? tl[0][0] : 0;
        tf[TF_Q10_Q11] = up ? tl[1][0] : tl[0][0];
        tf[TF_Z_Q11] = up ? tl[1][0] : 0;
        tf[TF_Q10_Q20] = up ? tl[0][1] : tl[0][0];
        tf[TF_Q20_Q21] = up ? tl[1][1] : tl[0][1];
        tf[TF_Q11_Q21] = up ? tl[1][1] : tl[1][0];
        int odd_off[4];
        odd_off[DF_L0_H0] = at + (up ? 0 : lo_pl);
        odd_off[DF_L1_L0] = at + lo_pl + (up ? 0 : bj1);
        odd_off[DF_H1_H0] = at + (up ? 0 : bj1);
        odd_off[DF_L1_H1] = at + bj1 + (up ? 0 : lo_pl);
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(odd_off[i]));
        const int base = cp * 32 + (rt & 1) * 32 - rot + r16 + 4 * g + 1;  // (odd rt whenever rot != 0)
        clk[0] = __builtin_amdgcn_s_memtime(), clk[1] = __builtin_amdgcn_s_memrealtime();
        for (int t = 0; t < tiles; ++t) {
            asm volatile("s_barrier" ::: "memory");
            v4i hh[NC][2], ll[NC][2];
            long df[4];
            v4i a1[3], a2[3];
            auto fetch = [&](int c) {
                if (c < NC) {
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) {
                        hh[c][bj] = *reinterpret_cast<const v4i *>(la + 16 * PP * bj + 64 * c);
                        ll[c][bj] = *reinterpret_cast<const v4i *>(la + 32 * PP + 16 * PP * bj + 64 * c);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) df[i] = *reinterpret_cast<const long *>(slot + odd_off[i]);
                }
            };
            fetch(0);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                fetch(c + 1);
                const bool first = c == 0;
                const auto &q = tq[c];
                const auto &hi = hh[c];
                const auto &lw = ll[c];
                a2[1] = mf64(q[0][0], lw[1], first ? zero4 : a2[1]);
                a1[0] = mf64(q[0][0], hi[0], first ? zero4 : a1[0]);
                a2[0] = mf64(q[0][0], lw[0], first ? zero4 : a2[0]);
                a2[1] = mf64(q[1][0], lw[0], a2[1]);
                a1[1] = mf64(q[0][0], hi[1], first ? zero4 : a1[1]);
                a1[2] = mf64(q[1][0], hi[1], first ? zero4 : a1[2]);
                a2[1] = mf64(q[0][1], hi[1], a2[1]);
                a2[2] = mf64(q[1][0], lw[1], first ? zero4 : a2[2]);
                a1[1] = mf64(q[1][0], hi[0], a1[1]);
                a2[1] = mf64(q[1][1], hi[0], a2[1]);
                a2[0] = mf64(q[0][1], hi[0], a2[0]);
                a2[2] = mf64(q[1][1], hi[1], a2[2]);
            }
            a1[0] = mf32(tf[TF_Z_Q10], df[DF_L0_H0], a1[0]);
            a2[1] = mf32(tf[TF_Q10_Q11], df[DF_L1_L0], a2[1]);
            a1[1] = mf32(tf[TF_Q10_Q11], df[DF_H1_H0], a1[1]);
            a2[0] = mf32(tf[TF_Q10_Q20], df[DF_L0_H0], a2[0]);
            a2[1] = mf32(tf[TF_Q20_Q21], df[DF_H1_H0], a2[1]);
            a1[2] = mf32(tf[TF_Z_Q11], df[DF_L1_H1], a1[2]);
            a2[2] = mf32(tf[TF_Q11_Q21], df[DF_L1_H1], a2[2]);
            const unsigned p = win(t * 64 + base);
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int comb = (a1[s][r] << 8) + a2[s][r];
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(4 * (16 * s + r)));
                }
        }
    }
    clk[2] = __builtin_amdgcn_s_memtime(), clk[3] = __builtin_amdgcn_s_memrealtime();
}

template <int BODY>
__global__ __launch_bounds__(768, 3) void k_probe_shape(const v4i *afrag, int *win_out, int tiles, unsigned long long *clk, int rot = 0)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using G = ShapeGeo<BODY>;
    constexpr int KS = SH_KS, PP = G::PP;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int *s_acc = reinterpret_cast<int *>(smem + 2 * G::SLOT);
    // the two parities' tiles: byte b of row `row` of plane `pl` of slot `cp` is the same in either body's layout
    for (int i = tid; i < 2 * 2 * 32 * 32 * KS; i += 768) {
        const int b = i % (32 * KS), row = (i / (32 * KS)) & 31, pl = (i / (32 * KS * 32)) & 1, cp = i / (32 * KS * 64);
        smem[cp * G::SLOT + pl * 32 * PP + row * PP + b] = static_cast<char>(sh_hash(i) >> 13);
    }
    for (int i = tid; i < 2 * SH_AS; i += 768) s_acc[i] = 0;
    __syncthreads();
    const int cp = (wave >> 2) & 1, rt = BODY >= 3 ? (wave & 3) ^ cp : wave & 3, h = lane >> 5, col = lane & 31;
    const char *slot = smem + cp * G::SLOT;
    unsigned long long c0 = 0, r0 = 0, c1 = 0, r1 = 0;
    if (wave >= 8) {  // the loader waves' place: barriers only
        for (int t = 0; t < tiles; ++t) asm volatile("s_barrier" ::: "memory");
    } else if constexpr (BODY >= 3) {
        unsigned long long ck[4];
        if (BODY == 3 && !(rt & 1)) sh_zedge_wave<true>(afrag, slot, s_acc, rt, cp, lane, tiles, rot, ck);
        else sh_zedge_wave<false>(afrag, slot, s_acc, rt, cp, lane, tiles, rot, ck);
        c0 = ck[0], r0 = ck[1], c1 = ck[2], r1 = ck[3];
    } else if constexpr (BODY == 0) {
        v4i fq[KS][2];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc) fq[ks][pc] = afrag[(ks * 8 + rt * 2 + pc) * 64 + lane];
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {  // the half last step: the upper lanes take values 8..15 of the lane 32 below
            const v4i f = fq[KS - 1][pc];
            const int z0 = __shfl(f.z, lane ^ 32, 64), w0 = __shfl(f.w, lane ^ 32, 64);
            if (h) {
                fq[KS - 1][pc].x = z0;
                fq[KS - 1][pc].y = w0;
            }
        }
        const char *la = slot + col * PP + 16 * h;
        const v16i zero16 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
        for (int t = 0; t < tiles; ++t) {
            asm volatile("s_barrier" ::: "memory");
            typedef int v2i __attribute__((ext_vector_type(2)));
            v4i hh[KS], ll[KS];
            v16i acc1 = zero16, acc2 = zero16;
            auto fetch = [&](int ks) {
                if (ks == KS - 1) {
                    const v2i h2 = *reinterpret_cast<const v2i *>(la - 8 * h + 32 * ks);
                    const v2i l2 = *reinterpret_cast<const v2i *>(la - 8 * h + 32 * PP + 32 * ks);
                    hh[ks].x = h2.x, hh[ks].y = h2.y, ll[ks].x = l2.x, ll[ks].y = l2.y;
                } else {
                    hh[ks] = *reinterpret_cast<const v4i *>(la + 32 * ks);
                    ll[ks] = *reinterpret_cast<const v4i *>(la + 32 * PP + 32 * ks);
                }
            };
            fetch(0);
            fetch(1);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const v4i hi = hh[ks], lo = ll[ks];
                if (ks + 2 < KS) fetch(ks + 2);
                if (ks == KS - 1) {
                    auto pack = [](int x, int y) { return static_cast<long>((static_cast<unsigned long long>(static_cast<unsigned>(y)) << 32) | static_cast<unsigned>(x)); };
                    const long a1 = pack(fq[ks][0].x, fq[ks][0].y), a2 = pack(fq[ks][1].x, fq[ks][1].y);
                    const long bh = pack(hi.x, hi.y), bl = pack(lo.x, lo.y);
                    acc1 = __builtin_amdgcn_mfma_i32_32x32x16_i8(a1, bh, acc1, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_i32_32x32x16_i8(a1, bl, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_i32_32x32x16_i8(a2, bh, acc2, 0, 0, 0);
                } else {
                    acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], hi, acc1, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][0], lo, acc2, 0, 0, 0);
                    acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(fq[ks][1], hi, acc2, 0, 0, 0);
                }
            }
            const unsigned p = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(
                s_acc + ((t * 64 + cp * 32 + col + 4 * h + 1) & 511) + (rt >> 1) * SH_AS + (rt & 1) * 32)));
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int comb = (acc1[q] << 8) + acc2[q];
                asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(4 * ((q & 3) + 8 * (q >> 2))));
            }
        }
        c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    } else {
        constexpr int NC = KS / 2;  // 64-value chunks; KS odd: one 32-value step behind them
        constexpr bool FOLD = BODY == 2;
        const int r16 = lane & 15, g = lane >> 4, up = g >> 1;
        v4i tq[NC][2][2];  // [chunk][tap-row half][piece]
        long tl[2][2];     // the odd last k step, BODY 1: values 8 g .. + 7 (16 .. 31 are zero taps)
        long tf[6];        // BODY 2: [x | y] -- lane groups 0, 1 values 8 (g & 1) .. + 7 of x, groups 2, 3 those of y
        enum { TF_Z_Q10, TF_Q10_Q11, TF_Z_Q11, TF_Q10_Q20, TF_Q20_Q21, TF_Q11_Q21 };  // q<piece><tap-row half>, Z = zeros
        enum { DF_L0_H0, DF_L1_L0, DF_H1_H0, DF_L1_H1 };  // [u ; v] of data bytes: plane H / L of data-row half 0 / 1
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) tq[c][bi][pc] = afrag[((2 * c + (g >> 1)) * 8 + rt * 2 + pc) * 64 + 16 * bi + r16 + 32 * (g & 1)];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int pc = 0; pc < 2; ++pc)
                tl[bi][pc] = reinterpret_cast<const long *>(afrag + ((KS - 1) * 8 + rt * 2 + pc) * 64 + 16 * bi + r16 + 32 * (FOLD ? 0 : up))[g & 1];
        tf[TF_Z_Q10] = up ? tl[0][0] : 0;
        tf[TF_Q10_Q11] = up ? tl[1][0] : tl[0][0];
        tf[TF_Z_Q11] = up ? tl[1][0] : 0;
        tf[TF_Q10_Q20] = up ? tl[0][1] : tl[0][0];
        tf[TF_Q20_Q21] = up ? tl[1][1] : tl[0][1];
        tf[TF_Q11_Q21] = up ? tl[1][1] : tl[1][0];
        const char *la = slot + r16 * PP + 16 * g;
        // the odd step's four 8-byte reads, an offset register each that the compiler cannot relate (paired into
        // ds_read2st64_b64 they are a 4-way conflict at this pitch).  BODY 1: [plane][data-row half]; BODY 2: DF_*
        int odd_off[4];
        {
            const int at = r16 * PP + 32 * (KS - 1), lo_pl = 32 * PP, bj1 = 16 * PP;
            if (FOLD) {
                odd_off[DF_L0_H0] = at + 8 * (g & 1) + (up ? 0 : lo_pl);
                odd_off[DF_L1_L0] = at + 8 * (g & 1) + lo_pl + (up ? 0 : bj1);
                odd_off[DF_H1_H0] = at + 8 * (g & 1) + (up ? 0 : bj1);
                odd_off[DF_L1_H1] = at + 8 * (g & 1) + bj1 + (up ? 0 : lo_pl);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) odd_off[i] = at + 8 * g + lo_pl * (i >> 1) + bj1 * (i & 1);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(odd_off[i]));
        }
        const v4i zero4 = {0, 0, 0, 0};
        c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
        for (int t = 0; t < tiles; ++t) {
            asm volatile("s_barrier" ::: "memory");
            v4i hh[NC][2], ll[NC][2];
            long ho[2], lo[2], df[4];
            v4i a1[3], a2[3];
            auto fetch = [&](int c) {
                if (c < NC) {
#pragma unroll
                    for (int bj = 0; bj < 2; ++bj) {
                        hh[c][bj] = *reinterpret_cast<const v4i *>(la + 16 * PP * bj + 64 * c);
                        ll[c][bj] = *reinterpret_cast<const v4i *>(la + 32 * PP + 16 * PP * bj + 64 * c);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) df[i] = *reinterpret_cast<const long *>(slot + odd_off[i]);
                    ho[0] = df[0], ho[1] = df[1], lo[0] = df[2], lo[1] = df[3];  // (BODY 1's names)
                }
            };
            // the twelve products of a step; an accumulator's uses lie at least two instructions apart
            auto step = [&](auto mf, const auto &q, const auto &hi, const auto &lw, bool first) {
                a2[1] = mf(q[0][0], lw[1], first ? zero4 : a2[1]);
                a1[0] = mf(q[0][0], hi[0], first ? zero4 : a1[0]);
                a2[0] = mf(q[0][0], lw[0], first ? zero4 : a2[0]);
                a2[1] = mf(q[1][0], lw[0], a2[1]);
                a1[1] = mf(q[0][0], hi[1], first ? zero4 : a1[1]);
                a1[2] = mf(q[1][0], hi[1], first ? zero4 : a1[2]);
                a2[1] = mf(q[0][1], hi[1], a2[1]);
                a2[2] = mf(q[1][0], lw[1], first ? zero4 : a2[2]);
                a1[1] = mf(q[1][0], hi[0], a1[1]);
                a2[1] = mf(q[1][1], hi[0], a2[1]);
                a2[0] = mf(q[0][1], hi[0], a2[0]);
                a2[2] = mf(q[1][1], hi[1], a2[2]);
            };
            auto mf64 = [](v4i x, v4i y, v4i z) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(x, y, z, 0, 0, 0); };
            auto mf32 = [](long x, long y, v4i z) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(x, y, z, 0, 0, 0); };
            fetch(0);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (c + 1 < NC + (KS & 1)) fetch(c + 1);
                step(mf64, tq[c], hh[c], ll[c], c == 0);
            }
            if constexpr (FOLD) {
                // the odd step's twelve K = 16 products folded along K: two products of one accumulator per instruction
                a1[0] = mf32(tf[TF_Z_Q10], df[DF_L0_H0], a1[0]);
                a2[1] = mf32(tf[TF_Q10_Q11], df[DF_L1_L0], a2[1]);
                a1[1] = mf32(tf[TF_Q10_Q11], df[DF_H1_H0], a1[1]);
                a2[0] = mf32(tf[TF_Q10_Q20], df[DF_L0_H0], a2[0]);
                a2[1] = mf32(tf[TF_Q20_Q21], df[DF_H1_H0], a2[1]);
                a1[2] = mf32(tf[TF_Z_Q11], df[DF_L1_H1], a1[2]);
                a2[2] = mf32(tf[TF_Q11_Q21], df[DF_L1_H1], a2[2]);
            } else if (KS & 1) {
                step(mf32, tl, ho, lo, NC == 0);
            }
            const unsigned p = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(
                s_acc + ((t * 64 + cp * 32 + (rt & 1) * 32 + r16 + 4 * g + 1) & 511) + (rt >> 1) * SH_AS)));
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int comb = (a1[s][r] << 8) + a2[s][r];
                    asm volatile("ds_add_u32 %0, %1 offset:%2" ::"v"(p), "v"(comb), "n"(4 * (16 * s + r)));
                }
        }
        c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    }
    if (lane == 0 && wave == 0) {
        clk[2 * blockIdx.x] = c1 - c0;
        clk[2 * blockIdx.x + 1] = r1 - r0;
    }
    // where the waves run: SIMD_ID of HW_ID (bits 5:4), one entry per wave of workgroup 0, behind the clocks
    if (BODY >= 3 && lane == 0 && blockIdx.x == 0) clk[512 + wave] = __builtin_amdgcn_s_getreg(4 | (4 << 6) | (1 << 11));
    // the window this block leaves, folded over the guard's aliases: equal for the two bodies
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (blockIdx.x == 0)
        for (int i = tid; i < 1024; i += 768) {
            const int s = i & 511, o = (i >> 9) * SH_AS;
            win_out[i] = s_acc[o + s] + (s < 64 ? s_acc[o + 512 + s] : 0);
        }
}

// bare issue rate of one MFMA form: one wave per SIMD, eight independent accumulators, cycles per instruction
template <int FORM>  // 0: 32x32x32, 1: 32x32x16, 2: 16x16x64, 3: 16x16x32
__global__ __launch_bounds__(256) void k_probe_rate(const v4i *taps, int *sink, int n, unsigned long long *clk)
{
    const int lane = threadIdx.x & 63;
    const v4i x = taps[lane], y = taps[64 + lane];
    const long xl = (static_cast<long>(x.y) << 32) | static_cast<unsigned>(x.x), yl = (static_cast<long>(y.y) << 32) | static_cast<unsigned>(y.x);
    v16i b[4] = {};
    v4i s[8] = {};
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // (inline asm: left to itself the compiler keeps these sums in accumulation registers and copies all of them
            // to and fro in every iteration; an accumulator's next use is 4 or 8 instructions away, past every hazard)
            if constexpr (FORM == 0) asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+v"(b[j & 3]) : "v"(x), "v"(y));
            if constexpr (FORM == 1) asm volatile("v_mfma_i32_32x32x16_i8 %0, %1, %2, %0" : "+v"(b[j & 3]) : "v"(xl), "v"(yl));
            if constexpr (FORM == 2) asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, %0" : "+v"(s[j]) : "v"(x), "v"(y));
            if constexpr (FORM == 3) asm volatile("v_mfma_i32_16x16x32_i8 %0, %1, %2, %0" : "+v"(s[j]) : "v"(xl), "v"(yl));
        }
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // (the last results, before the VALU reads them)
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc += b[j][q];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += s[j].x + s[j].y + s[j].z + s[j].w;
    if (acc == 0x12345678) sink[0] = acc;
    if (threadIdx.x == 0 && blockIdx.x == 0) clk[0] = c1 - c0;
}

template <int FORM>
static void run_rate(const v4i *taps, int *sink, unsigned long long *clk)
{
    const int n = 100000;
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((k_probe_rate<FORM>), dim3(256), dim3(256), 0, 0, taps, sink, n, clk);
    unsigned long long h = 0;
    hipMemcpy(&h, clk, 8, hipMemcpyDeviceToHost);
    static const char *names[4] = {"v_mfma_i32_32x32x32_i8", "v_mfma_i32_32x32x16_i8", "v_mfma_i32_16x16x64_i8", "v_mfma_i32_16x16x32_i8"};
    printf("%s: %.2f cycles per instruction, one wave per SIMD, back to back\n", names[FORM], double(h) / (8.0 * n));
}

// LDS access patterns of the two bodies, one per kernel name, for a counters-only run (SQ_LDS_BANK_CONFLICT,
// SQ_LDS_IDX_ACTIVE, SQ_INSTS_LDS per dispatch): `kstep_probe lds`.
//   KIND 0: ds_read_b128, lane l at row l & 15, unit l >> 4, rows P units apart (the 16x16x64 data operand)
//   KIND 1: ds_read_b128, lane l at row l & 31, unit l >> 5, rows P units apart (the 32x32x32 data operand)
//   KIND 2: ds_read_b64, lane l at row l & 15, 8 (l >> 4) bytes into the row (the 16x16x32 data operand)
//   KIND 3: ds_add_u32 at position (l & 15) + 4 (l >> 4) (the 16x16 blocks' scatter); KIND 4: at (l & 31) + 4 (l >> 5)
//   KIND 5..8: ds_read_b64, lane l at row l & 15, 8 ((l >> 4) & 1) bytes into the row, lane groups 0, 1 in one (plane,
//     data-row half) of a slot of 64 rows and groups 2, 3 in another (the folded odd step's data operands [lo0 ; hi0],
//     [lo1 ; lo0], [hi1 ; hi0], [lo1 ; hi1]: planes 32 rows apart, halves 16)
template <int KIND, int P>
__global__ __launch_bounds__(64) void k_probe_lds(int *sink, int n)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    for (int i = lane; i < 4096; i += 64) reinterpret_cast<int *>(smem)[i] = i;
    __syncthreads();
    static_assert(KIND < 5 || 64 * P * 16 <= 16384, "the slot of 64 rows must fit the kernel's LDS");
    const int up = lane >> 5, at = (lane & 15) * P * 16 + 8 * ((lane >> 4) & 1), lo_pl = 32 * P * 16, bj1 = 16 * P * 16;
    int off;
    if (KIND == 0) off = (lane & 15) * P * 16 + 16 * (lane >> 4);
    else if (KIND == 1) off = (lane & 31) * P * 16 + 16 * (lane >> 5);
    else if (KIND == 2) off = (lane & 15) * P * 16 + 8 * (lane >> 4);
    else if (KIND == 3) off = 4 * ((lane & 15) + 4 * (lane >> 4));
    else if (KIND == 4) off = 4 * ((lane & 31) + 4 * (lane >> 5));
    else if (KIND == 5) off = at + (up ? 0 : lo_pl);
    else if (KIND == 6) off = at + lo_pl + (up ? 0 : bj1);
    else if (KIND == 7) off = at + (up ? 0 : bj1);
    else off = at + bj1 + (up ? 0 : lo_pl);
    const unsigned p = static_cast<unsigned>(reinterpret_cast<size_t>((__attribute__((address_space(3))) const void *)(smem + off)));
    v4i v = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        if (KIND <= 1) asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(p) : "memory");
        else if (KIND == 2 || KIND >= 5) asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(*reinterpret_cast<long *>(&v)) : "v"(p) : "memory");
        else asm volatile("ds_add_u32 %0, %1\n\ts_waitcnt lgkmcnt(0)" ::"v"(p), "v"(lane) : "memory");
    }
    if (v.x == 0x12345678) sink[0] = v.y;
}

template <int KIND, int P>
static void run_lds(int *sink)
{
    hipLaunchKernelGGL((k_probe_lds<KIND, P>), dim3(256), dim3(64), 16384, 0, sink, 1000);
    hipDeviceSynchronize();
}

static int lds_main()
{
    int *sink;
    hipMalloc(&sink, 64);
    run_lds<0, 13>(sink);
    run_lds<0, 14>(sink);
    run_lds<0, 15>(sink);
    run_lds<0, 16>(sink);
    run_lds<0, 18>(sink);
    run_lds<1, 14>(sink);
    run_lds<1, 15>(sink);
    run_lds<2, 14>(sink);
    run_lds<2, 15>(sink);
    run_lds<3, 0>(sink);
    run_lds<4, 0>(sink);
    // the odd step's reads at the plane pitch of 7 and of 3 k steps: as they were, and the folded step's four
    run_lds<2, 6>(sink);
    run_lds<5, 14>(sink);
    run_lds<6, 14>(sink);
    run_lds<7, 14>(sink);
    run_lds<8, 14>(sink);
    run_lds<5, 6>(sink);
    run_lds<6, 6>(sink);
    run_lds<7, 6>(sink);
    run_lds<8, 6>(sink);
    return 0;
}

struct ShapeResult {
    double ns_per_round, ghz;
    std::vector<int> win;
    std::vector<unsigned long long> simd;
};

// `seconds` of back-to-back launches; the time and the in-kernel clock (median over workgroups) of the last batch
template <int BODY>
static ShapeResult run_shape(const v4i *afrag, int *win, unsigned long long *clk, int tiles, double seconds, int rot = 0)
{
    using G = ShapeGeo<BODY>;
    hipFuncSetAttribute(reinterpret_cast<const void *>(k_probe_shape<BODY>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    constexpr int BATCH = 8;
    double total_ms = 0;
    float ms = 0;
    while (total_ms < seconds * 1e3) {
        hipEventRecord(e0);
        for (int i = 0; i < BATCH; ++i) hipLaunchKernelGGL((k_probe_shape<BODY>), dim3(256), dim3(768), G::LDS, 0, afrag, win, tiles, clk, rot);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) {
            printf("launch failed: %s\n", hipGetErrorString(hipGetLastError()));
            exit(1);
        }
        hipEventElapsedTime(&ms, e0, e1);
        total_ms += ms;
    }
    std::vector<unsigned long long> h(512);
    hipMemcpy(h.data(), clk, 512 * 8, hipMemcpyDeviceToHost);
    std::vector<double> ghz(256);
    for (int i = 0; i < 256; ++i) ghz[i] = double(h[2 * i]) / double(h[2 * i + 1]) * 0.1;
    std::sort(ghz.begin(), ghz.end());
    ShapeResult r;
    r.ns_per_round = ms * 1e6 / (double(BATCH) * tiles);
    r.ghz = ghz[128];
    r.win.resize(1024);
    hipMemcpy(r.win.data(), win, 1024 * 4, hipMemcpyDeviceToHost);
    if (BODY >= 3) {  // (zedge_main's clock buffer has the room)
        unsigned long long simd[12];
        hipMemcpy(simd, clk + 512, sizeof simd, hipMemcpyDeviceToHost);
        r.simd.assign(simd, simd + 12);
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return r;
}

// kstep_probe zedge [seconds per run] [pairs]: the folded 16x16x64 body (BODY 2) against the same with the zero-q1 edge rows
// skipped and a light and a heavy wave on every SIMD (BODY 3), and against the pairing alone (BODY 4).  Taps: random bytes,
// q1 zero in config 2's zero-q1 rows (q - 1 = 52..63 and 0..9 of either component); BODY 3 reads them rotated by 12 slots
// and scatters every row to the position it had, so the three windows of sums must be equal.  Under a counters-only
// profiler run (`kstep_probe zedge 0.01 1`) each body is a kernel name of its own.
static int zedge_main(double seconds, int pairs)
{
    const int tiles = 20000, rot = 12;
    std::vector<signed char> q(2 * 128 * 224), ha(SH_KS * 8 * 64 * 16), hr(ha.size());
    unsigned seed = 12345u;
    for (int pc = 0; pc < 2; ++pc)
        for (int row = 0; row < 128; ++row)
            for (int k = 0; k < 224; ++k) {
                seed = seed * 1664525u + 1013904223u;
                const int qm = row & 63;
                const bool zero_q1 = qm >= 52 || qm < 10;
                q[(pc * 128 + row) * 224 + k] = (k < 208 && !(pc == 0 && zero_q1)) ? static_cast<signed char>(seed >> 24) : 0;
            }
    for (int ks = 0; ks < SH_KS; ++ks)
        for (int rp = 0; rp < 8; ++rp)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j) {
                    const int k = 32 * ks + 16 * (l >> 5) + j, pc = rp & 1, comp = rp >> 2, slot = 32 * ((rp >> 1) & 1) + (l & 31);
                    const size_t at = ((ks * 8 + rp) * 64 + l) * 16 + j;
                    ha[at] = q[(pc * 128 + comp * 64 + slot) * 224 + k];
                    hr[at] = q[(pc * 128 + comp * 64 + ((slot - rot + 64) & 63)) * 224 + k];
                }
    v4i *afrag, *afrag_rot;
    int *win;
    unsigned long long *clk;
    hipMalloc(&afrag, ha.size());
    hipMalloc(&afrag_rot, hr.size());
    hipMemcpy(afrag, ha.data(), ha.size(), hipMemcpyHostToDevice);
    hipMemcpy(afrag_rot, hr.data(), hr.size(), hipMemcpyHostToDevice);
    hipMalloc(&win, 1024 * 4);
    hipMalloc(&clk, (512 + 16) * 8);
    hipMemset(clk, 0, (512 + 16) * 8);
    int bad = 0, slower = 0;
    const ShapeResult ref = run_shape<0>(afrag, win, clk, tiles, 1e-3);  // (one batch: the 32x32x32 body's sums)
    for (int p = 0; p < pairs; ++p) {
        const ShapeResult a = run_shape<2>(afrag, win, clk, tiles, seconds);
        const ShapeResult b = run_shape<3>(afrag_rot, win, clk, tiles, seconds, rot);
        const ShapeResult c = run_shape<4>(afrag, win, clk, tiles, seconds);
        int diff = 0, diff_pair = 0, diff_ref = 0, nonzero = 0;
        for (int i = 0; i < 1024; ++i) diff += a.win[i] != b.win[i], diff_pair += a.win[i] != c.win[i], diff_ref += ref.win[i] != a.win[i], nonzero += a.win[i] != 0;
        bad += diff + diff_pair + diff_ref + (nonzero < 512);
        slower += !(b.ns_per_round < a.ns_per_round);
        printf("pair %d: shipped body %.1f ns per round at %.3f GHz; zero-q1 blocks skipped + light/heavy pairing: %.1f ns at %.3f GHz, ratio %.4f; pairing "
               "alone: %.1f ns at %.3f GHz, ratio %.4f; windows differ in %d / %d of 1024 sums, the shipped body's from the 32x32x32 body's in %d (%d nonzero, first %d)\n",
               p, a.ns_per_round, a.ghz, b.ns_per_round, b.ghz, b.ns_per_round / a.ns_per_round, c.ns_per_round, c.ghz, c.ns_per_round / a.ns_per_round, diff,
               diff_pair, diff_ref, nonzero, a.win[7]);
        if (p == 0) {
            printf("SIMD of waves 0..11 of workgroup 0 (HW_ID): with skipping");
            for (int w = 0; w < 12; ++w) printf(" %llu", b.simd[w]);
            printf("; pairing alone");
            for (int w = 0; w < 12; ++w) printf(" %llu", c.simd[w]);
            printf("\n");
        }
    }
    printf("gate (wall per round lower in every pair): %s; sums %s\n", slower ? "NOT met" : "met", bad ? "DIFFER" : "equal");
    return bad ? 1 : 0;
}

// kstep_probe shape [seconds per run] [pairs]; `fold`: the 16x16x64 body against the one with the folded odd step
static int shape_main(double seconds, int pairs, bool fold)
{
    const int tiles = 20000;
    std::vector<signed char> ha(SH_KS * 8 * 64 * 16);
    unsigned seed = 12345u;
    for (int ks = 0; ks < SH_KS; ++ks)
        for (int rp = 0; rp < 8; ++rp)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 16; ++j) {
                    seed = seed * 1664525u + 1013904223u;
                    const int k = 32 * ks + 16 * (l >> 5) + j;  // lane l holds tap row l & 31, values 16 (l >> 5) + j of the k step
                    ha[((ks * 8 + rp) * 64 + l) * 16 + j] = k < 208 ? static_cast<signed char>(seed >> 24) : 0;
                }
    v4i *afrag;
    int *win, *sink;
    unsigned long long *clk;
    hipMalloc(&afrag, ha.size());
    hipMemcpy(afrag, ha.data(), ha.size(), hipMemcpyHostToDevice);
    hipMalloc(&win, 1024 * 4);
    hipMalloc(&sink, 64);
    hipMalloc(&clk, 512 * 8);
    int bad = 0;
    if (fold) {
        const ShapeResult ref = run_shape<0>(afrag, win, clk, tiles, 1e-3);  // (one batch: the 32x32x32 body's sums)
        for (int p = 0; p < pairs; ++p) {
            const ShapeResult a = run_shape<1>(afrag, win, clk, tiles, seconds);
            const ShapeResult b = run_shape<2>(afrag, win, clk, tiles, seconds);
            int diff = 0, diff_ref = 0;
            for (int i = 0; i < 1024; ++i) diff += a.win[i] != b.win[i], diff_ref += ref.win[i] != b.win[i];
            bad += diff + diff_ref;
            printf("pair %d: 16x16x64 body, odd step of 12 x 16x16x32: %.1f ns per round at %.3f GHz; folded to 7: %.1f ns at %.3f GHz; ratio %.4f; "
                   "windows differ in %d of 1024 sums, from the 32x32x32 body's in %d (first %d)\n",
                   p, a.ns_per_round, a.ghz, b.ns_per_round, b.ghz, b.ns_per_round / a.ns_per_round, diff, diff_ref, b.win[7]);
        }
        return bad ? 1 : 0;
    }
    run_rate<0>(afrag, sink, clk);
    run_rate<1>(afrag, sink, clk);
    run_rate<2>(afrag, sink, clk);
    run_rate<3>(afrag, sink, clk);
    for (int p = 0; p < pairs; ++p) {
        const ShapeResult a = run_shape<0>(afrag, win, clk, tiles, seconds);
        const ShapeResult b = run_shape<1>(afrag, win, clk, tiles, seconds);
        int diff = 0;
        for (int i = 0; i < 1024; ++i) diff += a.win[i] != b.win[i];
        bad += diff;
        printf("pair %d: 32x32x32 body %.1f ns per round (two tiles per SIMD pair of waves) at %.3f GHz; 16x16x64 body %.1f ns at %.3f GHz; ratio %.4f; "
               "windows differ in %d of 1024 sums (first %d)\n",
               p, a.ns_per_round, a.ghz, b.ns_per_round, b.ghz, b.ns_per_round / a.ns_per_round, diff, a.win[7]);
    }
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "lds") return lds_main();
    if (argc > 1 && std::string(argv[1]) == "zedge") return zedge_main(argc > 2 ? atof(argv[2]) : 2.0, argc > 3 ? atoi(argv[3]) : 5);
    if (argc > 1 && (std::string(argv[1]) == "shape" || std::string(argv[1]) == "fold"))
        return shape_main(argc > 2 ? atof(argv[2]) : 2.0, argc > 3 ? atoi(argv[3]) : 4, std::string(argv[1]) == "fold");
    const int tiles = argc > 1 ? atoi(argv[1]) : 20000;
    v4i *taps;
    int *sink;
    unsigned long long *cyc;
    hipMalloc(&taps, 16 * 2 * 2 * 64 * 16 + 4096);
    hipMemset(taps, 1, 16 * 2 * 2 * 64 * 16 + 4096);
    hipMalloc(&sink, 64);
    hipMalloc(&cyc, 256 * 8);
    const bool rt_only = argc > 2;
    if (!rt_only) {
    run<0>(taps, sink, cyc, tiles);
    run<1>(taps, sink, cyc, tiles);
    run<2>(taps, sink, cyc, tiles);
    run<3>(taps, sink, cyc, tiles);
    run<4>(taps, sink, cyc, tiles);
    // mode 2 variants: 1 = prefetch 4 steps ahead, 2 = reads behind the step's MFMAs, 4 = compiler's own schedule,
    // 8 = one read per step, 16 = four ds_read_b64 per step
    run<2, 1>(taps, sink, cyc, tiles);
    run<2, 2>(taps, sink, cyc, tiles);
    run<2, 4>(taps, sink, cyc, tiles);
    run<2, 8>(taps, sink, cyc, tiles);
    run<2, 16>(taps, sink, cyc, tiles);
    run<2, 3>(taps, sink, cyc, tiles);
    run<2, 5>(taps, sink, cyc, tiles);
    run<3, 4>(taps, sink, cyc, tiles);  // barrier per tile, compiler's schedule
    run<4, 4>(taps, sink, cyc, tiles);  // + scatter
    }
    run_rt<13, 1, 8>(taps, sink, tiles, cyc);
    run_rt<13, 2, 4>(taps, sink, tiles, cyc);
    run_rt<13, 1, 4>(taps, sink, tiles, cyc);
    run_rt<7, 1, 8>(taps, sink, tiles, cyc);
    run_rt<7, 2, 8>(taps, sink, tiles, cyc);
    run_rt<7, 2, 4>(taps, sink, tiles, cyc);
    run_rt<7, 4, 4>(taps, sink, tiles, cyc);
    // the round structure: one barrier domain of 8 waves against two of 4 on the same CU, and one wave per SIMD with 64 rows
    run_rt<13, 1, 8, 1, 1>(taps, sink, tiles, cyc);
    run_rt<13, 1, 4, 1, 2>(taps, sink, tiles, cyc);
    run_rt<13, 2, 4, 1, 1>(taps, sink, tiles, cyc);
    run_rt<13, 2, 4, 1, 2>(taps, sink, tiles, cyc);
    run_rt<7, 1, 8, 1, 1>(taps, sink, tiles, cyc);
    run_rt<7, 1, 4, 1, 2>(taps, sink, tiles, cyc);
    run_rt<7, 2, 4, 1, 1>(taps, sink, tiles, cyc);
    run_rt<7, 2, 4, 1, 2>(taps, sink, tiles, cyc);
    run_cont<13, 8>(taps, sink, tiles, cyc);
    run_cont<13, 8, 1>(taps, sink, tiles, cyc);
    run_cont<13, 8, 2>(taps, sink, tiles, cyc);
    run_cont<13, 8, 3>(taps, sink, tiles, cyc);
    run_cont<13, 8, 4>(taps, sink, tiles, cyc);
    run_cont<7, 8>(taps, sink, tiles, cyc);
    run_cont<7, 8, 3>(taps, sink, tiles, cyc);
    if (argc > 3) return 0;
    run_rt<13, 1, 4, 2, 2>(taps, sink, tiles, cyc);
    run_rt<13, 2, 4, 2, 2>(taps, sink, tiles, cyc);
    run_rt<7, 1, 4, 2, 2>(taps, sink, tiles, cyc);
    run_rt<7, 2, 4, 2, 2>(taps, sink, tiles, cyc);
    return 0;
}
