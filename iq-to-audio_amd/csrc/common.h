// common.h -- shared helpers for the gfx950 hot-path library (error plumbing, launch checks).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/iqa_hotpath.h"

namespace iqa {

constexpr int kWave = 64;  // CDNA wavefront width

void set_error(const char *fmt, ...);

inline int fail_inval(const char *what)
{
    set_error("invalid argument: %s", what);
    return IQA_EINVAL;
}

inline int check_launch(const char *kernel)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("launch of %s failed: %s", kernel, hipGetErrorString(e));
        return IQA_EHIP;
    }
    return IQA_OK;
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline dim3 grid1d(int64_t n, int block) { return dim3(static_cast<unsigned>((n + block - 1) / block)); }

inline int frame_bytes(int fmt)
{
    switch (fmt) {
        case IQA_FMT_S16: return 4;
        case IQA_FMT_U8: return 2;
        case IQA_FMT_F32: return 8;
        default: return 0;
    }
}

// 64-lane butterfly sum (every lane ends with the total).
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
// (the integer forms: the order of the sum does not matter, the total is exact)
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// |z| as numpy >= 1.25 forms np.abs(complex64) on a host with fused multiply-add (x86 with FMA3 / AVX-512, aarch64), all in
// float32 (numpy's loops_unary_complex): larger * sqrt(1 + (smaller / larger)^2) with one fused multiply-add, and 0 / 0 taken
// as 0.  This is what numpy computes, not something it documents: a build without the fused form (7 k of 200 k samples differ)
// or an older one that calls hypotf gives other last bits, and tests/test_gpu_scan_exact.py's 1-ulp envelope bound and 1e-12
// mean-power bound then miss with no fault here.  The value is up to 2 float32 ulps from the true |z|, and so from hypotf and
// from a root taken in float64 (a third of all samples differ); the reference is numpy's, so this is the one to match.  The
// division and the root are correctly rounded at the default compiler flags (Makefile: no fast-math).
__device__ __forceinline__ float np_abs_c64(float re, float im)
{
    const float a = fabsf(re), b = fabsf(im);
    const float larger = fmaxf(a, b), smaller = fminf(a, b);
    const float ratio = (larger > 0.0f) ? smaller / larger : 0.0f;
    return sqrtf(fmaf(ratio, ratio, 1.0f)) * larger;
}

}  // namespace iqa
