// The image-side 1x1 convolutions and the uint8 ingest for images that are not RGB: J = 1, 2, 4 image channels (grayscale, gray + alpha,
// RGBA) and J = 8 (the conditional discriminator's [RGBA image, label embedding] input).  The 3-channel kernels of pointwise.hip stay what
// they are; these are their J-templated siblings with the same launch geometry (rgb_in_run / rgb_out_launch and the comments there):
// a grid-stride loop kernel for small launches, short-lived blocks that move one 16-byte vector of y / x per thread per trip above a
// size threshold, two-stage fixed-order fp64 partials for the weight gradient.  The image side of a pixel is ONE load of 4 J bytes (J = 8:
// two 16-byte loads); with J = 1 the lanes that share a pixel read the same dword (one request, broadcast), not a wider vector each.
#include "common.h"

// A/B switch and size threshold of the short-lived-block kernels: 0 = the loop kernels always, else the smallest number of 16-byte
// vectors of y (img_in) / of pixels (img_out) that takes them.  Measured: tools/imgconv_probe.py --sweep, see img_in_run below.
SGX_SWITCH(img1_min, "SGX_IMG1_MIN", 65536)
// The image channel counts the convolutions are instantiated for, and those of the uint8 ingest: sgx_by_int<IMG_JS>(J, f) calls f with J
// as a compile-time constant (common.h); the entry points have refused every other J before.
#define IMG_JS 1, 2, 4, 8
#define IMG_U8_JS 1, 2, 3, 4

template <int J>
__device__ __forceinline__ void img_load(const float* __restrict__ p, float (&v)[J]) {
    static_assert(J == 1 || J == 2 || J == 4 || J == 8, "image channels");
    if constexpr (J == 1) {
        v[0] = p[0];
    } else if constexpr (J == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y;
    } else {
#pragma unroll
        for (int q = 0; q < J / 4; ++q) {
            const float4 t = reinterpret_cast<const float4*>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    }
}
template <int J>
__device__ __forceinline__ void img_store(float* __restrict__ p, const float (&v)[J]) {
    static_assert(J == 1 || J == 2 || J == 4 || J == 8, "image channels");
    if constexpr (J == 1) {
        p[0] = v[0];
    } else if constexpr (J == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int q = 0; q < J / 4; ++q) reinterpret_cast<float4*>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
}

// ---------------------------------------------------------------- image -> activations: y[p][c] = bias[c] + sum_j img[p][j] (wscale W(j,c))
// Sum order (both kernels, so they agree bit for bit): ((i0 w0 + i1 w1) + i2 w2) + ..., the bias added last -- rgb_in_kernel's order.
template <typename T, int J>
__global__ void img_in_kernel(const float* __restrict__ img, const float* __restrict__ w, int sj, int sc, float wscale,
                              const float* __restrict__ bias, T* __restrict__ y, size_t npix, int C) {
    constexpr int VE = VecTraits<T>::VE;
    const int cv = C / VE;                                   // divides the grid stride (grid_for_hoisted)
    const size_t nvec = npix * cv;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c0 = (int)(i0 % cv) * VE;                      // the thread's channel group never changes: hoist its weights
    float tw[J][VE], bb[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) {
#pragma unroll
        for (int j = 0; j < J; ++j) tw[j][k] = wscale * w[j * sj + (c0 + k) * sc];
        bb[k] = bias ? bias[c0 + k] : 0.f;
    }
    for (size_t i = i0; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        float px[J], v[VE];
        img_load<J>(img + (i / cv) * J, px);
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            float s = px[0] * tw[0][k];
#pragma unroll
            for (int j = 1; j < J; ++j) s += px[j] * tw[j][k];
            v[k] = bb[k] + s;
        }
        VecTraits<T>::store(y + i * VE, v);
    }
}
// The same as short-lived blocks: four vectors per thread, the (J + 1) x C table (scaled weights, bias) through LDS once per block, the
// pixel loads requested before the block waits for its table.
template <typename T, int J>
__global__ __launch_bounds__(256) void img_in1_kernel(const float* __restrict__ img, const float* __restrict__ w, int sj, int sc, float wscale,
                                                      const float* __restrict__ bias, T* __restrict__ y, unsigned nvec, int C) {
    constexpr int VE = VecTraits<T>::VE, U = 4;
    extern __shared__ float tw[];                            // [J + 1][C]: wscale * W[j][c], bias[c]
    for (int c = threadIdx.x; c < C; c += 256) {
#pragma unroll
        for (int j = 0; j < J; ++j) tw[j * C + c] = wscale * w[j * sj + c * sc];
        tw[J * C + c] = bias ? bias[c] : 0.f;
    }
    const unsigned i0 = blockIdx.x * (256u * U) + threadIdx.x, cv = (unsigned)(C / VE);
    float px[U][J];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned i = i0 + u * 256u;
#pragma unroll
        for (int j = 0; j < J; ++j) px[u][j] = 0.f;
        if (i < nvec) img_load<J>(img + (size_t)(i / cv) * J, px[u]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned i = i0 + u * 256u;
        if (i >= nvec) continue;
        const int c0 = (int)(i % cv) * VE;
        float v[VE];
#pragma unroll
        for (int k = 0; k < VE; ++k) {
            float s = px[u][0] * tw[c0 + k];
#pragma unroll
            for (int j = 1; j < J; ++j) s += px[u][j] * tw[j * C + c0 + k];
            v[k] = tw[J * C + c0 + k] + s;
        }
        VecTraits<T>::store(y + (size_t)i * VE, v);
    }
}
template <typename T, int J>
static void img_in_run(const float* img, const float* w, int sj, int sc, float wscale, const float* bias, T* y, size_t npix, int C, hipStream_t st) {
    constexpr int VE = VecTraits<T>::VE;
    const size_t nvec = npix * (C / VE);
    // The threshold is rgb_in_run's, 65536 vectors.  Measured for this kernel (tools/imgconv_probe.py --sweep, profiles/imgconv_probe.json:
    // bf16, C = 16, J = 4, launches timed alone with events; loop kernel / short-lived blocks, us): 131072 pixels (262144 vectors) 10.5 / 9.4,
    // 262144 px 14.8 / 9.9, 1M px 43.0 / 13.6, 4M px 82.5 / 41.3; at 65536 pixels and below both read 8-9 us, the floor of an event-timed launch,
    // so the probe cannot place the crossover more finely than "at or below 131072 vectors" and the 3-channel kernel's figure stands.
    // C <= 1024 keeps the table at (J + 1) C floats <= 36 KB of LDS.
    const int min1 = img1_min();
    if (min1 > 0 && nvec >= (size_t)min1 && nvec < 0x7fffffffull && C <= 1024)
        hipLaunchKernelGGL((img_in1_kernel<T, J>), dim3((unsigned)((nvec + 1023) / 1024)), dim3(256), (size_t)(J + 1) * C * sizeof(float), st, img, w, sj, sc,
                           wscale, bias, y, (unsigned)nvec, C);
    else
        hipLaunchKernelGGL((img_in_kernel<T, J>), dim3(grid_for_hoisted(nvec, C / VE)), dim3(256), 0, st, img, w, sj, sc, wscale, bias, y, npix, C);
}
static inline bool img_aligned(const void* p, int J) { return (reinterpret_cast<uintptr_t>(p) & (size_t)(4 * (J > 4 ? 4 : J) - 1)) == 0; }

extern "C" int sgx_img_in(const float* img, const float* w, int J, int sj, int sc, float wscale, const float* bias, void* y, size_t npix, int C, int dtype,
                          void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SGX_REQUIRE(img && w && y && npix > 0, SGX_EINVAL, "img_in: null argument");
    SGX_REQUIRE(J == 1 || J == 2 || J == 4 || J == 8, SGX_EUNSUPPORTED, "img_in: J=%d (1, 2, 4 or 8 image channels)", J);
    return sgx_by_dtype(dtype, "img_in", [&](auto t) -> int {
        using T = decltype(t);
        SGX_REQUIRE(C > 0 && C % VecTraits<T>::VE == 0, SGX_EUNSUPPORTED, "img_in: C=%d (whole 16-byte channel vectors)", C);
        SGX_REQUIRE(img_aligned(img, J) && sgx_aligned16(y), SGX_EINVAL, "img_in: misaligned image or output");
        SGX_NOTE(2.0 * J * npix * C, npix * (4.0 * J + sgx_esize(dtype) * C), "img_in J%d %zux%d", J, npix, C);
        sgx_by_int<IMG_JS>(J, [&](auto j) { img_in_run<T, j()>(img, w, sj, sc, wscale, bias, as<T>(y), npix, C, st); });
        SGX_LAUNCH_CHECK("img_in");
        return 0;
    });
}

// ---------------------------------------------------------------- activations -> image: img[p][j] = bias[j] + sum_c x[p][c] (wscale W(j,c))
// One pixel per group of LPP lanes (LPP = C/VE capped at 16, a power of two); partial dot products reduced with shuffles; the J x C weights
// staged once per block in LDS, pre-multiplied by wscale; lane 0 of the group writes the pixel's J values as one store.
template <typename T, int J>
__global__ void img_out_kernel(const T* __restrict__ x, const float* __restrict__ w, int sj, int sc, float wscale, const float* __restrict__ bias,
                               float* __restrict__ img, size_t npix, int C, int lpp) {
    constexpr int VE = VecTraits<T>::VE;
    extern __shared__ float sw[];                            // [J][C]
    for (int i = threadIdx.x; i < J * C; i += blockDim.x) sw[i] = wscale * w[(i / C) * sj + (i % C) * sc];
    __syncthreads();
    float bj[J];
#pragma unroll
    for (int j = 0; j < J; ++j) bj[j] = bias ? bias[j] : 0.f;
    const int cv = C / VE;
    const int sub = threadIdx.x % lpp;
    const size_t gid = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / lpp;
    const size_t gstride = ((size_t)gridDim.x * blockDim.x) / lpp;
    const size_t niter = (npix + gstride - 1) / gstride;
    for (size_t it = 0; it < niter; ++it) {
        const size_t p = gid + it * gstride;
        float s[J];
#pragma unroll
        for (int j = 0; j < J; ++j) s[j] = 0.f;
        if (p < npix) {
            for (int v = sub; v < cv; v += lpp) {
                float t[VE];
                VecTraits<T>::load(x + (p * cv + v) * VE, t);
#pragma unroll
                for (int q = 0; q < VE / 4; ++q) {
                    const int c = v * VE + q * 4;
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        const float4 wj = *reinterpret_cast<const float4*>(sw + j * C + c);
                        s[j] += t[q * 4] * wj.x + t[q * 4 + 1] * wj.y + t[q * 4 + 2] * wj.z + t[q * 4 + 3] * wj.w;
                    }
                }
            }
        }
        for (int o = lpp >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < J; ++j) s[j] += __shfl_xor(s[j], o, 64);
        }
        if (p < npix && sub == 0) {
#pragma unroll
            for (int j = 0; j < J; ++j) s[j] += bj[j];
            img_store<J>(img + p * J, s);
        }
    }
}
// The same with FOUR pixels per lane group and no loop (as rgb_out1_kernel): every lane holds exactly one vector of its pixel (cv == lpp),
// the four loads are requested before the block waits for its weight table.  Same products, same sum order per pixel.
template <typename T, int J>
__global__ __launch_bounds__(256) void img_out1_kernel(const T* __restrict__ x, const float* __restrict__ w, int sj, int sc, float wscale,
                                                       const float* __restrict__ bias, float* __restrict__ img, unsigned npix, int C, int lpp) {
    constexpr int VE = VecTraits<T>::VE, U = 4;
    extern __shared__ float sw[];                            // [J][C]
    const int sub = threadIdx.x % lpp, grp = threadIdx.x / lpp, ppb = 256 / lpp;
    const unsigned p0 = blockIdx.x * (unsigned)(ppb * U) + grp;
    uint4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned p = p0 + u * ppb;
        raw[u] = make_uint4(0u, 0u, 0u, 0u);
        if (p < npix) raw[u] = *reinterpret_cast<const uint4*>(x + ((size_t)p * lpp + sub) * VE);
    }
    for (int i = threadIdx.x; i < J * C; i += 256) sw[i] = wscale * w[(i / C) * sj + (i % C) * sc];
    __syncthreads();
    float bj[J];
#pragma unroll
    for (int j = 0; j < J; ++j) bj[j] = bias ? bias[j] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned p = p0 + u * ppb;
        float s[J];
#pragma unroll
        for (int j = 0; j < J; ++j) s[j] = 0.f;
        if (p < npix) {
            float t[VE];
            const unsigned w4[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { t[(2 * k) % VE] = __uint_as_float(w4[k] << 16); t[(2 * k + 1) % VE] = __uint_as_float(w4[k] & 0xffff0000u); }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) t[k % VE] = __uint_as_float(w4[k]);
            }
#pragma unroll
            for (int q = 0; q < VE / 4; ++q) {
                const int c = sub * VE + q * 4;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const float4 wj = *reinterpret_cast<const float4*>(sw + j * C + c);
                    s[j] += t[q * 4] * wj.x + t[q * 4 + 1] * wj.y + t[q * 4 + 2] * wj.z + t[q * 4 + 3] * wj.w;
                }
            }
        }
        for (int o = lpp >> 1; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < J; ++j) s[j] += __shfl_xor(s[j], o, 64);
        }
        if (p < npix && sub == 0) {
#pragma unroll
            for (int j = 0; j < J; ++j) s[j] += bj[j];
            img_store<J>(img + (size_t)p * J, s);
        }
    }
}
template <typename T, int J>
static void img_out_run(const T* x, const float* w, int sj, int sc, float wscale, const float* bias, float* img, size_t npix, int C, int lpp, hipStream_t st) {
    constexpr int VE = VecTraits<T>::VE;
    const size_t sh = (size_t)J * C * sizeof(float);
    // short-lived blocks where every lane of a pixel group holds exactly one vector (C / VE == lpp <= 16) and the launch is large enough:
    // rgb_out_launch's rule and threshold (65536 pixels), read through the same switch as img_in's.  The same sweep for this kernel (loop /
    // short-lived, us): 262144 px 7.3 / 9.4, 1M px 16.3 / 15.3, 4M px 43.0 / 45.8 -- within the run-to-run spread of a launch timed alone
    // (the interleaved rows of the probe have the short-lived kernel at 38.6 us at 4M px): no case for a different rule than rgb_out's
    const int min1 = img1_min();
    if (min1 > 0 && C / VE == lpp && npix >= (size_t)min1 && npix < 0x7fffffffull) {
        const unsigned ppb4 = (unsigned)(256 / lpp) * 4;
        hipLaunchKernelGGL((img_out1_kernel<T, J>), dim3((unsigned)((npix + ppb4 - 1) / ppb4)), dim3(256), sh, st, x, w, sj, sc, wscale, bias, img, (unsigned)npix, C, lpp);
    } else {
        hipLaunchKernelGGL((img_out_kernel<T, J>), dim3(grid_for(npix * lpp)), dim3(256), sh, st, x, w, sj, sc, wscale, bias, img, npix, C, lpp);
    }
}
extern "C" int sgx_img_out(const void* x, const float* w, int J, int sj, int sc, float wscale, const float* bias, float* img, size_t npix, int C, int dtype,
                           void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SGX_REQUIRE(x && w && img && npix > 0, SGX_EINVAL, "img_out: null argument");
    SGX_REQUIRE(J == 1 || J == 2 || J == 4 || J == 8, SGX_EUNSUPPORTED, "img_out: J=%d (1, 2, 4 or 8 image channels)", J);
    return sgx_by_dtype(dtype, "img_out", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VE = VecTraits<T>::VE;
        SGX_REQUIRE(C > 0 && C % VE == 0 && (long)J * C <= 8192, SGX_EUNSUPPORTED, "img_out: C=%d (whole 16-byte channel vectors, J * C <= 8192: the weights' 32 KB of LDS)", C);
        const int lpp = C / VE > 16 ? 16 : C / VE;
        SGX_REQUIRE((lpp & (lpp - 1)) == 0, SGX_EUNSUPPORTED, "img_out: C=%d (min(vectors per pixel, 16) must be a power of two)", C);
        SGX_REQUIRE(img_aligned(img, J) && sgx_aligned16(x), SGX_EINVAL, "img_out: misaligned image or input");
        SGX_NOTE(2.0 * J * npix * C, npix * (4.0 * J + sgx_esize(dtype) * C), "img_out J%d %zux%d", J, npix, C);
        sgx_by_int<IMG_JS>(J, [&](auto j) { img_out_run<T, j()>(as<T>(x), w, sj, sc, wscale, bias, img, npix, C, lpp, st); });
        SGX_LAUNCH_CHECK("img_out");
        return 0;
    });
}

// ---------------------------------------------------------------- weight gradient: dW(j,c) = wscale sum_p img[p][j] f[p][c]
// Two stages, fixed order (as colsum_vec_stage1 / rgb_wgrad_stage2 of pointwise.hip): a block owns a contiguous range of pixels, a lane
// one 16-byte channel vector of every rows-th pixel of it and sums f * img[j] in fp32 (tens to a few hundred terms), the lanes of a
// block are summed in fp64 in row order, the blocks in fp64 in block order.  No atomics: the same bits at every run.
#define IMG_WGRAD_BLOCKS 1024
template <typename T, int J>
__global__ __launch_bounds__(256) void img_wgrad_stage1(const T* __restrict__ f, const float* __restrict__ img, double* __restrict__ ws, size_t npix, int C) {
    constexpr int VE = VecTraits<T>::VE, PJ = J > 4 ? 4 : J;                 // image channels per finishing pass: [256][PJ * VE + 1] floats <= 33 KB
    // a lane's row of partials, padded to an odd stride: at 32 words every lane of a wave wrote the same LDS bank, and the four blocks of a CU
    // finish together (tools/imgconv_probe.py, batch 4, bf16, J = 4: 1024^2 x 16 55.1 -> 44.9 us, 512^2 x 32 36.4 -> 24.5 us; rgb_wgrad 38.1 / 24.5)
    constexpr int LS = PJ * VE + 1;
    extern __shared__ float shf[];
    const int cv = C / VE, rows = 256 / cv;                                  // cv <= 256; threads past rows * cv idle until the finish
    const int tc = threadIdx.x % cv, tr = threadIdx.x / cv;
    const size_t per = (npix + gridDim.x - 1) / gridDim.x;
    const size_t p0 = (size_t)blockIdx.x * per, p1 = (p0 + per < npix) ? p0 + per : npix;
    float part[J * VE];
#pragma unroll
    for (int k = 0; k < J * VE; ++k) part[k] = 0.f;
    auto accum = [&](const float (&v)[VE], const float (&px)[J]) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int k = 0; k < VE; ++k) part[j * VE + k] += v[k] * px[j];
    };
    if (tr < rows) {
        size_t p = p0 + tr;
        for (; p + 3 * (size_t)rows < p1; p += 4 * (size_t)rows) {           // four rows in flight per lane
            float v0[VE], v1[VE], v2[VE], v3[VE], x0[J], x1[J], x2[J], x3[J];
            VecTraits<T>::load(f + (p * cv + tc) * VE, v0);
            VecTraits<T>::load(f + ((p + rows) * cv + tc) * VE, v1);
            VecTraits<T>::load(f + ((p + 2 * (size_t)rows) * cv + tc) * VE, v2);
            VecTraits<T>::load(f + ((p + 3 * (size_t)rows) * cv + tc) * VE, v3);
            img_load<J>(img + p * J, x0); img_load<J>(img + (p + rows) * J, x1);
            img_load<J>(img + (p + 2 * (size_t)rows) * J, x2); img_load<J>(img + (p + 3 * (size_t)rows) * J, x3);
            accum(v0, x0); accum(v1, x1); accum(v2, x2); accum(v3, x3);
        }
        for (; p < p1; p += rows) {
            float v[VE], px[J];
            VecTraits<T>::load(f + (p * cv + tc) * VE, v);
            img_load<J>(img + p * J, px);
            accum(v, px);
        }
    }
#pragma unroll
    for (int j0 = 0; j0 < J; j0 += PJ) {
#pragma unroll
        for (int k = 0; k < PJ * VE; ++k) shf[threadIdx.x * LS + k] = part[j0 * VE + k];
        __syncthreads();
        for (int o = threadIdx.x; o < cv * PJ * VE; o += 256) {              // output (channel vector, k): sum over the rows
            const int c = o / (PJ * VE), k = o % (PJ * VE);
            double s = 0.0;
            for (int r = 0; r < rows; ++r) s += (double)shf[(r * cv + c) * LS + k];
            ws[((size_t)blockIdx.x * J + j0 + k / VE) * C + c * VE + (k % VE)] = s;
        }
        __syncthreads();
    }
}
// sums the per-block partials [blk][J][C] in block order and scatters into the parameter layout dw[j*sj + c*sc]
__global__ __launch_bounds__(256) void img_wgrad_stage2(const double* __restrict__ ws, float* __restrict__ dw, int nblk, int J, int C, int sj, int sc,
                                                        float wscale) {
    __shared__ double sh[64][5];
    const int el = threadIdx.x & 3, pl = threadIdx.x >> 2;
    const int e = blockIdx.x * 4 + el;                       // e = j*C + c
    double s = 0.0;
    if (e < J * C)
        for (int b = pl; b < nblk; b += 64) s += ws[(size_t)b * J * C + e];
    sh[pl][el] = s;
    __syncthreads();
    if (pl == 0 && e < J * C) {
        double t = 0.0;
        for (int k = 0; k < 64; ++k) t += sh[k][el];
        dw[(e / C) * sj + (e % C) * sc] = (float)(t * (double)wscale);
    }
}
extern "C" size_t sgx_img_wgrad_ws_bytes(size_t npix, int J, int C) {
    (void)npix;
    return (size_t)IMG_WGRAD_BLOCKS * (size_t)(J > 0 ? J : 1) * (size_t)(C > 0 ? C : 1) * sizeof(double);
}
extern "C" int sgx_img_wgrad(const float* img, const void* f, float* dw, int J, int sj, int sc, float wscale, void* ws, size_t ws_bytes, size_t npix, int C,
                             int dtype, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SGX_REQUIRE(img && f && dw && ws && npix > 0, SGX_EINVAL, "img_wgrad: null argument");
    SGX_REQUIRE(J == 1 || J == 2 || J == 4 || J == 8, SGX_EUNSUPPORTED, "img_wgrad: J=%d (1, 2, 4 or 8 image channels)", J);
    return sgx_by_dtype(dtype, "img_wgrad", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VE = VecTraits<T>::VE;
        SGX_REQUIRE(C > 0 && C % VE == 0 && C / VE <= 256, SGX_EUNSUPPORTED, "img_wgrad: C=%d (whole 16-byte channel vectors, at most 256 of them)", C);
        SGX_REQUIRE(ws_bytes >= sgx_img_wgrad_ws_bytes(npix, J, C), SGX_EWORKSPACE, "img_wgrad: workspace");
        SGX_REQUIRE(img_aligned(img, J) && sgx_aligned16(f) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, SGX_EINVAL,
                    "img_wgrad: misaligned image, gradient or workspace");
        SGX_NOTE(2.0 * J * npix * C, npix * (4.0 * J + sgx_esize(dtype) * C), "img_wgrad J%d %zux%d", J, npix, C);
        int nblk = (int)((npix + 63) / 64);
        if (nblk > IMG_WGRAD_BLOCKS) nblk = IMG_WGRAD_BLOCKS;
        if (nblk < 1) nblk = 1;
        const size_t sh = (size_t)256 * ((J > 4 ? 4 : J) * VE + 1) * sizeof(float);
        sgx_by_int<IMG_JS>(J, [&](auto j) {
            hipLaunchKernelGGL((img_wgrad_stage1<T, j()>), dim3(nblk), dim3(256), sh, st, as<T>(f), img, (double*)ws, npix, C);
        });
        SGX_LAUNCH_CHECK("img_wgrad_stage1");
        hipLaunchKernelGGL(img_wgrad_stage2, dim3((J * C + 3) / 4), dim3(256), 0, st, (const double*)ws, dw, nblk, J, C, sj, sc, wscale);
        SGX_LAUNCH_CHECK("img_wgrad_stage2");
        return 0;
    });
}

// ---------------------------------------------------------------- uint8 images with J channels -> normalised NHWC activations
// sgx_images_u8_to_nhwc for J = 1, 2, 3, 4 channels: the same arithmetic in the same order, fp32 with IEEE division, (v / 255 - 0.5) / 0.5
// (/ 0.5 == * 2 exactly), bf16 rounded to nearest even on the store -- at J = 3 bit for bit the existing kernel.  Widths that are a multiple
// of 4: a lane converts 4 consecutive output pixels (J dword loads: 4 J contiguous bytes of an HWC row, or one dword from each plane of a
// CHW image -> 16 J / 8 J contiguous output bytes).  Other widths: one pixel per lane.
__device__ __forceinline__ float u8_norm(unsigned v) { return (__fdiv_rn((float)v, 255.0f) - 0.5f) * 2.0f; }
template <typename T, int J, bool CHW>
__global__ void images_u8_c_kernel(const unsigned char* __restrict__ src, T* __restrict__ dst, const int* __restrict__ flip, int B, int H, int W) {
    const int wq = W / 4;
    const size_t n = (size_t)B * H * wq;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int xq = (int)(i % wq);
        const size_t row = i / wq;
        const int yy = (int)(row % H), b = (int)(row / H);
        const bool fl = flip != nullptr && flip[b] != 0;
        const int sx = fl ? W - 4 - 4 * xq : 4 * xq;                 // first of the 4 source pixels (mirrored block if flipped)
        unsigned v[4][J];                                            // [source pixel][channel]
        if (CHW) {
#pragma unroll
            for (int c = 0; c < J; ++c) {
                const unsigned wd = *reinterpret_cast<const unsigned*>(src + (((size_t)b * J + c) * H + yy) * W + sx);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k][c] = (wd >> (8 * k)) & 0xffu;
            }
        } else {
            const unsigned* s4 = reinterpret_cast<const unsigned*>(src + (((size_t)b * H + yy) * W + sx) * J);
            unsigned wd[J];
#pragma unroll
            for (int q = 0; q < J; ++q) wd[q] = s4[q];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < J; ++c) { const int e = J * k + c; v[k][c] = (wd[e / 4] >> (8 * (e % 4))) & 0xffu; }
        }
        float o[4 * J];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < J; ++c) o[J * k + c] = u8_norm(fl ? v[3 - k][c] : v[k][c]);
        T* d = dst + (((size_t)b * H + yy) * W + 4 * xq) * J;
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int q = 0; q < J; ++q) reinterpret_cast<float4*>(d)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < J; ++q) {
                uint2 t;
                t.x = pack_bf16x2(o[4 * q], o[4 * q + 1]); t.y = pack_bf16x2(o[4 * q + 2], o[4 * q + 3]);
                reinterpret_cast<uint2*>(d)[q] = t;
            }
        }
    }
}
template <typename T, int J, bool CHW>
__global__ void images_u8_c_px_kernel(const unsigned char* __restrict__ src, T* __restrict__ dst, const int* __restrict__ flip, int B, int H, int W) {
    const size_t n = (size_t)B * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int xo = (int)(i % W);
        const size_t row = i / W;
        const int yy = (int)(row % H), b = (int)(row / H);
        const int sx = (flip != nullptr && flip[b] != 0) ? W - 1 - xo : xo;
#pragma unroll
        for (int c = 0; c < J; ++c) {
            const unsigned v = CHW ? src[(((size_t)b * J + c) * H + yy) * W + sx] : src[(((size_t)b * H + yy) * W + sx) * J + c];
            dst[i * J + c] = from_f<T>(u8_norm(v));
        }
    }
}
template <typename T, int J>
static void images_u8_c_run(const unsigned char* s, T* d, const int* flip, int B, int H, int W, int chw, hipStream_t st) {
    if (W % 4 == 0) {
        const unsigned g = grid_for((size_t)B * H * (W / 4));
        if (chw) hipLaunchKernelGGL((images_u8_c_kernel<T, J, true>), dim3(g), dim3(256), 0, st, s, d, flip, B, H, W);
        else hipLaunchKernelGGL((images_u8_c_kernel<T, J, false>), dim3(g), dim3(256), 0, st, s, d, flip, B, H, W);
    } else {
        const unsigned g = grid_for((size_t)B * H * W);
        if (chw) hipLaunchKernelGGL((images_u8_c_px_kernel<T, J, true>), dim3(g), dim3(256), 0, st, s, d, flip, B, H, W);
        else hipLaunchKernelGGL((images_u8_c_px_kernel<T, J, false>), dim3(g), dim3(256), 0, st, s, d, flip, B, H, W);
    }
}
extern "C" int sgx_images_u8_to_nhwc_c(const void* src, void* dst, const int* flip, int B, int H, int W, int J, int src_chw, int dtype, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SGX_REQUIRE(src && dst && B > 0 && H > 0 && W > 0, SGX_EINVAL, "images_u8_to_nhwc_c: bad arguments (B%d %dx%d)", B, H, W);
    SGX_REQUIRE(J >= 1 && J <= 4, SGX_EUNSUPPORTED, "images_u8_to_nhwc_c: J=%d (1 to 4 channels)", J);
    return sgx_by_dtype(dtype, "images_u8_to_nhwc_c", [&](auto t) -> int {
        using T = decltype(t);
        SGX_REQUIRE(W % 4 != 0 || ((reinterpret_cast<uintptr_t>(src) & 3) == 0 && sgx_aligned16(dst)), SGX_EINVAL,
                    "images_u8_to_nhwc_c: misaligned source or output");
        SGX_NOTE(0.0, (1.0 + sgx_esize(dtype)) * J * B * H * W, "images_u8 J%d B%d %dx%d", J, B, H, W);
        const auto* s = static_cast<const unsigned char*>(src);
        sgx_by_int<IMG_U8_JS>(J, [&](auto j) { images_u8_c_run<T, j()>(s, as<T>(dst), flip, B, H, W, src_chw, st); });
        SGX_LAUNCH_CHECK("images_u8_c_kernel");
        return 0;
    });
}
