// Small fp32 pieces: PixelNorm rows, minibatch-stddev (forward / backward / second-order backward for R1),
// and the MFMA fp32 GEMM behind EqualizedLinear (mapping network, style affine maps, discriminator head).
// Launch layer: an entry point checks its arguments, decides once -- mbstd_run (grid, dtype -> T through sgx_by_dtype), style_mb (batch -> MB
// through sgx_by_int), gemm_plan (kernel, splits, grids, vec: what sgx_gemm_plan reports without launching) -- and every kernel has one
// hipLaunchKernelGGL site, spelled with the parameter (T, MB, U) where the decision is a template argument.
#include "common.h"

// ---------------------------------------------------------------- PixelNorm over the feature dim of [B][C]
__global__ void pixelnorm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int C) {
    const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (row >= B) return;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) { const float v = x[(size_t)row * C + c]; ss += v * v; }
    ss = wave_sum(ss);
    const float r = rsqrtf(ss / C + 1e-8f);
    for (int c = lane; c < C; c += 64) y[(size_t)row * C + c] = x[(size_t)row * C + c] * r;
}
__global__ void pixelnorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int B, int C) {
    const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
    if (row >= B) return;
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = x[(size_t)row * C + c];
        ss += v * v; dot += v * dy[(size_t)row * C + c];
    }
    ss = wave_sum(ss); dot = wave_sum(dot);
    const float r = rsqrtf(ss / C + 1e-8f);
    const float k = r * r * r * dot / C;
    for (int c = lane; c < C; c += 64) dx[(size_t)row * C + c] = dy[(size_t)row * C + c] * r - x[(size_t)row * C + c] * k;
}
extern "C" int sgx_pixelnorm_fwd(const float* x, float* y, int B, int C, void* stream) {
    hipLaunchKernelGGL(pixelnorm_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, y, B, C);
    SGX_LAUNCH_CHECK("pixelnorm_fwd");
    return 0;
}
extern "C" int sgx_pixelnorm_bwd(const float* dy, const float* x, float* dx, int B, int C, void* stream) {
    hipLaunchKernelGGL(pixelnorm_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, dy, x, dx, B, C);
    SGX_LAUNCH_CHECK("pixelnorm_bwd");
    return 0;
}

// ---------------------------------------------------------------- minibatch stddev
// x [B][HW][C], y/dy [B][HW][Cpad].  Group g, slot m: sample g*M+m.  One block per slot m.
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
    return s;
}

// The kernels below touch 64 KB at batch 4 (4x4 pixels, 512 channels): their time is the number of dependent memory round trips a
// thread makes, not bytes.  Every loop therefore fetches all it needs for MBSTD_U elements (all G group members of each) before the
// first use, at clamped addresses where an element or a group member does not exist, and the padded copies fetch the G images of a
// position together instead of one image after the other.  The sums run in the order they always did (per thread over i ascending,
// then block_sum_d), so every result is bit for bit what the one-load-at-a-time loops gave.
#define MBSTD_U 8
// the group's members g < G (G <= 4), unrolled: a loop to the runtime G would index the per-member register arrays dynamically (scratch)
#define MBSTD_FOR_G(g) _Pragma("unroll") for (int g = 0; g < 4; ++g) if (g < G)
// sqrt(var + eps) of the G values v (the group's standard deviation at one position and channel); mu is returned too
__device__ __forceinline__ float mbstd_std(const float (&v)[4], int G, float& mu) {
    mu = 0.f;
    MBSTD_FOR_G(g) mu += v[g];
    mu /= G;
    float var = 0.f;
    MBSTD_FOR_G(g) { const float d = v[g] - mu; var += d * d; }
    return sqrtf(var / G + 1e-8f);
}
// sum over the slot's G images and HW positions of the statistic channel of dy (per thread, before block_sum_d)
template <typename T>
__device__ __forceinline__ double mbstd_gy_partial(const T* __restrict__ dy, int G, int M, int m, int HW, int C, int Cpad) {
    double acc = 0.0;
    for (int i0 = threadIdx.x; i0 < G * HW; i0 += MBSTD_U * blockDim.x) {
        float t[MBSTD_U];
#pragma unroll
        for (int u = 0; u < MBSTD_U; ++u) {
            const int i = i0 + u * blockDim.x, ii = i < G * HW ? i : G * HW - 1, g = ii / HW, p = ii % HW;
            t[u] = to_f(dy[((size_t)(g * M + m) * HW + p) * Cpad + C]);
        }
#pragma unroll
        for (int u = 0; u < MBSTD_U; ++u)
            if (i0 + u * (int)blockDim.x < G * HW) acc += (double)t[u];
    }
    return acc;
}
// y[b][p][0..Cpad) = (src[b][p][0..C), stat, 0...) for the slot's G images: this block's share of the positions
template <typename T>
__device__ __forceinline__ void mbstd_padded_copy(const T* __restrict__ src, T* __restrict__ y, float stat, int G, int M, int m, int HW,
                                                  int C, int Cpad) {
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < HW * Cpad; i += gridDim.y * blockDim.x) {
        const int p = i / Cpad, c = i % Cpad, cc = c < C ? c : C - 1;
        T v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) v[g] = src[((size_t)((g < G ? g : 0) * M + m) * HW + p) * C + cc];
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g < G) y[((size_t)(g * M + m) * HW + p) * Cpad + c] = c < C ? from_f<T>(to_f(v[g])) : from_f<T>(c == C ? stat : 0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void mbstd_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int HW, int C, int Cpad) {
    __shared__ double sh[16];
    const int G = B < 4 ? B : 4, M = B / G, m = blockIdx.x, n = HW * C;
    double acc = 0.0;
    for (int i0 = threadIdx.x; i0 < n; i0 += MBSTD_U * blockDim.x) {
        float v[MBSTD_U][4];
#pragma unroll
        for (int u = 0; u < MBSTD_U; ++u) {
            const int i = i0 + u * blockDim.x, ii = i < n ? i : n - 1;
#pragma unroll
            for (int g = 0; g < 4; ++g) v[u][g] = to_f(x[(size_t)((g < G ? g : 0) * M + m) * n + ii]);
        }
#pragma unroll
        for (int u = 0; u < MBSTD_U; ++u)
            if (i0 + u * (int)blockDim.x < n) { float mu; acc += (double)mbstd_std(v[u], G, mu); }
    }
    const float stat = (float)(block_sum_d(acc, sh) / n);
    // every block of the slot computed the statistic (redundantly: it is a 32-KB reduction); the padded copy is split over them
    mbstd_padded_copy(x, y, stat, G, M, m, HW, C, Cpad);
}

template <typename T>
__global__ __launch_bounds__(1024) void mbstd_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, T* __restrict__ dx, int B,
                                                        int HW, int C, int Cpad) {
    __shared__ double sh[16];
    const int G = B < 4 ? B : 4, M = B / G, m = blockIdx.x, n = HW * C;
    const double acc = mbstd_gy_partial(dy, G, M, m, HW, C, Cpad);
    const float k = (float)(block_sum_d(acc, sh) / n) / G;              // gy / (C*HW*G)
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += gridDim.y * blockDim.x) {
        const int p = i / C, c = i % C;
        float v[4], d[4], mu;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const size_t b = (size_t)((g < G ? g : 0) * M + m);
            v[g] = to_f(x[b * n + i]);
            d[g] = to_f(dy[(b * HW + p) * Cpad + c]);
        }
        const float s = mbstd_std(v, G, mu);
#pragma unroll
        for (int g = 0; g < 4; ++g)
            if (g < G) dx[(size_t)(g * M + m) * n + i] = from_f<T>(d[g] + k * (v[g] - mu) / s);
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void mbstd_bwd2_kernel(const T* __restrict__ ggx, const T* __restrict__ dy, const T* __restrict__ x,
                                                         T* __restrict__ ddy, T* __restrict__ gx, int B, int HW, int C, int Cpad) {
    __shared__ double sh[16];
    const int G = B < 4 ? B : 4, M = B / G, m = blockIdx.x, n = HW * C;
    const double a_gy = mbstd_gy_partial(dy, G, M, m, HW, C, Cpad);
    double a_dd = 0.0;
    for (int i0 = threadIdx.x; i0 < n; i0 += MBSTD_U * blockDim.x) {
        float v[MBSTD_U][4], gg[MBSTD_U][4];
#pragma unroll
        for (int u = 0; u < MBSTD_U; ++u) {
            const int i = i0 + u * blockDim.x, ii = i < n ? i : n - 1;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const size_t o = (size_t)((g < G ? g : 0) * M + m) * n + ii;
                v[u][g] = to_f(x[o]); gg[u][g] = to_f(ggx[o]);
            }
        }
#pragma unroll
        for (int u = 0; u < MBSTD_U; ++u)
            if (i0 + u * (int)blockDim.x < n) {
                float mu = 0.f;
                MBSTD_FOR_G(g) mu += v[u][g];
                mu /= G;
                float var = 0.f, dot = 0.f;
                MBSTD_FOR_G(g) {
                    const float d = v[u][g] - mu;
                    var += d * d;
                    dot += d * gg[u][g];
                }
                a_dd += (double)(dot / sqrtf(var / G + 1e-8f));
            }
    }
    const float k = (float)(block_sum_d(a_gy, sh) / n) / G;             // gy / (C*HW*G)
    const float dstat = (float)(block_sum_d(a_dd, sh) / n) / G;         // d L / d gy[m]
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += gridDim.y * blockDim.x) {
        float v[4], gg[4], mu = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const size_t o = (size_t)((g < G ? g : 0) * M + m) * n + i;
            v[g] = to_f(x[o]); gg[g] = to_f(ggx[o]);
        }
        MBSTD_FOR_G(g) mu += v[g];
        mu /= G;
        float var = 0.f, dot = 0.f;
        MBSTD_FOR_G(g) { const float d = v[g] - mu; var += d * d; dot += d * gg[g]; }
        const float s = sqrtf(var / G + 1e-8f);
        float u[4], um = 0.f;
        MBSTD_FOR_G(g) { u[g] = gg[g] / s - dot * (v[g] - mu) / (G * s * s * s); um += u[g]; }
        um /= G;
        MBSTD_FOR_G(g) gx[(size_t)(g * M + m) * n + i] = from_f<T>(k * (u[g] - um));
    }
    mbstd_padded_copy(ggx, ddy, dstat, G, M, m, HW, C, Cpad);
}

#ifndef MBSTD_NB
#define MBSTD_NB 8                                             // blocks per slot: each recomputes the scalars, writes 1/8 of the output
#endif
static int mbstd_check(int B, int C, int Cpad) {
    SGX_REQUIRE(B > 0 && (B < 4 || B % 4 == 0), SGX_EINVAL, "mbstd: batch %d not divisible by group size", B);
    SGX_REQUIRE(Cpad > C, SGX_EINVAL, "mbstd: Cpad must exceed C");
    return 0;
}
// The three entry points: the shape check, the (M, MBSTD_NB) grid and dtype -> T, once; f(T{}, grid, stream) holds the kernel's launch site
template <typename F> static int mbstd_run(const char* name, int B, int C, int Cpad, int dtype, void* stream, F f) {
    int rc = mbstd_check(B, C, Cpad); if (rc) return rc;
    return sgx_by_dtype(dtype, name, [&](auto t) -> int {
        f(t, dim3(B / (B < 4 ? B : 4), MBSTD_NB), (hipStream_t)stream);
        SGX_LAUNCH_CHECK(name);
        return 0;
    });
}
extern "C" int sgx_mbstd_fwd(const void* x, void* y, int B, int HW, int C, int Cpad, int dtype, void* stream) {
    return mbstd_run("mbstd_fwd", B, C, Cpad, dtype, stream, [&](auto t, dim3 grid, hipStream_t st) {
        using T = decltype(t);
        hipLaunchKernelGGL(mbstd_fwd_kernel<T>, grid, dim3(1024), 0, st, as<T>(x), as<T>(y), B, HW, C, Cpad);
    });
}
extern "C" int sgx_mbstd_bwd(const void* dy, const void* x, void* dx, int B, int HW, int C, int Cpad, int dtype, void* stream) {
    return mbstd_run("mbstd_bwd", B, C, Cpad, dtype, stream, [&](auto t, dim3 grid, hipStream_t st) {
        using T = decltype(t);
        hipLaunchKernelGGL(mbstd_bwd_kernel<T>, grid, dim3(1024), 0, st, as<T>(dy), as<T>(x), as<T>(dx), B, HW, C, Cpad);
    });
}
extern "C" int sgx_mbstd_bwd2(const void* ggx, const void* dy, const void* x, void* ddy, void* gx, int B, int HW, int C, int Cpad,
                              int dtype, void* stream) {
    return mbstd_run("mbstd_bwd2", B, C, Cpad, dtype, stream, [&](auto t, dim3 grid, hipStream_t st) {
        using T = decltype(t);
        hipLaunchKernelGGL(mbstd_bwd2_kernel<T>, grid, dim3(1024), 0, st, as<T>(ggx), as<T>(dy), as<T>(x), as<T>(ddy), as<T>(gx), B, HW, C, Cpad);
    });
}

// ---------------------------------------------------------------- fp32 GEMM on v_mfma_f32_16x16x4_f32
// C[M][N] = alpha * op(A)[M][K] * op(B)[K][N].  One 16x16 output tile per block; the block's 4 waves split K and
// reduce through LDS (fixed order: deterministic).  Operand fragments are read straight from global memory: these
// GEMMs have M = batch (4..64) and are weight-bandwidth/latency bound.
// Optional fusions for the EqualizedLinear layers (mapping network, style affines):
//   amask  : A is read as A * slope(amask) (same layout as A) -- the LeakyReLU backward folded into the operand load
//   bias   : C = act(alpha * A B + bscale * bias[column])      -- bias and LeakyReLU folded into the store
//   colsum : colsum[row of C] = cscale * sum_k A'[row][k]      -- with A = gy^T this is the bias gradient, out of the
//            same launch as the weight gradient (written by the blocks of column tile 0)
//   vec    : set by gemm_launch (from gemm_plan), not by the entry points: bit 0 = A (and amask) are 16-byte aligned, bit 1 = B is.  The 16-byte operand
//            loads below are taken only then; a pointer 4 bytes off gets the scalar loads of the same k, hence the same bits
struct GemmFuse { const float* amask; const float* bias; float bscale; int act; float* colsum; float cscale; unsigned vec; };
// One 16-k step of a lane: its four operand values a4 (row ic of op(A), k = kk..kk+3) and b4 (column jc of op(B)).  No branch depends
// on the lane: rows / columns beyond the matrix are read at the clamped index ic / jc (their products land in output rows / columns
// that are never stored), and in the K tail (TAIL) a k beyond ke is read at ke - 1 and replaced by zero.  That lets the compiler issue
// the loads of several steps back to back; with a branch per element every load waited for the one before it (8 - 17 dependent
// round trips per wave at K = 512: the t00 shapes took 13.5 us, the K = 4 outer product 20.7).
template <bool VA, bool VB, bool MASK, bool TAIL>
__device__ __forceinline__ void gemm_step_load(const float* __restrict__ A, const float* __restrict__ am, const float* __restrict__ Bm,
                                               size_t arow, size_t sa_k, size_t bcol, size_t sb_k, int kk, int ke, float (&a4)[4],
                                               float (&b4)[4]) {
    if (VA && !TAIL) {
        const float4 t = *reinterpret_cast<const float4*>(A + arow + kk);
        a4[0] = t.x; a4[1] = t.y; a4[2] = t.z; a4[3] = t.w;
        if (MASK) {
            const float4 m = *reinterpret_cast<const float4*>(am + arow + kk);
            a4[0] *= lrelu_slope(m.x); a4[1] *= lrelu_slope(m.y); a4[2] *= lrelu_slope(m.z); a4[3] *= lrelu_slope(m.w);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kc = (TAIL && kk + s >= ke) ? ke - 1 : kk + s;
            const size_t o = arow + kc * sa_k;
            float v = A[o];
            if (MASK) v *= lrelu_slope(am[o]);
            a4[s] = (TAIL && kk + s >= ke) ? 0.f : v;
        }
    }
    if (VB && !TAIL) {
        const float4 t = *reinterpret_cast<const float4*>(Bm + bcol + kk);
        b4[0] = t.x; b4[1] = t.y; b4[2] = t.z; b4[3] = t.w;
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kc = (TAIL && kk + s >= ke) ? ke - 1 : kk + s;
            const float v = Bm[kc * sb_k + bcol];
            b4[s] = (TAIL && kk + s >= ke) ? 0.f : v;
        }
    }
}
// U = 16-k steps whose loads are in flight together
template <int U, bool VA, bool VB, bool MASK>
__device__ __forceinline__ f32x4 gemm_wave_slice(const float* __restrict__ A, const float* __restrict__ am, const float* __restrict__ Bm,
                                                 size_t arow, size_t sa_k, size_t bcol, size_t sb_k, int kb, int ke, int q) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int k = kb;
    for (; k + 16 * U <= ke; k += 16 * U) {
        float a[U][4], b[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) gemm_step_load<VA, VB, MASK, false>(A, am, Bm, arow, sa_k, bcol, sb_k, k + 16 * u + 4 * q, ke, a[u], b[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], b[u][s], acc, 0, 0, 0);
    }
    for (; k + 16 <= ke; k += 16) {
        float a[4], b[4];
        gemm_step_load<VA, VB, MASK, false>(A, am, Bm, arow, sa_k, bcol, sb_k, k + 4 * q, ke, a, b);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
    if (k < ke) {                                              // K tail of the slice: fewer than 16 k left
        float a[4], b[4];
        gemm_step_load<VA, VB, MASK, true>(A, am, Bm, arow, sa_k, bcol, sb_k, k + 4 * q, ke, a, b);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
    return acc;
}
template <int U>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, const float* __restrict__ Bm, float* __restrict__ Cm,
                                                       int M, int N, int K, int ta, int tb, float alpha, GemmFuse fu) {
    __shared__ float red[4][16][17];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
    const int ic = i0 + l15 < M ? i0 + l15 : M - 1, jc = j0 + l15 < N ? j0 + l15 : N - 1;
    // split K: blockIdx.z owns [z*kz, (z+1)*kz) (partials go to Cm + z*M*N, summed by gemm_splitk_reduce), its 4 waves
    // split that range again
    const int kz = ((K + (int)gridDim.z - 1) / (int)gridDim.z + 15) / 16 * 16;
    const int kz0 = blockIdx.z * kz, kz1 = (kz0 + kz < K) ? kz0 + kz : K;
    const int kper = (((kz1 > kz0 ? kz1 - kz0 : 0) + 3) / 4 + 15) / 16 * 16;   // K slice per wave, multiple of 16
    const int kb = kz0 + wave * kper, ke = (kb + kper < kz1) ? kb + kper : kz1;
    Cm += (size_t)blockIdx.z * M * N;
    const size_t sa_i = ta ? 1 : (size_t)K, sa_k = ta ? (size_t)M : 1;
    const size_t sb_k = tb ? 1 : (size_t)N, sb_j = tb ? (size_t)K : 1;
    const size_t arow = ic * sa_i, bcol = jc * sb_j;
    // 16 k per step: lane group q owns k = k0+4q..+3 (any k order is valid as long as A and B agree), so an
    // operand whose k axis is contiguous is fetched with one 16-byte load per lane instead of four 4-byte ones.
    const bool va = !ta && (K % 4 == 0) && (fu.vec & 1), vb = tb && (K % 4 == 0) && (fu.vec & 2);
    f32x4 acc;
#define GEMM_SLICE(VA, VB, MK) acc = gemm_wave_slice<U, VA, VB, MK>(A, fu.amask, Bm, arow, sa_k, bcol, sb_k, kb, ke, q)
    if (fu.amask) {
        if (va) { if (vb) GEMM_SLICE(true, true, true); else GEMM_SLICE(true, false, true); }
        else    { if (vb) GEMM_SLICE(false, true, true); else GEMM_SLICE(false, false, true); }
    } else {
        if (va) { if (vb) GEMM_SLICE(true, true, false); else GEMM_SLICE(true, false, false); }
        else    { if (vb) GEMM_SLICE(false, true, false); else GEMM_SLICE(false, false, false); }
    }
#undef GEMM_SLICE
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][q * 4 + r][l15] = acc[r];
    __syncthreads();
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
    if (threadIdx.x < 256 && i0 + r < M && j0 + c < N) {
        const float s = ((red[0][r][c] + red[1][r][c]) + red[2][r][c]) + red[3][r][c];
        float v = alpha * s;
        if (fu.bias) v += fu.bscale * fu.bias[j0 + c];
        if (fu.act == SGX_ACT_LRELU) v = lrelu(v);
        Cm[(size_t)(i0 + r) * N + j0 + c] = v;
    }
    if (fu.colsum && blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x < 16 && i0 + (int)threadIdx.x < M) {
        const int row = i0 + threadIdx.x;                     // sum over the whole K axis of row `row` of op(A) (masked)
        float t = 0.f;
        int k = 0;
        for (; k + 8 <= K; k += 8) {                           // 8 (x2) loads in flight, summed in k order
            float v[8], m[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t o = row * sa_i + (k + u) * sa_k;
                v[u] = A[o];
                m[u] = fu.amask ? fu.amask[o] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) t += fu.amask ? v[u] * lrelu_slope(m[u]) : v[u];
        }
        for (; k < K; ++k) {
            const size_t o = row * sa_i + k * sa_k;
            t += fu.amask ? A[o] * lrelu_slope(fu.amask[o]) : A[o];
        }
        fu.colsum[row] = fu.cscale * t;
    }
}
// K <= 4 with B row-major (tb = 0) is an outer product, not a GEMM: C = alpha * sum_k A[:, k] B[k, :] is M * N stores and next to
// no reads (batch 4: dW[512][8192] = gy^T x of the discriminator's dense layer, 16 MB written from 130 KB).  A 16x16 tile per block
// makes that 16384 four-wave blocks of one MFMA step, an LDS round trip and 4-byte stores (20.7 us); here a lane owns four
// consecutive columns and makes one 16-byte store.  The sum is formed the way the MFMA forms it for these shapes, a chain of fused
// multiply-adds in k order from zero, so the result is bit for bit the tile kernel's (tools/small_probe.py compares the two builds).
__global__ __launch_bounds__(256) void gemm_outer_kernel(const float* __restrict__ A, const float* __restrict__ Bm, float* __restrict__ Cm,
                                                         int M, int N, int K, size_t sa_i, size_t sa_k, float alpha) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, n4 = (size_t)N / 4;
    if (idx >= (size_t)M * n4) return;
    const size_t i = idx / n4, j = (idx % n4) * 4;
    float a[4];
    float4 b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kc = k < K ? k : 0;
        a[k] = A[i * sa_i + kc * sa_k];
        b[k] = *reinterpret_cast<const float4*>(Bm + (size_t)kc * N + j);
    }
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < K) {
            acc.x = fmaf(a[k], b[k].x, acc.x); acc.y = fmaf(a[k], b[k].y, acc.y); acc.z = fmaf(a[k], b[k].z, acc.z); acc.w = fmaf(a[k], b[k].w, acc.w);
        }
    acc.x *= alpha; acc.y *= alpha; acc.z *= alpha; acc.w *= alpha;
    *reinterpret_cast<float4*>(Cm + i * N + j) = acc;
}
__global__ void gemm_splitk_reduce(const float* __restrict__ part, float* __restrict__ Cm, int MN, int splits, float alpha) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MN) return;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[(size_t)z * MN + i];     // fixed order: deterministic
    Cm[i] = alpha * s;
}
// Skinny problems (M = batch: few 16x16 output tiles) with a long K are split over blockIdx.z so that the weight
// matrix is streamed by many CUs instead of a handful.
static int gemm_splits(int M, int N, int K) {
    const int tiles = ((M + 15) / 16) * ((N + 15) / 16);
    if (tiles >= 256 || K < 1024) return 1;
    int s = K / 256, cap = (512 + tiles - 1) / tiles;
    if (s > cap) s = cap;
    return s < 1 ? 1 : s;
}
extern "C" size_t sgx_gemm_ws_bytes(int M, int N, int K) {
    const int s = gemm_splits(M, N, K);
    return s > 1 ? (size_t)s * M * N * sizeof(float) : 0;
}
// Everything one GEMM call will do: the ints of sgx_gemm_plan (include/sgx.h) in its order.  unroll: 0 = gemm_outer_kernel, else U of
// gemm_f32_kernel<U>, 1 or 8 (reported as kind 1 / 2); (gx, gy, gz): that kernel's grid; reduce_gx: gemm_splitk_reduce's, 0 when unsplit.
//   fuse  : bit 0 = amask given, bit 1 = bias, activation or colsum given (those are not carried through a split)
//   align : bit 0 = A and amask 16-byte aligned, bit 1 = B, bit 2 = C;  ws_bytes: what the caller holds, 0 for a NULL workspace
struct GemmPlan { int unroll, splits, gx, gy, gz, reduce_gx, vec; };
static GemmPlan gemm_plan(int M, int N, int K, int ta, int tb, int fuse, size_t ws_bytes, int align) {
    if (K <= 4 && !tb && N % 4 == 0 && !fuse && (align & 6) == 6) return GemmPlan{0, 1, (int)(((size_t)M * (N / 4) + 255) / 256), 1, 1, 0, 0};
    int splits = gemm_splits(M, N, K);
    if (splits > 1 && (ws_bytes < (size_t)splits * M * N * sizeof(float) || (fuse & 2))) splits = 1;
    // A wave's K slice of 128 or more (K = 512 unsplit, every split-K launch) runs with the loads of 8 steps in flight: 106 registers.
    // Shorter slices never enter that loop, and their launches are many small blocks (K = 8: 1024 of them) that want the
    // 8 blocks per CU a small register file allows, so they get the instantiation without the unrolled loop.
    const int unroll = (K + splits - 1) / splits >= 512 ? 8 : 1;
    return GemmPlan{unroll, splits, (N + 15) / 16, (M + 15) / 16, splits, splits > 1 ? (M * N + 255) / 256 : 0, align & 3};
}
extern "C" int sgx_gemm_plan(int M, int N, int K, int ta, int tb, int fuse, size_t ws_bytes, int align, int* out) {
    SGX_REQUIRE(M > 0 && N > 0 && K > 0, SGX_EINVAL, "gemm: bad shape %d %d %d", M, N, K);
    SGX_REQUIRE(out, SGX_EINVAL, "gemm_plan: out is NULL");
    const GemmPlan p = gemm_plan(M, N, K, ta, tb, fuse, ws_bytes, align);
    const int v[SGX_GEMM_PLAN_INTS] = {p.unroll == 8 ? 2 : p.unroll, p.splits, p.gx, p.gy, p.gz, p.reduce_gx, p.vec};
    for (int i = 0; i < SGX_GEMM_PLAN_INTS; ++i) out[i] = v[i];
    return 0;
}
static int gemm_launch(const float* A, const float* Bm, float* C, int M, int N, int K, int ta, int tb, float alpha, GemmFuse fu, void* ws,
                       size_t ws_bytes, hipStream_t st) {
    SGX_REQUIRE(M > 0 && N > 0 && K > 0, SGX_EINVAL, "gemm: bad shape %d %d %d", M, N, K);
    const GemmPlan p = gemm_plan(M, N, K, ta, tb, (fu.amask ? 1 : 0) | (fu.bias || fu.act || fu.colsum ? 2 : 0), ws ? ws_bytes : 0,
                                 (sgx_aligned16(A) && sgx_aligned16(fu.amask) ? 1 : 0) | (sgx_aligned16(Bm) ? 2 : 0) | (sgx_aligned16(C) ? 4 : 0));
    SGX_NOTE(2.0 * M * N * K, 4.0 * ((double)M * K + (double)K * N + (double)M * N), "gemm %dx%dx%d t%d%d%s", M, N, K, ta, tb,
             fu.amask || fu.bias || fu.colsum ? " fused" : "");
    const dim3 grid(p.gx, p.gy, p.gz);
    if (!p.unroll) {
        hipLaunchKernelGGL(gemm_outer_kernel, grid, dim3(256), 0, st, A, Bm, C, M, N, K, ta ? (size_t)1 : (size_t)K, ta ? (size_t)M : (size_t)1, alpha);
        SGX_LAUNCH_CHECK("gemm_outer");
        return 0;
    }
    fu.vec = p.vec;
    const bool split = p.splits > 1;                           // the partials go to the workspace unscaled: alpha is the reduce's
    sgx_by_int<1, 8>(p.unroll, [&](auto u) {
        constexpr int U = u();
        hipLaunchKernelGGL(gemm_f32_kernel<U>, grid, dim3(256), 0, st, A, Bm, split ? (float*)ws : C, M, N, K, ta, tb, split ? 1.0f : alpha, fu);
    });
    SGX_LAUNCH_CHECK("gemm_f32");
    if (split) {
        hipLaunchKernelGGL(gemm_splitk_reduce, dim3(p.reduce_gx), dim3(256), 0, st, (const float*)ws, C, M * N, p.splits, alpha);
        SGX_LAUNCH_CHECK("gemm_splitk_reduce");
    }
    return 0;
}
extern "C" int sgx_gemm_f32(const float* A, const float* Bm, float* C, int M, int N, int K, int ta, int tb, float alpha, void* ws,
                            size_t ws_bytes, void* stream) {
    return gemm_launch(A, Bm, C, M, N, K, ta, tb, alpha, GemmFuse{nullptr, nullptr, 0.f, SGX_ACT_NONE, nullptr, 0.f}, ws, ws_bytes,
                       (hipStream_t)stream);
}
// EqualizedLinear (models/CustomLayers.py:64-103) as three launches instead of nine:
//   forward : y[B][N] = act(w_mul * x[B][K] W[N][K]^T + b_mul * bias)
//   backward: gz = gy * slope(y) (if act) folded into the operand loads of both
//             gx[B][K] = w_mul * gz W        and        dW[N][K] = w_mul * gz^T x,  db[N] = b_mul * sum_b gz
extern "C" int sgx_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int N, int K, float w_mul, float b_mul,
                              int act, void* stream) {
    return gemm_launch(x, w, y, B, N, K, 0, 1, w_mul, GemmFuse{nullptr, bias, b_mul, act, nullptr, 0.f}, nullptr, 0, (hipStream_t)stream);
}
extern "C" int sgx_linear_bwd_data(const float* gy, const float* y_act, const float* w, float* gx, int B, int N, int K, float w_mul,
                                   void* stream) {
    return gemm_launch(gy, w, gx, B, K, N, 0, 0, w_mul, GemmFuse{y_act, nullptr, 0.f, SGX_ACT_NONE, nullptr, 0.f}, nullptr, 0,
                       (hipStream_t)stream);
}
extern "C" int sgx_linear_bwd_param(const float* gy, const float* y_act, const float* x, float* dw, float* db, int B, int N, int K,
                                    float w_mul, float b_mul, void* stream) {
    return gemm_launch(gy, x, dw, N, K, B, 1, 0, w_mul, GemmFuse{y_act, nullptr, 0.f, SGX_ACT_NONE, db, b_mul}, nullptr, 0,
                       (hipStream_t)stream);
}

// ---------------------------------------------------------------- all style affines of a generator forward in one launch
// StyleMod.lin (models/CustomLayers.py:203-216) of every active layer: y_g[B][N_g] = w_mul_g * x_g[B][D] W_g[N_g][D]^T +
// b_mul_g * bias_g, with x_g = lm[layer_g] (the layer-major dlatents [L][B][D]).  18 small GEMMs (M = batch) are latency, not
// work: one launch forward, two backward.  tab: G rows of SGX_STYLE_ROW 64-bit words
//   [W, bias, N, y offset (elements, = B * sum of earlier N), first tile, w_mul bits, b_mul bits, layer]
#define STYLE_MAXB 32
// group of a tile: the last row whose first tile is <= tile.  Lane g reads row g's first tile and one ballot counts the rows that
// qualify (first tiles ascend), where a walk over the rows made up to G dependent reads before the block's first weight load.
__device__ __forceinline__ int style_group(const long long* __restrict__ tab, int G, unsigned tile) {
    if (G <= 64) {
        const int l = threadIdx.x & 63;
        const bool le = l < G && (unsigned)tab[(l < G ? l : 0) * SGX_STYLE_ROW + 4] <= tile;
        return __builtin_amdgcn_readfirstlane(__popcll(__ballot(le)) - 1);
    }
    int g = 0;
    while (g + 1 < G && (unsigned)tab[(g + 1) * SGX_STYLE_ROW + 4] <= tile) ++g;
    return g;
}
// block: 16 output columns x 16 k-lanes; x_g staged in LDS
template <int MB>
__global__ __launch_bounds__(256) void style_fwd_kernel(const float* __restrict__ lm, const long long* __restrict__ tab, float* __restrict__ y,
                                                        int G, int B, int D) {
    extern __shared__ float xs[];                                  // [B][D]
    const int g = style_group(tab, G, blockIdx.x);
    const long long* r = tab + (size_t)g * SGX_STYLE_ROW;
    const float* W = reinterpret_cast<const float*>(r[0]);
    const float* bias = reinterpret_cast<const float*>(r[1]);
    const int N = (int)r[2], layer = (int)r[7];
    const float w_mul = __uint_as_float((unsigned)r[5]), b_mul = __uint_as_float((unsigned)r[6]);
    const float* x = lm + (size_t)layer * B * D;
    const int col = threadIdx.x >> 4, kl = threadIdx.x & 15;
    const int n = ((int)blockIdx.x - (int)r[4]) * 16 + col;
    // A lane's share of weight row n is D / 64 16-byte pieces (8 at D = 512).  STYLE_U of them are requested before the first is
    // used -- the first STYLE_U before x is staged, so the weight stream starts with the block -- and consumed in k order: the
    // sums are the ones the one-load-per-iteration loop formed (that loop was D / 64 dependent round trips to memory: 19 us).
    constexpr int STYLE_U = 8;
    const float* wrow = W + (size_t)(n < N ? n : N - 1) * D;
    float4 w[STYLE_U];
#pragma unroll
    for (int u = 0; u < STYLE_U; ++u) { const int k = kl * 4 + 64 * u; w[u] = *reinterpret_cast<const float4*>(wrow + (k < D ? k : D - 4)); }
    for (int i = threadIdx.x; i < B * D / 4; i += 256) reinterpret_cast<float4*>(xs)[i] = reinterpret_cast<const float4*>(x)[i];
    __syncthreads();
    float acc[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[b] = 0.f;
    for (int k0 = kl * 4; k0 < D; k0 += 64 * STYLE_U) {
        if (k0 != kl * 4) {
#pragma unroll
            for (int u = 0; u < STYLE_U; ++u) { const int k = k0 + 64 * u; w[u] = *reinterpret_cast<const float4*>(wrow + (k < D ? k : D - 4)); }
        }
#pragma unroll
        for (int u = 0; u < STYLE_U; ++u) {
            const int k = k0 + 64 * u;
            if (k < D) {
#pragma unroll
                for (int b = 0; b < MB; ++b)
                    if (b < B) {
                        const float4 v = *reinterpret_cast<const float4*>(xs + b * D + k);
                        acc[b] += (w[u].x * v.x + w[u].y * v.y) + (w[u].z * v.z + w[u].w * v.w);
                    }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < MB; ++b)
        if (b < B) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[b] += __shfl_xor(acc[b], o, 64);
        }
    if (n < N && kl == 0) {
        const float bb = bias ? b_mul * bias[n] : 0.f;
        float* yo = y + (size_t)r[3] + n;
#pragma unroll
        for (int b = 0; b < MB; ++b)
            if (b < B) yo[(size_t)b * N] = w_mul * acc[b] + bb;
    }
}
// data gradient: glm[layer][b][k] = w_mul * sum_n gy_g[b][n] W_g[n][k].  grid (D/64, G); the 4 waves split n, LDS reduce.
template <int MB>
__global__ __launch_bounds__(256) void style_bwd_data_kernel(const float* __restrict__ gy, const long long* __restrict__ tab,
                                                             float* __restrict__ glm, int G, int B, int D) {
    extern __shared__ float sh[];                                  // gy_g [B][N] then the wave partials [4][B][64]
    const int g = blockIdx.y;
    const long long* r = tab + (size_t)g * SGX_STYLE_ROW;
    const float* W = reinterpret_cast<const float*>(r[0]);
    const int N = (int)r[2], layer = (int)r[7];
    const float w_mul = __uint_as_float((unsigned)r[5]);
    const float* gyg = gy + (size_t)r[3];
    // gy_g transposed to [n][MB] (rows of images, zero beyond B): the MB values of one n are consecutive, so a lane fetches them with
    // MB / 4 broadcast ds_read_b128 instead of MB ds_read_b32 -- the loop is LDS-issue bound (batch 32: 293 us with the [b][n] image)
    for (int i = threadIdx.x; i < MB * N; i += 256) {
        const int n = i / MB, b = i % MB;
        sh[i] = b < B ? gyg[(size_t)b * N + n] : 0.f;
    }
    __syncthreads();
    const int kk = blockIdx.x * 64 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
    float acc[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) acc[b] = 0.f;
    if (kk < D) {
        // 16 independent weight loads per lane and chunk (a dependent one-load-per-iteration loop is pure latency), and the next
        // chunk's 16 are requested before the FMAs of this one: a wave walks up to N / 4 = 256 rows, and with one chunk in flight at
        // a time that was 16 round trips to memory in a row (34.5 us for 20 MB of weights at batch 4).  n order, hence every sum,
        // is unchanged.
        int n = wave;
        const int full = N > wave ? (N - wave + 3) / 4 / 16 : 0;   // chunks of 16 rows (stride 4) this wave owns entirely
        float wa[16], wb[16];
        auto ld = [&](float (&w)[16], int n0) {
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = W[(size_t)(n0 + 4 * u) * D + kk];
        };
        auto fm = [&](const float (&w)[16], int n0) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float4* row = reinterpret_cast<const float4*>(sh + (size_t)(n0 + 4 * u) * MB);
#pragma unroll
                for (int q = 0; q < MB / 4; ++q) {
                    const float4 g4 = row[q];
                    acc[4 * q] += g4.x * w[u]; acc[4 * q + 1] += g4.y * w[u]; acc[4 * q + 2] += g4.z * w[u]; acc[4 * q + 3] += g4.w * w[u];
                }
            }
        };
        if constexpr (MB <= 8) {
            int c = 0;
            if (full > 0) ld(wa, n);
            for (; c + 1 < full; c += 2, n += 128) {
                ld(wb, n + 64);
                fm(wa, n);
                if (c + 2 < full) ld(wa, n + 128);
                fm(wb, n + 64);
            }
            if (c < full) { fm(wa, n); n += 64; }
        } else {                                               // MB accumulators + two chunks do not fit the register file: one chunk at a time
            for (int c = 0; c < full; ++c, n += 64) { ld(wa, n); fm(wa, n); }
        }
        for (; n < N; n += 4) {
            const float w = W[(size_t)n * D + kk];
            const float4* row = reinterpret_cast<const float4*>(sh + (size_t)n * MB);
#pragma unroll
            for (int q = 0; q < MB / 4; ++q) {
                const float4 g4 = row[q];
                acc[4 * q] += g4.x * w; acc[4 * q + 1] += g4.y * w; acc[4 * q + 2] += g4.z * w; acc[4 * q + 3] += g4.w * w;
            }
        }
    }
    __syncthreads();
    float* part = sh;                                              // reuse: [4][B][64]
#pragma unroll
    for (int b = 0; b < MB; ++b)
        if (b < B) part[(wave * B + b) * 64 + (threadIdx.x & 63)] = acc[b];
    __syncthreads();
    for (int i = threadIdx.x; i < B * 64; i += 256) {
        const int b = i / 64, kl = i % 64, k = blockIdx.x * 64 + kl;
        if (k < D) {
            const float sum = (part[(0 * B + b) * 64 + kl] + part[(1 * B + b) * 64 + kl]) + (part[(2 * B + b) * 64 + kl] + part[(3 * B + b) * 64 + kl]);
            glm[((size_t)layer * B + b) * D + k] = w_mul * sum;
        }
    }
}
// parameter gradients: dW_g[n][k] = w_mul * sum_b gy_g[b][n] x_g[b][k],  db_g[n] = b_mul * sum_b gy_g[b][n].  Flat outputs
// dw[(sum of earlier N + n) * D + k], db[sum of earlier N + n]; block = 16 rows n x all k.
template <int MB>
__global__ __launch_bounds__(256) void style_bwd_param_kernel(const float* __restrict__ gy, const float* __restrict__ lm,
                                                              const long long* __restrict__ tab, float* __restrict__ dw,
                                                              float* __restrict__ db, int G, int B, int D) {
    __shared__ float gs[MB][16];
    const int g = style_group(tab, G, blockIdx.x);
    const long long* r = tab + (size_t)g * SGX_STYLE_ROW;
    const int N = (int)r[2], layer = (int)r[7];
    const float w_mul = __uint_as_float((unsigned)r[5]), b_mul = __uint_as_float((unsigned)r[6]);
    const int n0 = ((int)blockIdx.x - (int)r[4]) * 16;
    const size_t noff = (size_t)r[3] / B;                          // sum of earlier N
    const float* gyg = gy + (size_t)r[3];
    for (int i = threadIdx.x; i < B * 16; i += 256) {
        const int b = i / 16, j = i % 16;
        gs[b][j] = (n0 + j < N) ? gyg[(size_t)b * N + n0 + j] : 0.f;
    }
    __syncthreads();
    const float* x = lm + (size_t)layer * B * D;
    for (int k = threadIdx.x; k < D; k += 256) {
        float xv[MB];
#pragma unroll
        for (int b = 0; b < MB; ++b) xv[b] = b < B ? x[(size_t)b * D + k] : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (n0 + j < N) {
                float s = 0.f;
#pragma unroll
                for (int b = 0; b < MB; ++b)
                    if (b < B) s += gs[b][j] * xv[b];
                dw[(noff + n0 + j) * D + k] = w_mul * s;
            }
    }
    if (db && threadIdx.x < 16 && n0 + (int)threadIdx.x < N) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += gs[b][threadIdx.x];
        db[noff + n0 + threadIdx.x] = b_mul * s;
    }
}
static int style_check(int G, int B, int D) {
    SGX_REQUIRE(G > 0 && B > 0 && B <= STYLE_MAXB && D > 0 && D % 64 == 0, SGX_EUNSUPPORTED, "style affines: G=%d B=%d D=%d", G, B, D);
    return 0;
}
// the MB a batch runs with: the smallest of the instantiations 4, 8, 16, 32 (the sgx_by_int lists below) that holds it
static_assert(STYLE_MAXB == 32, "style_mb and the sgx_by_int<4, 8, 16, 32> lists end at STYLE_MAXB");
static int style_mb(int B) { return B <= 4 ? 4 : (B <= 8 ? 8 : (B <= 16 ? 16 : 32)); }
extern "C" int sgx_style_fwd(const float* lm, const void* table, float* y, int G, int B, int D, int total_tiles, void* stream) {
    int rc = style_check(G, B, D); if (rc) return rc;
    // the kernel stages lm and reads the weight rows with 16-byte loads.  lm is checked here; the W pointers live in the device table,
    // which the host does not read: their alignment is the caller's contract (include/sgx.h)
    SGX_REQUIRE((uintptr_t)lm % 16 == 0, SGX_EINVAL, "style_fwd: lm must be 16-byte aligned");
    SGX_NOTE(0.0, 0.0, "style_fwd G%d B%d", G, B);
    sgx_by_int<4, 8, 16, 32>(style_mb(B), [&](auto mb) {
        constexpr int MB = mb();
        hipLaunchKernelGGL(style_fwd_kernel<MB>, dim3(total_tiles), dim3(256), (size_t)B * D * sizeof(float), (hipStream_t)stream, lm, (const long long*)table, y, G, B, D);
    });
    SGX_LAUNCH_CHECK("style_fwd");
    return 0;
}
extern "C" int sgx_style_bwd_data(const float* gy, const void* table, float* glm, int G, int B, int D, int max_n, void* stream) {
    int rc = style_check(G, B, D); if (rc) return rc;
    const size_t a = (size_t)style_mb(B) * max_n, b = (size_t)4 * B * 64;  // the transposed gy image [max_n][MB], then the wave partials
    SGX_NOTE(0.0, 0.0, "style_bwd_data G%d B%d", G, B);
    sgx_by_int<4, 8, 16, 32>(style_mb(B), [&](auto mb) {
        constexpr int MB = mb();
        hipLaunchKernelGGL(style_bwd_data_kernel<MB>, dim3(D / 64, G), dim3(256), (a > b ? a : b) * sizeof(float), (hipStream_t)stream, gy, (const long long*)table, glm, G, B, D);
    });
    SGX_LAUNCH_CHECK("style_bwd_data");
    return 0;
}
extern "C" int sgx_style_bwd_param(const float* gy, const float* lm, const void* table, float* dw, float* db, int G, int B, int D,
                                   int total_tiles, void* stream) {
    int rc = style_check(G, B, D); if (rc) return rc;
    SGX_NOTE(0.0, 0.0, "style_bwd_param G%d B%d", G, B);
    sgx_by_int<4, 8, 16, 32>(style_mb(B), [&](auto mb) {
        constexpr int MB = mb();
        hipLaunchKernelGGL(style_bwd_param_kernel<MB>, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, gy, lm, (const long long*)table, dw, db, G, B, D);
    });
    SGX_LAUNCH_CHECK("style_bwd_param");
    return 0;
}

// ---------------------------------------------------------------- R1 penalty head: out[0] = sum(x^2)   (models/Losses.py:210)
// and its backward  out = alpha * s[0] * x  with the upstream scalar s kept on the device.
#define SUMSQ_BLOCKS 1024
__global__ __launch_bounds__(256) void sumsq_f32_stage1(const float* __restrict__ x, size_t n, double* __restrict__ partial) {
    __shared__ double sh[16];
    const size_t nvec = n / 4;
    double acc = 0.0;
    float part = 0.f; int cnt = 0;
    const size_t gs = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * gs < nvec; i += 4 * gs) {                      // four 16-byte loads in flight per lane
        const float4 v0 = reinterpret_cast<const float4*>(x)[i], v1 = reinterpret_cast<const float4*>(x)[i + gs];
        const float4 v2 = reinterpret_cast<const float4*>(x)[i + 2 * gs], v3 = reinterpret_cast<const float4*>(x)[i + 3 * gs];
        part += ((v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w)) + ((v1.x * v1.x + v1.y * v1.y) + (v1.z * v1.z + v1.w * v1.w));
        part += ((v2.x * v2.x + v2.y * v2.y) + (v2.z * v2.z + v2.w * v2.w)) + ((v3.x * v3.x + v3.y * v3.y) + (v3.z * v3.z + v3.w * v3.w));
        if (++cnt == 4) { acc += (double)part; part = 0.f; cnt = 0; }
    }
    for (; i < nvec; i += gs) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        part += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (size_t i = nvec * 4; i < n; ++i) part += x[i] * x[i];
    acc += (double)part;
    const double s = block_sum_d(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sumsq_f32_stage2(const double* __restrict__ partial, int nblk, float* __restrict__ out) {
    __shared__ double sh[16];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
    const double s = block_sum_d(acc, sh);
    if (threadIdx.x == 0) out[0] = (float)s;
}
extern "C" size_t sgx_sumsq_ws_bytes(void) { return SUMSQ_BLOCKS * sizeof(double); }
extern "C" int sgx_sumsq_f32(const float* x, size_t n, void* ws, size_t ws_bytes, float* out, void* stream) {
    SGX_REQUIRE(ws_bytes >= SUMSQ_BLOCKS * sizeof(double), SGX_EWORKSPACE, "sumsq: workspace");
    int nblk = (int)((n / 4 + 255) / 256);
    if (nblk > SUMSQ_BLOCKS) nblk = SUMSQ_BLOCKS;
    if (nblk < 1) nblk = 1;
    hipLaunchKernelGGL(sumsq_f32_stage1, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, n, (double*)ws);
    SGX_LAUNCH_CHECK("sumsq_stage1");
    hipLaunchKernelGGL(sumsq_f32_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, nblk, out);
    SGX_LAUNCH_CHECK("sumsq_stage2");
    return 0;
}
// ---- logistic GAN loss heads (models/Losses.py:213-229) in one launch: the scalar loss AND its derivative w.r.t. every logit
//   discriminator: loss = scale * (mean softplus(fake) + mean softplus(-real)),  d/dfake = scale * sigmoid(fake) / n_fake,
//                                                                                   d/dreal = -scale * sigmoid(-real) / n_real
//   generator:     loss = scale * mean softplus(-fake),                            d/dfake = -scale * sigmoid(-fake) / n_fake
// softplus as torch computes it (threshold 20: beyond it the identity).  One wave: a batch is at most a few hundred logits.
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }
__global__ void logistic_loss_kernel(const float* __restrict__ fake, int nf, const float* __restrict__ real, int nr, float scale, int gen,
                                     float* __restrict__ loss, float* __restrict__ gfake, float* __restrict__ greal) {
    const int l = threadIdx.x;
    float sf = 0.f, sr = 0.f;
    const float sgn = gen ? -1.f : 1.f;                     // the generator wants its fakes called real
    for (int i = l; i < nf; i += 64) {
        const float x = sgn * fake[i];
        sf += softplus_f(x);
        gfake[i] = sgn * scale * sigmoid_f(x) / (float)nf;
    }
    for (int i = l; i < nr; i += 64) {
        const float x = -real[i];
        sr += softplus_f(x);
        greal[i] = -scale * sigmoid_f(x) / (float)nr;
    }
    sf = wave_sum(sf); sr = wave_sum(sr);
    if (l == 0) loss[0] = scale * (sf / (float)(nf > 0 ? nf : 1) + (nr > 0 ? sr / (float)nr : 0.f));
}
extern "C" int sgx_logistic_loss(const float* fake, int n_fake, const float* real, int n_real, float scale, int generator, float* loss,
                                 float* g_fake, float* g_real, void* stream) {
    SGX_REQUIRE(fake && n_fake > 0 && loss && g_fake, SGX_EINVAL, "logistic_loss: fake logits, loss and g_fake are required");
    SGX_REQUIRE(generator ? n_real == 0 : (real && g_real && n_real > 0), SGX_EINVAL, "logistic_loss: real logits %s", generator ? "are not part of the generator loss" : "are required");
    hipLaunchKernelGGL(logistic_loss_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, fake, n_fake, real, n_real, scale, generator, loss, g_fake, g_real);
    SGX_LAUNCH_CHECK("logistic_loss");
    return 0;
}
__global__ void scale_dev_kernel(const float* __restrict__ x, const float* __restrict__ s, float alpha, float* __restrict__ out, size_t n) {
    const float k = alpha * s[0];
    const size_t nvec = n / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<const float4*>(x)[i];
        v.x *= k; v.y *= k; v.z *= k; v.w *= k;
        reinterpret_cast<float4*>(out)[i] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (size_t i = nvec * 4; i < n; ++i) out[i] = k * x[i];
}
extern "C" int sgx_scale_dev_f32(const float* x, const float* s, float alpha, float* out, size_t n, void* stream) {
    size_t g = (n / 4 + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(scale_dev_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, x, s, alpha, out, n);
    SGX_LAUNCH_CHECK("scale_dev");
    return 0;
}
