// The image-space filtering group of the ADA paper (Karras et al., NeurIPS 2020, App. B) on the discriminator's fp32 RGB input: four
// per-image band gains folded into ONE symmetric 43-tap filter h[k] = c[|k - 21|], applied separably with whole-sample reflection
// (definitions in include/sgx.h):
//   y = A_v A_h x            forward            (A x)[i] = sum_k h[k] x[refl(i + k - 21)]
//   z = A_h^T A_v^T g        adjoint, a gather: every q in [-21, N + 20] of the zero-extended correlation folded onto refl(q)
// sgx_ada_filter_matrix turns one D evaluation's draws (and, under ADA, its gate uniforms against p) into the per-image half-rows c
// once; the passes read the table, never p.  One axis per launch over a workspace image (horizontal then vertical; the adjoint the
// other way round): no pass computes more taps than the image has outputs, and each is a 1-D stencil.  Every output is
//   acc = c[0] v(0);  acc = fma(c[j], v(+j) + v(-j), acc)  for j = 1 .. 21
// (the symmetric pairing halves the multiplies, the fma is explicit: the library is built with -ffp-contract=off) in BOTH kernels, so
// they agree bit for bit; the tile kernel sends an adjoint output whose window leaves the image to the general kernel's own function.
// A row equal to (1, 0, ..., 0) is the identity flag: both kernels copy such an image (a block-uniform branch), bit for bit.
#include "aug.h"

enum { DF_IMGFILTER = 8192 };
constexpr int DF_BLOCK = 256, DF_HALF = 21, DF_ROW = 22;
constexpr int DF_TILE_MIN = 44;                                      // the tile kernel's least H and W (>= 43: a tile reflects once per side)
// the tiles: horizontal 16 rows x 64 pixels with 24 pixels of halo (21, rounded up so that a staged row starts on a 16-byte boundary),
// vertical 64 rows x 64 floats with 21 rows of halo.  Row strides: 336 + 1 floats (lanes read 12 floats apart, four rows per wave: the
// rows land in the four bank classes mod 4), 64 + 4 floats (one access width, 16-byte reads)
constexpr int DF_H_ROWS = 16, DF_H_PX = 64, DF_H_HALO = 24, DF_H_STRIDE = 3 * (DF_H_PX + 2 * DF_H_HALO) + 1;
constexpr int DF_V_ROWS = 64, DF_V_COLS = 64, DF_V_STRIDE = DF_V_COLS + 4;
constexpr int DF_LDS_FLOATS = (DF_V_ROWS + 2 * DF_HALF) * DF_V_STRIDE;
static_assert(DF_H_ROWS * DF_H_STRIDE <= DF_LDS_FLOATS, "one LDS array serves both axes");
static_assert(DF_H_ROWS * (DF_H_PX / 4) == DF_BLOCK && (DF_V_ROWS / 4) * (DF_V_COLS / 4) == DF_BLOCK, "four outputs along the axis per lane");

// fbh[i][j] = fb[i][21 + j]: band i of the sym2 bank (include/sgx.h), built in fp64; every tap is a dyadic rational that fp32 holds exactly
__constant__ float df_fbh[4][DF_ROW] = {
    {1.250000000e-01f, 1.186523438e-01f, 1.054687500e-01f, 8.905029297e-02f, 7.031250000e-02f, 5.108642578e-02f, 3.222656250e-02f, 1.428222656e-02f,
     0.000000000e+00f, -6.469726562e-03f, -8.789062500e-03f, -9.063720703e-03f, -7.812500000e-03f, -6.317138672e-03f, -4.394531250e-03f,
     -2.014160156e-03f, 0.000000000e+00f, 5.493164062e-04f, 4.882812500e-04f, 2.746582031e-04f, 0.000000000e+00f, -3.051757812e-05f},
    {1.250000000e-01f, 9.228515625e-02f, 3.515625000e-02f, -2.459716797e-02f, -7.031250000e-02f, -6.866455078e-02f, -4.785156250e-02f, -2.307128906e-02f,
     0.000000000e+00f, 7.446289062e-03f, 8.789062500e-03f, 9.063720703e-03f, 7.812500000e-03f, 6.317138672e-03f, 4.394531250e-03f,
     2.014160156e-03f, 0.000000000e+00f, -5.493164062e-04f, -4.882812500e-04f, -2.746582031e-04f, 0.000000000e+00f, 3.051757812e-05f},
    {2.500000000e-01f, 7.031250000e-02f, -1.406250000e-01f, -9.570312500e-02f, 0.000000000e+00f, 1.757812500e-02f, 1.562500000e-02f, 8.789062500e-03f,
     0.000000000e+00f, -9.765625000e-04f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
    {5.000000000e-01f, -2.812500000e-01f, 0.000000000e+00f, 3.125000000e-02f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f,
     0.f, 0.f, 0.f}};

// z = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3)
__device__ __forceinline__ float df_normal(float ua, float ub) {
    const float r = sqrtf(__fmul_rn(-2.f, logf(__fsub_rn(1.f, ua))));
    const float z = __fmul_rn(r, cosf(__fmul_rn(6.283185307179586f, ub)));
    return fminf(fmaxf(z, -3.f), 3.f);
}

__global__ __launch_bounds__(DF_BLOCK) void ada_filter_matrix_kernel(const float* __restrict__ u, int u_stride, const float* __restrict__ gu,
                                                                     int gu_stride, const float* __restrict__ state, int policy,
                                                                     float* __restrict__ mat, int B) {
    const int b = blockIdx.x * DF_BLOCK + threadIdx.x;
    if (b >= B) return;
    int on = (policy & DF_IMGFILTER) ? 15 : 0;                   // bit i: band i is on for this image
    if (gu) {
        const float p = state[0];
        const float* g = gu + (size_t)gu_stride * b;
        on &= (g[0] < p ? 1 : 0) | (g[1] < p ? 2 : 0) | (g[2] < p ? 4 : 0) | (g[3] < p ? 8 : 0);
    }
    float* c = mat + DF_ROW * (size_t)b;
    if (!on) {                                                   // the identity row, what the pass kernels copy under (a branch: not the sum)
        c[0] = 1.f;
#pragma unroll
        for (int j = 1; j < DF_ROW; ++j) c[j] = 0.f;
        return;
    }
    const float* ub = u + (size_t)u_stride * b;
    float g[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {                                // t = e_i-scaled ones, t <- t / sqrt(mean(t^2)), g <- g t; a band that is off: n == 1
        const float t = ((on >> i) & 1) ? exp2f(df_normal(ub[2 * i], ub[2 * i + 1])) : 1.f;
        const float n = sqrtf(__fmul_rn(0.25f, __fadd_rn(3.f, __fmul_rn(t, t))));
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = __fmul_rn(g[k], __fdiv_rn(k == i ? t : 1.f, n));
    }
#pragma unroll
    for (int j = 0; j < DF_ROW; ++j)
        c[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(g[0], df_fbh[0][j]), __fmul_rn(g[1], df_fbh[1][j])), __fmul_rn(g[2], df_fbh[2][j])),
                         __fmul_rn(g[3], df_fbh[3][j]));
}

// One image's half-row (block-uniform); -> it is the identity flag.
__device__ __forceinline__ bool df_load_row(const float* __restrict__ m, float (&c)[DF_ROW]) {
    bool id = true;
#pragma unroll
    for (int j = 0; j < DF_ROW; ++j) {
        c[j] = m[j];
        id = id && c[j] == (j == 0 ? 1.f : 0.f);
    }
    return id;
}

// Whole-sample reflection continued periodically (np.pad(mode="reflect") for any pad width), N >= 2.
__device__ __forceinline__ int df_refl(int q, int N) {
    const int P = 2 * (N - 1);
    int m = q % P;
    if (m < 0) m += P;
    return m < N ? m : P - m;
}

// ---- the general functions: one output along an axis of N samples `s` floats apart, x0 the sample at position 0, c the image's row in
// memory (a uniform address; their loops are rolled, and a rolled loop over a register array would index it through scratch)
__device__ __forceinline__ float df_fwd_at(const float* __restrict__ x0, int s, int N, int i, const float* __restrict__ c) {
    float acc = __fmul_rn(c[0], x0[(size_t)i * s]);
#pragma unroll 1
    for (int j = 1; j <= DF_HALF; ++j)
        acc = __fmaf_rn(c[j], __fadd_rn(x0[(size_t)df_refl(i + j, N) * s], x0[(size_t)df_refl(i - j, N) * s]), acc);
    return acc;
}
// the correlation of the zero-extended input at q (any q)
__device__ __forceinline__ float df_z_at(const float* __restrict__ x0, int s, int N, int q, const float* __restrict__ c) {
    auto g = [&](int i) { return (i >= 0 && i < N) ? x0[(size_t)i * s] : 0.f; };
    float acc = __fmul_rn(c[0], g(q));
#pragma unroll 1
    for (int j = 1; j <= DF_HALF; ++j) acc = __fmaf_rn(c[j], __fadd_rn(g(q + j), g(q - j)), acc);
    return acc;
}
// (A^T g)[j]: the q in [-21, N + 20] with refl(q) == j are m P - j (for 0 < j < N - 1) and m P + j, P = 2 (N - 1); summed in ascending q
__device__ __forceinline__ float df_adj_at(const float* __restrict__ x0, int s, int N, int j, const float* __restrict__ c) {
    const int P = 2 * (N - 1), lo = -DF_HALF, hi = N + DF_HALF - 1;
    const bool two = j != 0 && j != N - 1;
    float acc = 0.f;
    bool first = true;
    for (int m = -(DF_HALF / P + 1); m <= hi / P + 1; ++m) {
        const int q[2] = {m * P - j, m * P + j};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if ((e == 0 && !two) || q[e] < lo || q[e] > hi) continue;
            const float z = df_z_at(x0, s, N, q[e], c);
            acc = first ? z : __fadd_rn(acc, z);
            first = false;
        }
    }
    return acc;
}

// Any H, W >= 2, any 4-byte aligned base, any number of reflections: one output float per thread.  AXIS 0 filters along W (samples 3
// floats apart), 1 along H (3 W apart).  grid (ceil(3 H W / DF_BLOCK), B).
template <int AXIS, bool ADJ>
__global__ __launch_bounds__(DF_BLOCK) void ada_filter_px_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat,
                                                                 int H, int W) {
    const int b = blockIdx.y;
    float c[DF_ROW];
    const bool identity = df_load_row(mat + DF_ROW * (size_t)b, c);
    const int L = 3 * W, n = H * L;
    const int f = blockIdx.x * DF_BLOCK + threadIdx.x;
    if (f >= n) return;
    const float* xb = x + (size_t)b * n;
    float* yb = y + (size_t)b * n;
    if (identity) {                                              // (block-uniform) a copy, bit for bit
        yb[f] = xb[f];
        return;
    }
    const int row = f / L, e = f - row * L;
    const int pos = AXIS == 0 ? e / 3 : row, N = AXIS == 0 ? W : H, s = AXIS == 0 ? 3 : L;
    const float* x0 = xb + (f - pos * s);
    const float* cm = mat + DF_ROW * (size_t)b;
    yb[f] = ADJ ? df_adj_at(x0, s, N, pos, cm) : df_fwd_at(x0, s, N, pos, cm);
}

// Four consecutive outputs along the axis for V adjacent floats, from LDS: w points at output 0's sample, samples PS floats apart.  The
// window slides through registers: every LDS value is read once.
template <int V, int PS>
__device__ __forceinline__ void df_run4(const float* w, const float (&c)[DF_ROW], float (&acc)[4][V]) {
    float up[4][V], dn[4][V];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            up[o][v] = dn[o][v] = w[o * PS + v];
            acc[o][v] = __fmul_rn(c[0], up[o][v]);
        }
#pragma unroll
    for (int j = 1; j <= DF_HALF; ++j) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            up[0][v] = up[1][v]; up[1][v] = up[2][v]; up[2][v] = up[3][v]; up[3][v] = w[(3 + j) * PS + v];
            dn[3][v] = dn[2][v]; dn[2][v] = dn[1][v]; dn[1][v] = dn[0][v]; dn[0][v] = w[-j * PS + v];
        }
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[o][v] = __fmaf_rn(c[j], __fadd_rn(up[o][v], dn[o][v]), acc[o][v]);
    }
}

// W % 4 == 0, 16-byte aligned bases, H, W >= DF_TILE_MIN: a block stages its tile and the halo along the axis through LDS (16-byte
// loads; the reflection is applied while staging, so the filter loop is branch-free) and every lane filters four consecutive outputs
// (16-byte stores).  An adjoint output whose window leaves the image (position <= 21 or >= N - 22: the zero extension and the folds)
// is df_adj_at's, the general kernel's function.  grid (tiles, B), tiles row major.
template <int AXIS, bool ADJ>
__global__ __launch_bounds__(DF_BLOCK) void ada_filter_tile_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mat,
                                                                   int H, int W, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float lds[DF_LDS_FLOATS];
    const int b = blockIdx.y, t = threadIdx.x;
    float c[DF_ROW];
    const bool identity = df_load_row(mat + DF_ROW * (size_t)b, c);
    const int L = 3 * W;
    const float* xb = x + (size_t)b * H * L;
    float* yb = y + (size_t)b * H * L;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    if (AXIS == 0) {
        const int row0 = ty * DF_H_ROWS, p0 = tx * DF_H_PX;
        const int r = t / (DF_H_PX / 4), px = p0 + 4 * (t % (DF_H_PX / 4)), row = row0 + r;
        const bool live = row < H && px < W;                     // (W % 4 == 0: a lane's four pixels are inside together)
        const size_t at = (size_t)row * L + 3 * px;
        if (identity) {                                          // (block-uniform) a copy, bit for bit
            if (live) {
                const float4* s = reinterpret_cast<const float4*>(xb + at);
                const float4 v0 = s[0], v1 = s[1], v2 = s[2];
                float4* d = reinterpret_cast<float4*>(yb + at);
                d[0] = v0; d[1] = v1; d[2] = v2;
            }
            return;
        }
        constexpr int CH = 3 * (DF_H_PX + 2 * DF_H_HALO) / 4;    // 16-byte chunks of a staged row; 3 W % 4 == 0: a chunk is inside or outside whole
        const int g0 = 3 * (p0 - DF_H_HALO);
        for (int k = t; k < DF_H_ROWS * CH; k += DF_BLOCK) {
            const int lr = k / CH, v = k - lr * CH, srow = row0 + lr, g = g0 + 4 * v;
            if (srow >= H) continue;
            const float* xr = xb + (size_t)srow * L;
            float q[4];
            if (g >= 0 && g + 4 <= L) {
                const float4 ld = *reinterpret_cast<const float4*>(xr + g);
                q[0] = ld.x; q[1] = ld.y; q[2] = ld.z; q[3] = ld.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int gg = g + e, p = gg >= 0 ? gg / 3 : -((2 - gg) / 3), ch = gg - 3 * p;
                    q[e] = xr[3 * df_refl(p, W) + ch];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) lds[lr * DF_H_STRIDE + 4 * v + e] = q[e];
        }
        __syncthreads();
        if (!live) return;
        float acc[4][3];
        df_run4<3, 3>(lds + r * DF_H_STRIDE + 3 * (DF_H_HALO + (px - p0)), c, acc);
        if (ADJ && (px <= DF_HALF || px + 3 >= W - DF_ROW)) {
#pragma unroll 1
            for (int e = 0; e < 12; ++e) {                       // (rolled: one copy of the general function; the result is selected into place)
                const int pos = px + e / 3;
                if (pos > DF_HALF && pos < W - DF_ROW) continue;
                const float z = df_adj_at(xb + (size_t)row * L + e % 3, 3, W, pos, mat + DF_ROW * (size_t)b);
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k == e) acc[k / 3][k % 3] = z;
            }
        }
        float4* d = reinterpret_cast<float4*>(yb + at);
        d[0] = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[1][0]);
        d[1] = make_float4(acc[1][1], acc[1][2], acc[2][0], acc[2][1]);
        d[2] = make_float4(acc[2][2], acc[3][0], acc[3][1], acc[3][2]);
    } else {
        const int row0 = ty * DF_V_ROWS, f0 = tx * DF_V_COLS;
        const int fx = f0 + 4 * (t % (DF_V_COLS / 4)), ro = 4 * (t / (DF_V_COLS / 4));
        const bool live = fx < L && row0 + ro < H;               // (3 W % 4 == 0: a lane's four floats are inside together)
        if (identity) {                                          // (block-uniform) a copy, bit for bit
            if (live) {
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (row0 + ro + o < H) {
                        const size_t at = (size_t)(row0 + ro + o) * L + fx;
                        *reinterpret_cast<float4*>(yb + at) = *reinterpret_cast<const float4*>(xb + at);
                    }
            }
            return;
        }
        constexpr int CH = DF_V_COLS / 4;
        for (int k = t; k < (DF_V_ROWS + 2 * DF_HALF) * CH; k += DF_BLOCK) {
            const int lr = k / CH, v = k - lr * CH, f = f0 + 4 * v;
            if (f >= L) continue;
            const int srow = df_refl(row0 - DF_HALF + lr, H);
            *reinterpret_cast<float4*>(lds + lr * DF_V_STRIDE + 4 * v) = *reinterpret_cast<const float4*>(xb + (size_t)srow * L + f);
        }
        __syncthreads();
        if (!live) return;
        float acc[4][4];
        df_run4<4, DF_V_STRIDE>(lds + (DF_HALF + ro) * DF_V_STRIDE + (fx - f0), c, acc);
        if (ADJ && (row0 + ro <= DF_HALF || row0 + ro + 3 >= H - DF_ROW)) {
#pragma unroll 1
            for (int e = 0; e < 16; ++e) {                       // (rolled, as above)
                const int row = row0 + ro + e / 4;
                if (row >= H || (row > DF_HALF && row < H - DF_ROW)) continue;
                const float z = df_adj_at(xb + fx + e % 4, L, H, row, mat + DF_ROW * (size_t)b);
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k == e) acc[k / 4][k % 4] = z;
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int row = row0 + ro + o;
            if (row < H) *reinterpret_cast<float4*>(yb + (size_t)row * L + fx) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
        }
    }
}

extern "C" int sgx_ada_filter_matrix(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, float* mat,
                                     int B, void* stream) {
    if (int rc = aug_check_matrix("ada_filter_matrix", u, u_stride, 8, gu, gu_stride, 4, state, mat, B, policy_bits, DF_IMGFILTER, "imgfilter 8192"))
        return rc;
    SGX_NOTE(0.0, (32.0 + (gu ? 20.0 : 0.0) + 88.0) * B, "ada_filter_matrix B%d", B);
    hipLaunchKernelGGL(ada_filter_matrix_kernel, dim3((B + DF_BLOCK - 1) / DF_BLOCK), dim3(DF_BLOCK), 0, (hipStream_t)stream, u, u_stride, gu,
                       gu_stride, state, policy_bits, mat, B);
    SGX_LAUNCH_CHECK("ada_filter_matrix");
    return 0;
}

// Two launches, one axis each, through the workspace: horizontal then vertical (the adjoint: vertical then horizontal).  The tile
// kernel where rows split into whole groups of four pixels, the bases are aligned and both sides reach DF_TILE_MIN; else the general one.
enum { DF_K_PX = 0, DF_K_TILE = 1 };
struct DfLaunch { int kernel, axis, adjoint, gx, gy, tiles_x; };
struct DfPlan { int n; DfLaunch l[2]; };
static_assert(SGX_ADA_FILTER_PLAN_INTS == 1 + 2 * sizeof(DfLaunch) / sizeof(int), "sgx_ada_filter_plan: the count, then two launches");
static int df_plan(bool ptrs_ok, int B, int H, int W, int adjoint, bool aligned, DfPlan* p) {
    if (int rc = aug_check_images("ada_filter", ptrs_ok, B, H, W)) return rc;
    SGX_REQUIRE(H >= 2 && W >= 2, SGX_EINVAL, "ada_filter: the reflection needs H, W >= 2, got %dx%d", H, W);
    const bool tile = aug_vec4(W, aligned) && H >= DF_TILE_MIN && W >= DF_TILE_MIN;
    p->n = 2;
    for (int i = 0; i < 2; ++i) {
        const int axis = adjoint ? 1 - i : i;
        int gx = aug_grid((size_t)3 * H * W), tiles_x = 0;
        if (tile) {
            tiles_x = axis == 0 ? (W + DF_H_PX - 1) / DF_H_PX : (3 * W + DF_V_COLS - 1) / DF_V_COLS;
            gx = tiles_x * (axis == 0 ? (H + DF_H_ROWS - 1) / DF_H_ROWS : (H + DF_V_ROWS - 1) / DF_V_ROWS);
        }
        p->l[i] = DfLaunch{tile ? DF_K_TILE : DF_K_PX, axis, adjoint != 0, gx, B, tiles_x};
    }
    return 0;
}

extern "C" size_t sgx_ada_filter_workspace_bytes(int B, int H, int W) {
    return (B < 1 || H < 2 || W < 2) ? 0 : (size_t)12 * B * H * W;      // the image between the two axes
}

extern "C" int sgx_ada_filter_plan(int B, int H, int W, int adjoint, int aligned, int* out) {
    SGX_REQUIRE(out, SGX_EINVAL, "ada_filter_plan: out is NULL");
    for (int i = 0; i < SGX_ADA_FILTER_PLAN_INTS; ++i) out[i] = 0;
    DfPlan p;
    if (int rc = df_plan(true, B, H, W, adjoint, aligned != 0, &p)) return rc;
    out[0] = p.n;
    for (int i = 0; i < p.n; ++i) {
        const DfLaunch& l = p.l[i];
        const int v[6] = {l.kernel, l.axis, l.adjoint, l.gx, l.gy, l.tiles_x};
        for (int k = 0; k < 6; ++k) out[1 + 6 * i + k] = v[k];
    }
    return 0;
}

extern "C" int sgx_ada_filter(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* ws, size_t ws_bytes, void* stream) {
    DfPlan p;
    if (int rc = df_plan(x && y && mat, B, H, W, adjoint, aug_aligned(x, y), &p)) return rc;
    if (int rc = aug_check_out_of_place("ada_filter", x, y, "")) return rc;
    if (int rc = aug_check_ws("ada_filter", ws, ws_bytes, sgx_ada_filter_workspace_bytes(B, H, W))) return rc;
    SGX_REQUIRE(sgx_aligned16(ws) && ws != x && ws != y, SGX_EWORKSPACE, "ada_filter: the workspace must be 16-byte aligned and apart from x and y");
    hipStream_t st = (hipStream_t)stream;
    float* mid = static_cast<float*>(ws);
    for (int i = 0; i < p.n; ++i) {
        const DfLaunch& l = p.l[i];
        const float* src = i == 0 ? x : mid;
        float* dst = i == 0 ? mid : y;
        const dim3 grid(l.gx, l.gy), block(DF_BLOCK);
        const bool tile = l.kernel == DF_K_TILE;
        SGX_NOTE(2.0 * 43 * 3 * B * H * W, 24.0 * B * H * W, "ada_filter_%s B%d %dx%d %s %s", tile ? "tile" : "px", B, H, W, adjoint ? "adj" : "fwd",
                 l.axis ? "v" : "h");
        sgx_by_int<0, 1, 2, 3>(2 * l.axis + l.adjoint, [&](auto v) {
            constexpr int AXIS = v() / 2;
            constexpr bool ADJ = v() % 2 == 1;
            if (tile) hipLaunchKernelGGL((ada_filter_tile_kernel<AXIS, ADJ>), grid, block, 0, st, src, dst, mat, H, W, l.tiles_x);
            else hipLaunchKernelGGL((ada_filter_px_kernel<AXIS, ADJ>), grid, block, 0, st, src, dst, mat, H, W);
        });
        SGX_LAUNCH_CHECK("ada_filter");
    }
    return 0;
}
