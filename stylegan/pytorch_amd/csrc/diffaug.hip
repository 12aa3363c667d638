// DiffAugment (Zhao et al., NeurIPS 2020) on the discriminator's fp32 RGB input, policy ⊆ {color, translation, cutout} in that order:
//   y = Mask(Shift(L x + b))        forward (with_bias) / forward without the bias (the linear part, for the R1 double backward)
//   z = L(Shift^T(Mask g))          adjoint
// per image b with seven uniform draws u[b][0..6] (definitions in include/sgx.h).  L x = c*s*(x - m_x) + c*(m_x - M_x) + M_x, with m_x
// the per-pixel and M_x the per-image mean: symmetric, so it is its own adjoint.  Every pass is a gather (an output pixel computes its
// source pixel, the cutout test and the colour term): no scatter, no atomics.  The per-image sum M needs one pass of its own
// (diffaug_sum_kernel: fixed-order partials, one per block) which the apply kernel's prologue finishes in a fixed order, so results are
// bit-identical run to run.  With colour off there is no sum pass.
//
// ADA (Karras et al., NeurIPS 2020): the same kernels with GATED = true take every image's ops from img_bits[b] (sgx_ada_gates: op k of
// image b is on iff its gate uniform is < p, p = state[0] read on the device) instead of one policy for the batch; an image without
// the colour bit is gathers and zeros only (its sum-pass blocks return before loading, the apply kernel does not read their partials).
// sgx_ada_update is the controller: one block that adds this D step's sign(D(real)) to the state and, every `interval` calls, moves p.
//
// Pixel blitting (the first group of the ADA paper; sgx_diffaug_blit): policy bits 8 = xflip and 16 = rot90 put an orientation
// G = Rot^k o Flip (two more draws, u7 and u8) between the colour and the shift:  y = Mask(Shift(G(L x + b))),  z = L(G^T(Shift^T(Mask g))).
// G is a pixel permutation, so it lives in the index arithmetic of the gather and both sum passes sum what they sum without it, in the
// same order.  A launch without the rot90 bit reads rows (reversed in registers under a flip: diffaug_blit_row_kernel); a launch with
// it may turn rows into columns for some of its images and stages a square tile through LDS (diffaug_blit_tile_kernel).  What a policy
// of the first three ops launches (sgx_diffaug, sgx_diffaug_gated) is untouched by it.
#include "aug.h"

enum { DA_COLOR = 1, DA_TRANSLATION = 2, DA_CUTOUT = 4, DA_XFLIP = 8, DA_ROT90 = 16 };
enum { DA_OPS3 = DA_COLOR | DA_TRANSLATION | DA_CUTOUT, DA_OPS5 = DA_OPS3 | DA_XFLIP | DA_ROT90 };
enum { DA_PLAIN = 0, DA_FWD = 1, DA_ADJ = 2 };      // what a unit load gathers: the input itself / Shift(.) with the output mask / Shift^T(Mask .)
constexpr int DA_BLOCK = 256;
constexpr int DA_PART_PIXELS = 16384;               // pixels per partial sum of the sum pass (64 partials per 1024^2 image)

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte access at a 4-byte aligned address (dwordx4)

struct DaImg {
    int tx, ty;                  // y[i][j] = x[i + tx][j + ty]
    int r0, r1, c0, c1;          // cutout rows [r0, r1) x columns [c0, c1), already intersected with the image
    float b, s, c;               // brightness, saturation, contrast
};

__device__ __forceinline__ int da_draw(float u, int n, int hi) {        // min(floor(u * n), hi) with the product in fp32
    return min((int)floorf(__fmul_rn(u, (float)n)), hi);
}

__device__ __forceinline__ DaImg da_params(const float* __restrict__ u, int H, int W, int policy) {
    DaImg q;
    q.tx = q.ty = 0;
    q.r0 = q.r1 = q.c0 = q.c1 = 0;
    q.b = 0.f; q.s = 1.f; q.c = 1.f;
    if (policy & DA_COLOR) { q.b = u[0] - 0.5f; q.s = 2.f * u[1]; q.c = u[2] + 0.5f; }
    if (policy & DA_TRANSLATION) {
        const int sh = (H + 4) / 8, sw = (W + 4) / 8;                 // int(H * 0.125 + 0.5)
        q.tx = da_draw(u[3], 2 * sh + 1, 2 * sh) - sh;
        q.ty = da_draw(u[4], 2 * sw + 1, 2 * sw) - sw;
    }
    if (policy & DA_CUTOUT) {
        const int ch = (H + 1) / 2, cw = (W + 1) / 2;                 // int(H * 0.5 + 0.5)
        const int ox = da_draw(u[5], H + 1 - ch % 2, H - ch % 2), oy = da_draw(u[6], W + 1 - cw % 2, W - cw % 2);
        q.r0 = max(ox - ch / 2, 0); q.r1 = min(ox - ch / 2 + ch, H);
        q.c0 = max(oy - cw / 2, 0); q.c1 = min(oy - cw / 2 + cw, W);
    }
    return q;
}

// The 3P source values of the P pixels (i, j0 .. j0+P-1) of one image, ok[k] = whether pixel k has a source (zero otherwise).
// DA_FWD: source (i + tx, j + ty), masked by the cutout at the output pixel.  DA_ADJ: source (i - tx, j - ty), masked at the source.
template <int P, int MODE>
__device__ __forceinline__ void da_load(const float* __restrict__ xb, int H, int W, int i, int j0, const DaImg& q, float (&v)[3 * P], bool (&ok)[P]) {
    if (MODE == DA_PLAIN) {
        const float* s = xb + ((size_t)i * W + j0) * 3;
        if (P == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 t = reinterpret_cast<const float4*>(s)[k];
                v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * P; ++k) v[k] = s[k];
        }
#pragma unroll
        for (int k = 0; k < P; ++k) ok[k] = true;
        return;
    }
    const int si = MODE == DA_FWD ? i + q.tx : i - q.tx;
    const int sj0 = MODE == DA_FWD ? j0 + q.ty : j0 - q.ty;
    const bool row_in = si >= 0 && si < H;
    const int mi = MODE == DA_FWD ? i : si, mj0 = MODE == DA_FWD ? j0 : sj0;          // where the cutout is tested
    const bool row_cut = mi >= q.r0 && mi < q.r1;
    const bool none_cut = !row_cut || mj0 + P <= q.c0 || mj0 >= q.c1;
    if (row_in && sj0 >= 0 && sj0 + P <= W && none_cut) {
        const float* s = xb + ((size_t)si * W + sj0) * 3;                                // 4-byte aligned: ty shifts by whole pixels
        if (P == 4) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const f32x4u t = reinterpret_cast<const f32x4u*>(s)[k];
                v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * P; ++k) v[k] = s[k];
        }
#pragma unroll
        for (int k = 0; k < P; ++k) ok[k] = true;
        return;
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {                                                      // image border or cutout edge: pixel by pixel
        const int sj = sj0 + k, mj = mj0 + k;
        ok[k] = row_in && sj >= 0 && sj < W && !(row_cut && mj >= q.c0 && mj < q.c1);
        if (ok[k]) {
            const float* s = xb + ((size_t)si * W + sj) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = s[ch];
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = 0.f;
        }
    }
}

// Per-image sums of what the apply kernel's colour term averages: the input (forward) or Shift^T(Mask g) (adjoint).  grid (nparts, B):
// block p of image b sums pixels [p * DA_PART_PIXELS, (p + 1) * DA_PART_PIXELS) in a fixed order into part[b * nparts + p].
template <int P, int MODE, bool GATED>
__global__ __launch_bounds__(DA_BLOCK) void diffaug_sum_kernel(const float* __restrict__ x, const float* __restrict__ u, float* __restrict__ part,
                                                               int nparts, int H, int W, int policy, const int* __restrict__ img_bits) {
    const int b = blockIdx.y;
    if (GATED) {
        policy &= img_bits[b];
        if (!(policy & DA_COLOR)) return;                        // (block-uniform) nobody reads this image's partials
    }
    const DaImg q = da_params(u + 7 * b, H, W, policy);
    const float* xb = x + (size_t)b * H * W * 3;
    const int upr = W / P, nunits = H * upr;
    constexpr int UPT = DA_PART_PIXELS / (DA_BLOCK * P);                               // units per thread
    float acc = 0.f;
#pragma unroll 4
    for (int it = 0; it < UPT; ++it) {
        const int unit = (blockIdx.x * UPT + it) * DA_BLOCK + threadIdx.x;
        if (unit < nunits) {
            const int i = unit / upr, j0 = (unit - i * upr) * P;
            float v[3 * P]; bool ok[P];
            da_load<P, MODE>(xb, H, W, i, j0, q, v, ok);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 3 * P; ++k) s += v[k];
            acc += s;
        }
    }
    __shared__ float red[DA_BLOCK / WAVE];
    acc = wave_sum(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
#pragma unroll
        for (int w = 1; w < DA_BLOCK / WAVE; ++w) t += red[w];
        part[(size_t)b * nparts + blockIdx.x] = t;
    }
}

// One unit (P pixels of a row) per thread, one trip (short-lived blocks).  grid (ceil(units / DA_BLOCK), B).
template <int P, bool ADJ, bool GATED>
__global__ __launch_bounds__(DA_BLOCK) void diffaug_apply_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ u,
                                                                 const float* __restrict__ part, int nparts, int H, int W, int policy, int with_bias,
                                                                 const int* __restrict__ img_bits) {
    const int b = blockIdx.y;
    if (GATED) policy &= img_bits[b];                            // this image's ops (block-uniform); 0: a plain copy
    const int upr = W / P;
    const int unit = blockIdx.x * DA_BLOCK + threadIdx.x;
    const DaImg q = da_params(u + 7 * b, H, W, policy);
    float M = 0.f;
    if (policy & DA_COLOR) {                                     // finish the image's sum: every wave, fixed order, all lanes active
        const int lane = threadIdx.x & (WAVE - 1);
        float t = 0.f;
        for (int k = lane; k < nparts; k += WAVE) t += part[(size_t)b * nparts + k];
        M = wave_sum(t) / (3.f * (float)H * (float)W);
    }
    if (unit >= H * upr) return;
    const int i = unit / upr, j0 = (unit - i * upr) * P;
    float v[3 * P]; bool ok[P];
    da_load<P, ADJ ? DA_ADJ : DA_FWD>(x + (size_t)b * H * W * 3, H, W, i, j0, q, v, ok);
    if (policy & DA_COLOR) {
        const float cs = q.c * q.s, k0 = (1.f - q.c) * M + (with_bias && !ADJ ? q.b : 0.f);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const float m = (v[3 * k] + v[3 * k + 1] + v[3 * k + 2]) * (1.f / 3.f);
            const float cm = q.c * m + k0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float o = cs * (v[3 * k + ch] - m) + cm;
                v[3 * k + ch] = (ADJ || ok[k]) ? o : 0.f;                              // forward: the mask comes after the colour
            }
        }
    }
    float* d = y + (((size_t)b * H + i) * W + j0) * 3;
    if (P == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<float4*>(d)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * P; ++k) d[k] = v[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Pixel blitting: the orientation G = Rot^k o Flip in the gather (definitions in include/sgx.h)
//
// G as an index map: G(x)[p][q] = x[row][col] with (a, b) = t ? (q, p) : (p, q), row = nr ? H-1-a : a, col = nc ? W-1-b : b, where
// t = k & 1, nr = k >> 1, nc = f ^ (k == 1 || k == 2) (the table of sgx.h, one line per k, with the flip folded in).  Its inverse,
// which the adjoint walks, has the same form with nr and nc exchanged when t is set.  Block-uniform, like the gated policy.
struct DaOri { int t, nr, nc; };

__device__ __forceinline__ DaOri da_orient(const float* __restrict__ u, int policy, bool inverse) {
    const int f = (policy & DA_XFLIP) ? da_draw(u[7], 2, 1) : 0;
    const int k = (policy & DA_ROT90) ? da_draw(u[8], 4, 3) : 0;
    DaOri o;
    o.t = k & 1;
    const int nr = k >> 1, nc = f ^ (((k + 1) >> 1) & 1);
    o.nr = (inverse && o.t) ? nc : nr;
    o.nc = (inverse && o.t) ? nr : nc;
    return o;
}

__device__ __forceinline__ void da_orient_at(const DaOri& o, int H, int W, int p, int q, int& row, int& col) {
    const int a = o.t ? q : p, b = o.t ? p : q;
    row = o.nr ? H - 1 - a : a;
    col = o.nc ? W - 1 - b : b;
}

// Source pixel of output pixel (i, j).  Forward: G^-1 of the shifted position (i + tx, j + ty) in x (in the image exactly when the
// shifted position is: G permutes the image).  Adjoint: (a, b) = G(i, j), then (a - tx, b - ty) in g.
template <bool ADJ>
__device__ __forceinline__ void da_blit_src(const DaImg& q, const DaOri& o, int H, int W, int i, int j, int& si, int& sj) {
    if (ADJ) {
        da_orient_at(o, H, W, i, j, si, sj);
        si -= q.tx; sj -= q.ty;
    } else {
        da_orient_at(o, H, W, i + q.tx, j + q.ty, si, sj);
    }
}

// Whether output pixel (i, j) with source (si, sj) has a value: the source in the image, and no cutout at the output pixel (forward)
// or at the source (adjoint).
template <bool ADJ>
__device__ __forceinline__ bool da_blit_ok(const DaImg& q, int H, int W, int i, int j, int si, int sj) {
    const int mi = ADJ ? si : i, mj = ADJ ? sj : j;
    return si >= 0 && si < H && sj >= 0 && sj < W && !(mi >= q.r0 && mi < q.r1 && mj >= q.c0 && mj < q.c1);
}

// da_load with the orientation.  The four sources of a group that stays in its row (t = 0) are a contiguous run, read forwards or
// backwards: three dwordx4 as in da_load, the pixel order reversed in registers.  Everything else (a border, a cutout edge, a turned
// image, P = 1) goes pixel by pixel.
template <int P, bool ADJ>
__device__ __forceinline__ void da_load_blit(const float* __restrict__ xb, int H, int W, int i, int j0, const DaImg& q, const DaOri& o,
                                             float (&v)[3 * P], bool (&ok)[P]) {
    if (P == 4 && !o.t) {
        int si, s0, s3;
        da_blit_src<ADJ>(q, o, H, W, i, j0, si, s0);
        s3 = o.nc ? s0 - 3 : s0 + 3;
        const int lo = min(s0, s3);
        const int mi = ADJ ? si : i, mj0 = ADJ ? lo : j0;                                  // where the cutout is tested
        const bool none_cut = !(mi >= q.r0 && mi < q.r1) || mj0 + P <= q.c0 || mj0 >= q.c1;
        if (si >= 0 && si < H && lo >= 0 && lo + P <= W && none_cut) {
            const float* s = xb + ((size_t)si * W + lo) * 3;
            float t[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const f32x4u w = reinterpret_cast<const f32x4u*>(s)[k];
                t[4 * k] = w.x; t[4 * k + 1] = w.y; t[4 * k + 2] = w.z; t[4 * k + 3] = w.w;
            }
            const bool rev = o.nc != 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ok[k] = true;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = rev ? t[3 * (3 - k) + ch] : t[3 * k + ch];
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
        int si, sj;
        da_blit_src<ADJ>(q, o, H, W, i, j0 + k, si, sj);
        ok[k] = da_blit_ok<ADJ>(q, H, W, i, j0 + k, si, sj);
        if (ok[k]) {
            const float* s = xb + ((size_t)si * W + sj) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = s[ch];
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = 0.f;
        }
    }
}

// The image mean from the sum pass's partials (every wave, fixed order, all lanes active), the colour term and the store: the
// arithmetic of diffaug_apply_kernel, operation by operation, so an image without a flip or a turn comes out with the same bits.
__device__ __forceinline__ float da_blit_mean(const float* __restrict__ part, int nparts, int b, int H, int W) {
    const int lane = threadIdx.x & (WAVE - 1);
    float t = 0.f;
    for (int k = lane; k < nparts; k += WAVE) t += part[(size_t)b * nparts + k];
    return wave_sum(t) / (3.f * (float)H * (float)W);
}

template <int P, bool ADJ>
__device__ __forceinline__ void da_blit_finish(float (&v)[3 * P], const bool (&ok)[P], const DaImg& q, int policy, float M, int with_bias,
                                               float* __restrict__ d) {
    if (policy & DA_COLOR) {
        const float cs = q.c * q.s, k0 = (1.f - q.c) * M + (with_bias && !ADJ ? q.b : 0.f);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const float m = (v[3 * k] + v[3 * k + 1] + v[3 * k + 2]) * (1.f / 3.f);
            const float cm = q.c * m + k0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float o = cs * (v[3 * k + ch] - m) + cm;
                v[3 * k + ch] = (ADJ || ok[k]) ? o : 0.f;
            }
        }
    }
    if (P == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<float4*>(d)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * P; ++k) d[k] = v[k];
    }
}

// The sum pass of a blit launch: diffaug_sum_kernel's body, statement for statement (a sum does not see a permutation, so it sums the
// same values in the same order), with the draws a row stride apart and the gates optional (img_bits == NULL: the policy for every
// image).  Its own copy: sharing the body through a device function changes the code the compiler emits for diffaug_sum_kernel.
template <int P, int MODE>
__global__ __launch_bounds__(DA_BLOCK) void diffaug_blit_sum_kernel(const float* __restrict__ x, const float* __restrict__ u, int u_stride,
                                                                    float* __restrict__ part, int nparts, int H, int W, int policy,
                                                                    const int* __restrict__ img_bits) {
    const int b = blockIdx.y;
    if (img_bits) policy &= img_bits[b];
    if (!(policy & DA_COLOR)) return;                            // (block-uniform) nobody reads this image's partials
    const DaImg q = da_params(u + (size_t)u_stride * b, H, W, policy);
    const float* xb = x + (size_t)b * H * W * 3;
    const int upr = W / P, nunits = H * upr;
    constexpr int UPT = DA_PART_PIXELS / (DA_BLOCK * P);                               // units per thread
    float acc = 0.f;
#pragma unroll 4
    for (int it = 0; it < UPT; ++it) {
        const int unit = (blockIdx.x * UPT + it) * DA_BLOCK + threadIdx.x;
        if (unit < nunits) {
            const int i = unit / upr, j0 = (unit - i * upr) * P;
            float v[3 * P]; bool ok[P];
            da_load<P, MODE>(xb, H, W, i, j0, q, v, ok);
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 3 * P; ++k) s += v[k];
            acc += s;
        }
    }
    __shared__ float red[DA_BLOCK / WAVE];
    acc = wave_sum(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = red[0];
#pragma unroll
        for (int w = 1; w < DA_BLOCK / WAVE; ++w) t += red[w];
        part[(size_t)b * nparts + blockIdx.x] = t;
    }
}

// Row path: diffaug_apply_kernel with the orientation.  grid (ceil(units / DA_BLOCK), B).
template <int P, bool ADJ>
__global__ __launch_bounds__(DA_BLOCK) void diffaug_blit_row_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ u,
                                                                    int u_stride, const float* __restrict__ part, int nparts, int H, int W,
                                                                    int policy, int with_bias, const int* __restrict__ img_bits) {
    const int b = blockIdx.y;
    if (img_bits) policy &= img_bits[b];
    const float* ub = u + (size_t)u_stride * b;
    const int upr = W / P;
    const int unit = blockIdx.x * DA_BLOCK + threadIdx.x;
    const DaImg q = da_params(ub, H, W, policy);
    const DaOri o = da_orient(ub, policy, ADJ);
    float M = 0.f;
    if (policy & DA_COLOR) M = da_blit_mean(part, nparts, b, H, W);
    if (unit >= H * upr) return;
    const int i = unit / upr, j0 = (unit - i * upr) * P;
    float v[3 * P]; bool ok[P];
    da_load_blit<P, ADJ>(x + (size_t)b * H * W * 3, H, W, i, j0, q, o, v, ok);
    da_blit_finish<P, ADJ>(v, ok, q, policy, M, with_bias, y + (((size_t)b * H + i) * W + j0) * 3);
}

// Tile path (H == W, W % 4 == 0, 16-byte aligned bases): a block owns a DA_TILE x DA_TILE output tile.  Under every orientation the
// sources of the tile are a DA_TILE x DA_TILE square of the input (shifted, mirrored, turned: the index map is affine with unit steps),
// so the block reads that square row by row -- thread (r, c) the four pixels (r, 4c .. 4c+3), eight lanes a run of 384 contiguous
// bytes, three cache lines -- into LDS, and after one barrier every thread picks the four pixels of its output group out of LDS, along
// a row or along a column, and stores them as the row path does (three 16-byte stores).  Pixels outside the image are neither read nor
// staged; the output side tests the source before it reads LDS, so nothing unstaged is read.
//
// LDS row stride: 3 * DA_TILE + 3 = 99 floats, all accesses one float wide (the stride is odd, a pixel is 12 bytes: nothing wider
// is aligned).  A 4-byte LDS access is served in two groups of 32 lanes on 32 banks; 32 consecutive lanes are (r, c) = (r0 .. r0+3,
// 0 .. 7).  Staging writes float m of the group to r * 99 + 12 c + m: bank 3 r + 12 c (mod 32), r < 4, c < 8.  A row-wise read of
// pixel k, channel ch is at row * 99 + 3 (4 c + k) + ch: 3 r + 12 c again.  A column-wise read is at (4 c + k) * 99 + 3 r + ch, and
// 4 * 99 = 12 (mod 32): 3 r + 12 c a third time (a mirrored direction negates a term).  {12 c mod 32} = {0, 4, .., 28} and
// {3 r} = {0, 3, 6, 9} give 32 different banks: no access conflicts.  A stride that is a multiple of 4 (for 16-byte LDS accesses)
// would make 4 * stride a multiple of 16 and put the eight c of a column-wise read on two banks.
constexpr int DA_TILE = 32;
constexpr int DA_TILE_STRIDE = 3 * DA_TILE + 3;
static_assert(DA_TILE * DA_TILE == 4 * DA_BLOCK && DA_TILE == 4 * 8, "one group of four pixels per thread, eight groups per tile row");

template <bool ADJ>
__global__ __launch_bounds__(DA_BLOCK) void diffaug_blit_tile_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ u,
                                                                     int u_stride, const float* __restrict__ part, int nparts, int N, int tiles,
                                                                     int policy, int with_bias, const int* __restrict__ img_bits) {
    __shared__ float tile[DA_TILE * DA_TILE_STRIDE];
    const int b = blockIdx.y;
    if (img_bits) policy &= img_bits[b];
    const float* ub = u + (size_t)u_stride * b;
    const DaImg q = da_params(ub, N, N, policy);
    const DaOri o = da_orient(ub, policy, ADJ);
    float M = 0.f;
    if (policy & DA_COLOR) M = da_blit_mean(part, nparts, b, N, N);
    const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles;
    const int I0 = ti * DA_TILE, J0 = tj * DA_TILE;
    const int r = threadIdx.x >> 3, c = threadIdx.x & 7;
    int ra, ca, rb, cb;                                          // the source square: from the sources of two opposite corners
    da_blit_src<ADJ>(q, o, N, N, I0, J0, ra, ca);
    da_blit_src<ADJ>(q, o, N, N, I0 + DA_TILE - 1, J0 + DA_TILE - 1, rb, cb);
    const int sr0 = min(ra, rb), sc0 = min(ca, cb);
    const float* xb = x + (size_t)b * N * N * 3;
    {
        const int row = sr0 + r, col = sc0 + 4 * c;
        float* l = tile + r * DA_TILE_STRIDE + 12 * c;
        if (row >= 0 && row < N) {
            if (col >= 0 && col + 4 <= N) {
                const float* s = xb + ((size_t)row * N + col) * 3;                         // 4-byte aligned: the shift moves by whole pixels
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const f32x4u w = reinterpret_cast<const f32x4u*>(s)[k];
                    l[4 * k] = w.x; l[4 * k + 1] = w.y; l[4 * k + 2] = w.z; l[4 * k + 3] = w.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (col + k >= 0 && col + k < N) {
                        const float* s = xb + ((size_t)row * N + (col + k)) * 3;
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) l[3 * k + ch] = s[ch];
                    }
                }
            }
        }
    }
    __syncthreads();
    const int i = I0 + r, j0 = J0 + 4 * c;
    if (i >= N || j0 >= N) return;                               // the tile overhangs the image (N % 4 == 0: whole groups)
    float v[12]; bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int si, sj;
        da_blit_src<ADJ>(q, o, N, N, i, j0 + k, si, sj);
        ok[k] = da_blit_ok<ADJ>(q, N, N, i, j0 + k, si, sj);
        const float* l = tile + (si - sr0) * DA_TILE_STRIDE + (sj - sc0) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = ok[k] ? l[ch] : 0.f;
    }
    da_blit_finish<4, ADJ>(v, ok, q, policy, M, with_bias, y + (((size_t)b * N + i) * N + j0) * 3);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// What a call launches: da_plan decides it, da_run executes it, sgx_aug_plan reports it without launching
static inline int da_nparts(int H, int W) { return (int)(((size_t)H * W + DA_PART_PIXELS - 1) / DA_PART_PIXELS); }

extern "C" size_t sgx_diffaug_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * da_nparts(H, W) * sizeof(float);
}

static const char* const DA_NAME[] = {"diffaug", "diffaug_gated", "diffaug_blit"};         // by SGX_AUG_PLAN_DIFFAUG / _GATED / _BLIT

// The sum pass if the policy has colour, then one apply launch.  Four pixels (three 16-byte stores) per lane where rows split into
// whole groups of four and the bases are 16-byte aligned, else one.  A blit call takes the tile path wherever an image of the launch
// may be turned and groups of four are whole and aligned, the row path (four pixels per lane) without the rot90 bit, the row kernel
// per pixel for everything else.
static int da_plan(int entry, bool ptrs_ok, int B, int H, int W, int policy, int adjoint, bool aligned, AugPlan* p) {
    const char* name = DA_NAME[entry];
    const bool blit = entry == SGX_AUG_PLAN_BLIT;
    if (int rc = aug_check_images(name, ptrs_ok, B, H, W)) return rc;
    SGX_REQUIRE(policy >= 0 && policy <= (blit ? DA_OPS5 : DA_OPS3), SGX_EINVAL, "%s: policy bits %d", name, policy);
    SGX_REQUIRE(!(policy & DA_ROT90) || H == W, SGX_EINVAL, "%s: rot90 needs square images, got %dx%d", name, H, W);
    const bool vec = aug_vec4(W, aligned);
    const int P = vec ? 4 : 1, nparts = da_nparts(H, W), gated = entry == SGX_AUG_PLAN_GATED, adj = adjoint != 0;
    *p = AugPlan{};
    if (policy & DA_COLOR) p->l[p->n++] = AugLaunch{blit ? AUG_K_BLIT_SUM : AUG_K_SUM, P, adj ? DA_ADJ : DA_PLAIN, gated, 0, nparts, B, nparts};
    if (blit && vec && (policy & DA_ROT90)) {
        const int tiles = (W + DA_TILE - 1) / DA_TILE;
        p->l[p->n++] = AugLaunch{AUG_K_BLIT_TILE, 0, adj, 0, 0, tiles * tiles, B, nparts, tiles};
    } else {
        p->l[p->n++] = AugLaunch{blit ? AUG_K_BLIT_ROW : AUG_K_APPLY, P, adj, gated, 0, aug_grid((size_t)H * (W / P)), B, nparts};
    }
    return 0;
}

// f(P, M, G): a launch's template arguments as integral constants, M of the list Ms
template <int... Ms, typename F> static void da_by_targs(const AugLaunch& l, F f) {
    sgx_by_int<1, 4>(l.P, [&](auto p) { sgx_by_int<Ms...>(l.mode, [&](auto m) { sgx_by_int<0, 1>(l.gated, [&](auto g) { f(p, m, g); }); }); });
}

struct DaCall {
    const float *x; float* y; const float* u; int u_stride; const int* img_bits;
    int B, H, W, policy, adjoint, with_bias; void* ws; size_t ws_bytes; void* stream;
};

static int da_run(int entry, const DaCall& c) {
    const char* name = DA_NAME[entry];
    AugPlan p;
    if (int rc = da_plan(entry, c.x && c.y && c.u && (entry != SGX_AUG_PLAN_GATED || c.img_bits), c.B, c.H, c.W, c.policy, c.adjoint, aug_aligned(c.x, c.y), &p))
        return rc;
    SGX_REQUIRE(entry != SGX_AUG_PLAN_BLIT || c.u_stride >= 9, SGX_EINVAL, "%s: draws %d floats apart, need at least 9", name, c.u_stride);
    if (int rc = aug_check_out_of_place(name, c.x, c.y, " (the passes gather)")) return rc;
    if (c.policy & DA_COLOR)
        if (int rc = aug_check_ws(name, c.ws, c.ws_bytes, sgx_diffaug_ws_bytes(c.B, c.H, c.W))) return rc;
    hipStream_t st = (hipStream_t)c.stream;
    float* part = (float*)c.ws;
    const int B = c.B, H = c.H, W = c.W;
    const char *dir = c.adjoint ? "adj" : "fwd", *tag = entry == SGX_AUG_PLAN_GATED ? "_gated" : "";
    for (int i = 0; i < p.n; ++i) {
        const AugLaunch& l = p.l[i];
        const dim3 grid(l.gx, l.gy), block(DA_BLOCK);
        switch (l.kernel) {
        case AUG_K_SUM:
            SGX_NOTE(0.0, 12.0 * B * H * W, "diffaug_sum%s B%d %dx%d %s", tag, B, H, W, dir);
            da_by_targs<DA_PLAIN, DA_ADJ>(l, [&](auto P, auto M, auto G) {
                hipLaunchKernelGGL((diffaug_sum_kernel<P(), M(), bool(G())>), grid, block, 0, st, c.x, c.u, part, l.nparts, H, W, c.policy, c.img_bits);
            });
            break;
        case AUG_K_APPLY:
            SGX_NOTE(0.0, 24.0 * B * H * W, "diffaug%s B%d %dx%d %s", tag, B, H, W, dir);
            da_by_targs<0, 1>(l, [&](auto P, auto M, auto G) {
                hipLaunchKernelGGL((diffaug_apply_kernel<P(), bool(M()), bool(G())>), grid, block, 0, st, c.x, c.y, c.u, (const float*)part, l.nparts, H, W, c.policy,
                                   c.with_bias, c.img_bits);
            });
            break;
        case AUG_K_BLIT_SUM:
            SGX_NOTE(0.0, 12.0 * B * H * W, "diffaug_blit_sum B%d %dx%d %s", B, H, W, dir);
            da_by_targs<DA_PLAIN, DA_ADJ>(l, [&](auto P, auto M, auto) {
                hipLaunchKernelGGL((diffaug_blit_sum_kernel<P(), M()>), grid, block, 0, st, c.x, c.u, c.u_stride, part, l.nparts, H, W, c.policy, c.img_bits);
            });
            break;
        case AUG_K_BLIT_ROW:
            SGX_NOTE(0.0, 24.0 * B * H * W, "diffaug_blit_%s B%d %dx%d %s", l.P == 4 ? "row" : "px", B, H, W, dir);
            da_by_targs<0, 1>(l, [&](auto P, auto M, auto) {
                hipLaunchKernelGGL((diffaug_blit_row_kernel<P(), bool(M())>), grid, block, 0, st, c.x, c.y, c.u, c.u_stride, (const float*)part, l.nparts, H, W,
                                   c.policy, c.with_bias, c.img_bits);
            });
            break;
        case AUG_K_BLIT_TILE:
            SGX_NOTE(0.0, 24.0 * B * H * W, "diffaug_blit_tile B%d %dx%d %s", B, H, W, dir);
            sgx_by_int<0, 1>(l.mode, [&](auto M) {
                hipLaunchKernelGGL((diffaug_blit_tile_kernel<bool(M())>), grid, block, 0, st, c.x, c.y, c.u, c.u_stride, (const float*)part, l.nparts, W, l.tiles,
                                   c.policy, c.with_bias, c.img_bits);
            });
            break;
        }
    }
    SGX_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int sgx_diffaug(const float* x, float* y, const float* u, int B, int H, int W, int policy_bits, int adjoint, int with_bias,
                           void* ws, size_t ws_bytes, void* stream) {
    return da_run(SGX_AUG_PLAN_DIFFAUG, DaCall{x, y, u, 7, nullptr, B, H, W, policy_bits, adjoint, with_bias, ws, ws_bytes, stream});
}

extern "C" int sgx_diffaug_gated(const float* x, float* y, const float* u, const int* img_bits, int B, int H, int W, int policy_bits, int adjoint,
                                 int with_bias, void* ws, size_t ws_bytes, void* stream) {
    return da_run(SGX_AUG_PLAN_GATED, DaCall{x, y, u, 7, img_bits, B, H, W, policy_bits, adjoint, with_bias, ws, ws_bytes, stream});
}

extern "C" int sgx_diffaug_blit(const float* x, float* y, const float* u, int u_stride, const int* img_bits, int B, int H, int W, int policy_bits,
                                int adjoint, int with_bias, void* ws, size_t ws_bytes, void* stream) {
    return da_run(SGX_AUG_PLAN_BLIT, DaCall{x, y, u, u_stride, img_bits, B, H, W, policy_bits, adjoint, with_bias, ws, ws_bytes, stream});
}

extern "C" int sgx_aug_plan(int entry, int B, int H, int W, int policy_bits, int adjoint, int with_bias, int aligned, int* out) {
    SGX_REQUIRE(out, SGX_EINVAL, "aug_plan: out is NULL");
    for (int i = 0; i < SGX_AUG_PLAN_INTS; ++i) out[i] = 0;
    SGX_REQUIRE(entry >= SGX_AUG_PLAN_DIFFAUG && entry <= SGX_AUG_PLAN_COLOR, SGX_EINVAL, "aug_plan: entry %d", entry);
    AugPlan p;
    if (int rc = entry == SGX_AUG_PLAN_GEOM    ? dg_plan(true, B, H, W, adjoint, aligned != 0, &p)
                 : entry == SGX_AUG_PLAN_COLOR ? dc_plan(true, B, H, W, adjoint, with_bias, aligned != 0, &p)
                                               : da_plan(entry, true, B, H, W, policy_bits, adjoint, aligned != 0, &p))
        return rc;
    out[0] = p.n;
    for (int i = 0; i < p.n; ++i) {
        const AugLaunch& l = p.l[i];
        const int v[] = {l.kernel, l.P, l.mode, l.gated, l.bias, l.gx, l.gy, l.nparts, l.tiles, l.HW};
        for (int k = 0; k < 10; ++k) out[1 + 10 * i + k] = v[k];
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ADA: the per-image gates and the controller (definitions in include/sgx.h)
constexpr int ADA_BLOCK = 256;

__global__ __launch_bounds__(ADA_BLOCK) void ada_gates_kernel(const float* __restrict__ gu, const float* __restrict__ state, int* __restrict__ img_bits,
                                                              int policy, int B) {
    const int b = blockIdx.x * ADA_BLOCK + threadIdx.x;
    if (b >= B) return;
    const float p = state[0];
    const int on = (gu[3 * b] < p ? DA_COLOR : 0) | (gu[3 * b + 1] < p ? DA_TRANSLATION : 0) | (gu[3 * b + 2] < p ? DA_CUTOUT : 0);
    img_bits[b] = policy & on;
}

extern "C" int sgx_ada_gates(const float* gu, const float* state, int policy_bits, int* img_bits, int B, void* stream) {
    SGX_REQUIRE(gu && state && img_bits && B > 0, SGX_EINVAL, "ada_gates: bad arguments (B=%d)", B);
    SGX_REQUIRE(policy_bits >= 0 && policy_bits <= DA_OPS3, SGX_EINVAL, "ada_gates: policy bits %d", policy_bits);
    SGX_NOTE(0.0, 16.0 * B, "ada_gates B%d", B);
    hipLaunchKernelGGL(ada_gates_kernel, dim3((B + ADA_BLOCK - 1) / ADA_BLOCK), dim3(ADA_BLOCK), 0, (hipStream_t)stream, gu, state, img_bits,
                       policy_bits, B);
    SGX_LAUNCH_CHECK("ada_gates");
    return 0;
}

// The gates of up to five ops: column g of a row of gu (rows gu_stride floats apart) gates bit 1 << g.
__global__ __launch_bounds__(ADA_BLOCK) void ada_gates_n_kernel(const float* __restrict__ gu, int gu_stride, int n_ops, const float* __restrict__ state,
                                                                int* __restrict__ img_bits, int policy, int B) {
    const int b = blockIdx.x * ADA_BLOCK + threadIdx.x;
    if (b >= B) return;
    const float p = state[0];
    const float* g = gu + (size_t)gu_stride * b;
    int on = 0;
    for (int k = 0; k < n_ops; ++k) on |= g[k] < p ? 1 << k : 0;
    img_bits[b] = policy & on;
}

extern "C" int sgx_ada_gates_n(const float* gu, int gu_stride, int n_ops, const float* state, int policy_bits, int* img_bits, int B, void* stream) {
    SGX_REQUIRE(gu && state && img_bits && B > 0, SGX_EINVAL, "ada_gates_n: bad arguments (B=%d)", B);
    SGX_REQUIRE(n_ops >= 1 && n_ops <= 5 && gu_stride >= n_ops, SGX_EINVAL, "ada_gates_n: %d ops, rows %d floats apart", n_ops, gu_stride);
    SGX_REQUIRE(policy_bits >= 0 && policy_bits < (1 << n_ops), SGX_EINVAL, "ada_gates_n: policy bits %d for %d ops", policy_bits, n_ops);
    SGX_NOTE(0.0, (4.0 * n_ops + 4.0) * B, "ada_gates_n B%d", B);
    hipLaunchKernelGGL(ada_gates_n_kernel, dim3((B + ADA_BLOCK - 1) / ADA_BLOCK), dim3(ADA_BLOCK), 0, (hipStream_t)stream, gu, gu_stride, n_ops, state,
                       img_bits, policy_bits, B);
    SGX_LAUNCH_CHECK("ada_gates_n");
    return 0;
}

// One block.  The signs are summed as integers (exact, so the order is immaterial: thread t takes logits t, t + 256, ..., the wave and
// block sums follow); thread 0 then updates the state, every product and sum rounded to fp32 on its own.
__global__ __launch_bounds__(ADA_BLOCK) void ada_update_kernel(const float* __restrict__ logits, int B, float* __restrict__ state, float target,
                                                               float adjust_per_image, int interval) {
    int acc = 0;
    for (int k = threadIdx.x; k < B; k += ADA_BLOCK) {
        const float v = logits[k];
        acc += (v > 0.f) - (v < 0.f);                            // +-0 and NaN: 0
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ int red[ADA_BLOCK / WAVE];
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int total = red[0];
#pragma unroll
    for (int w = 1; w < ADA_BLOCK / WAVE; ++w) total += red[w];
    const float signs = __fadd_rn(state[1], (float)total);
    const float seen = __fadd_rn(state[2], (float)B);
    const float calls = __fadd_rn(state[3], 1.f);
    if (calls >= (float)interval) {
        const float rt = __fdiv_rn(signs, seen);
        const float dir = rt > target ? 1.f : (rt < target ? -1.f : 0.f);     // sign(r_t - target) without forming the difference
        const float p = __fadd_rn(state[0], __fmul_rn(dir, __fmul_rn(adjust_per_image, seen)));
        state[0] = fminf(fmaxf(p, 0.f), 1.f);
        state[1] = 0.f; state[2] = 0.f; state[3] = 0.f;
        state[4] = rt;
        state[5] = __fadd_rn(state[5], 1.f);
    } else {
        state[1] = signs; state[2] = seen; state[3] = calls;
    }
}

extern "C" int sgx_ada_update(const float* real_logits, int B, float* state, float target, float adjust_per_image, int interval, void* stream) {
    SGX_REQUIRE(real_logits && state && B > 0 && B <= (1 << 24) && interval > 0, SGX_EINVAL, "ada_update: bad arguments (B=%d interval=%d)", B, interval);
    SGX_REQUIRE(target > 0.f && target < 1.f && adjust_per_image >= 0.f, SGX_EINVAL, "ada_update: target %g, adjust %g", (double)target,
                (double)adjust_per_image);
    SGX_NOTE(0.0, 4.0 * B + 64.0, "ada_update B%d", B);
    hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(ADA_BLOCK), 0, (hipStream_t)stream, real_logits, B, state, target, adjust_per_image, interval);
    SGX_LAUNCH_CHECK("ada_update");
    return 0;
}
