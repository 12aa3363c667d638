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
#include "common.h"

enum { DA_COLOR = 1, DA_TRANSLATION = 2, DA_CUTOUT = 4 };
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

static inline int da_nparts(int H, int W) { return (int)(((size_t)H * W + DA_PART_PIXELS - 1) / DA_PART_PIXELS); }

template <int P, bool GATED>
static void da_launch(const float* x, float* y, const float* u, const int* img_bits, float* part, int B, int H, int W, int policy, int adjoint,
                      int with_bias, hipStream_t st) {
    const int nparts = da_nparts(H, W);
    const char* tag = GATED ? "_gated" : "";
    if (policy & DA_COLOR) {
        SGX_NOTE(0.0, 12.0 * B * H * W, "diffaug_sum%s B%d %dx%d %s", tag, B, H, W, adjoint ? "adj" : "fwd");
        if (adjoint) hipLaunchKernelGGL((diffaug_sum_kernel<P, DA_ADJ, GATED>), dim3(nparts, B), dim3(DA_BLOCK), 0, st, x, u, part, nparts, H, W, policy, img_bits);
        else hipLaunchKernelGGL((diffaug_sum_kernel<P, DA_PLAIN, GATED>), dim3(nparts, B), dim3(DA_BLOCK), 0, st, x, u, part, nparts, H, W, policy, img_bits);
    }
    const unsigned gx = (unsigned)(((size_t)H * (W / P) + DA_BLOCK - 1) / DA_BLOCK);
    SGX_NOTE(0.0, 24.0 * B * H * W, "diffaug%s B%d %dx%d %s", tag, B, H, W, adjoint ? "adj" : "fwd");
    if (adjoint) hipLaunchKernelGGL((diffaug_apply_kernel<P, true, GATED>), dim3(gx, B), dim3(DA_BLOCK), 0, st, x, y, u, (const float*)part, nparts, H, W, policy, with_bias, img_bits);
    else hipLaunchKernelGGL((diffaug_apply_kernel<P, false, GATED>), dim3(gx, B), dim3(DA_BLOCK), 0, st, x, y, u, (const float*)part, nparts, H, W, policy, with_bias, img_bits);
}

extern "C" size_t sgx_diffaug_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * da_nparts(H, W) * sizeof(float);
}

template <bool GATED>
static int da_run(const char* name, const float* x, float* y, const float* u, const int* img_bits, int B, int H, int W, int policy_bits, int adjoint,
                  int with_bias, void* ws, size_t ws_bytes, void* stream) {
    SGX_REQUIRE(x && y && u && (!GATED || img_bits) && B > 0 && H > 0 && W > 0 && B <= 65535, SGX_EINVAL, "%s: bad arguments (B=%d %dx%d)", name, B, H, W);
    SGX_REQUIRE((size_t)H * W * 3 < (size_t)1 << 31, SGX_EUNSUPPORTED, "%s: image of %dx%d too large", name, H, W);
    SGX_REQUIRE(policy_bits >= 0 && policy_bits <= (DA_COLOR | DA_TRANSLATION | DA_CUTOUT), SGX_EINVAL, "%s: policy bits %d", name, policy_bits);
    SGX_REQUIRE(x != y, SGX_EINVAL, "%s: in place is not supported (the passes gather)", name);
    if (policy_bits & DA_COLOR)
        SGX_REQUIRE(ws && ws_bytes >= sgx_diffaug_ws_bytes(B, H, W), SGX_EWORKSPACE, "%s: workspace %zu < %zu bytes", name, ws_bytes,
                    sgx_diffaug_ws_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    // four pixels (three 16-byte stores) per lane where rows split into whole groups of four and the bases are 16-byte aligned
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    if (vec) da_launch<4, GATED>(x, y, u, img_bits, (float*)ws, B, H, W, policy_bits, adjoint, with_bias, st);
    else da_launch<1, GATED>(x, y, u, img_bits, (float*)ws, B, H, W, policy_bits, adjoint, with_bias, st);
    SGX_LAUNCH_CHECK(name);
    return 0;
}

extern "C" int sgx_diffaug(const float* x, float* y, const float* u, int B, int H, int W, int policy_bits, int adjoint, int with_bias,
                           void* ws, size_t ws_bytes, void* stream) {
    return da_run<false>("diffaug", x, y, u, nullptr, B, H, W, policy_bits, adjoint, with_bias, ws, ws_bytes, stream);
}

extern "C" int sgx_diffaug_gated(const float* x, float* y, const float* u, const int* img_bits, int B, int H, int W, int policy_bits, int adjoint,
                                 int with_bias, void* ws, size_t ws_bytes, void* stream) {
    return da_run<true>("diffaug_gated", x, y, u, img_bits, B, H, W, policy_bits, adjoint, with_bias, ws, ws_bytes, stream);
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
    SGX_REQUIRE(policy_bits >= 0 && policy_bits <= (DA_COLOR | DA_TRANSLATION | DA_CUTOUT), SGX_EINVAL, "ada_gates: policy bits %d", policy_bits);
    SGX_NOTE(0.0, 16.0 * B, "ada_gates B%d", B);
    hipLaunchKernelGGL(ada_gates_kernel, dim3((B + ADA_BLOCK - 1) / ADA_BLOCK), dim3(ADA_BLOCK), 0, (hipStream_t)stream, gu, state, img_bits,
                       policy_bits, B);
    SGX_LAUNCH_CHECK("ada_gates");
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
