/* sgx.h -- C ABI of libsgx_hip.so: the MI355X (gfx950) kernels behind the StyleGAN G+D training hot path.
 *
 * The reference (huangzh13/StyleGAN.pytorch) is pure Python and has no FFI: its seam for this path is the
 * nn.Module surface of models/CustomLayers.py, models/Blocks.py and models/GAN.py.  Every entry point below
 * replaces one composition of PyTorch ops that those modules issue; the comment above each one cites it
 * (file:line relative to the reference root).  stylegan/pytorch_amd/native.py binds them with ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers.
 *   - activations are NHWC ("channels last"): x[b][h][w][c].  dtype: SGX_F32 or SGX_BF16 storage
 *     (accumulation is always fp32).  Parameters, statistics, RGB images and gradients of parameters are fp32.
 *   - `stream` is a hipStream_t passed as void*; the library never allocates, frees or synchronises.
 *     Scratch memory is supplied by the caller (`ws`, `ws_bytes`; query with the *_ws_bytes functions).
 *   - every function returns 0 on success, a negative SGX_E* code for argument errors, or a positive
 *     hipError_t; sgx_last_error() returns a thread-local message.  Nothing throws or aborts.
 *   - re-entrant: no global mutable state (backward runs on autograd worker threads).
 */
#ifndef SGX_H
#define SGX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { SGX_F32 = 0, SGX_BF16 = 1 };
/* LeakyReLU(0.2) / ReLU: the 'lrelu' | 'relu' nonlinearity of models/GAN.py:67-68,150-151,346-347.  The fused epilogues of
 * the convolution / linear kernels implement NONE and LRELU (what every shipped config uses); RELU is served by
 * sgx_bias_act + sgx_lrelu_bwd(slope 0) after the un-activated kernel.                                               */
enum { SGX_ACT_NONE = 0, SGX_ACT_LRELU = 1, SGX_ACT_RELU = 2 };
enum { SGX_EINVAL = -1, SGX_EUNSUPPORTED = -2, SGX_EWORKSPACE = -3 };

int sgx_version(void);
const char* sgx_last_error(void);
int sgx_clear_error(void);          /* forget the message and HIP's sticky last error (returns it); after a failed capture */
/* Stream ordering without a host object per fork: `waiter` waits for all work enqueued on `signaler` so far (pooled
 * events inside the library; valid during stream capture, where it becomes a graph edge).  Replaces the
 * torch.cuda.Stream.wait_stream calls a multi-stream implementation of models/GAN.py:595-655 would make.            */
int sgx_stream_wait_stream(void* waiter, void* signaler);
/* Hardware self-test of ds_read_b64_tr_b16 (the transpose read of the bf16 weight-gradient kernel): with lds[e] = e and
 * lane l addressing elements [4l,4l+4), writes the 4 int16 values each of the 64 lanes received to out256.          */
int sgx_selftest_tr16(void* out256, void* stream);

/* ---- per-launch profiler.  Every kernel the library launches can be bracketed by two HIP events recorded on the launch
 * stream itself.  sgx_prof_start(1, 0): record every launch (clears earlier records); (2, i): record only launches of
 * the kernel that record i belongs to; (0, 0): stop, keeping the records.  sgx_prof_get waits for record i and returns
 * the demangled kernel name (as rocprofv3 prints it), the milliseconds between its events, and the flops, algorithmic
 * bytes and layer description attached by the entry point that launched it (0 / "" when it attached none).
 * sgx_prof_get_launch returns record i's launch geometry as the runtime was given it: grid3 and block3 take x, y, z,
 * lds the dynamic LDS bytes (any of the three may be NULL); it waits for nothing. */
int sgx_prof_start(int mode, int only_of);
int sgx_prof_count(void);
int sgx_prof_get(int i, char* name, int name_cap, float* ms, double* flops, double* bytes, char* desc, int desc_cap);
int sgx_prof_get_launch(int i, unsigned* grid3, unsigned* block3, size_t* lds);

/* ---------------------------------------------------------------- convolutions (MFMA implicit GEMM)
 * Packed weight layout for all three: w[tap][n][k], n = output channel of THIS launch, k = reduction
 * channel, k contiguous; dtype = activation dtype.  bias (fp32, may be NULL) and act are fused in the store.
 *
 * sgx_conv3x3: EqualizedConv2d plain path, F.conv2d(x, W*w_mul, b, padding=1) -- models/CustomLayers.py:170-171;
 *   also its data gradient (call with the flipped/transposed pack).
 *   y[b,h,w,n] = act(bias[n] + sum_{ty,tx,k} x[b,h+ty-1,w+tx-1,k] * w[ty*3+tx][n][k])
 *   mask (may be NULL; a tensor shaped and typed like y): y *= (mask > 0 ? 1 : 0.2) in the store.  As a DATA-GRADIENT launch
 *   of a layer whose input is the LeakyReLU output of the layer below (DiscriminatorBlock conv0 after the previous block's
 *   conv1_down + act, models/Blocks.py:140-146), that is the activation's autograd applied where the gradient is produced
 *   instead of in a pass of its own; bit-identical to sgx_lrelu_bwd on the stored result.                              */
int sgx_conv3x3(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                int act, const void* mask, int dtype, void* stream);
/* sgx_conv4x4s2_down: fused conv+downscale, F.conv2d(x, W4, stride=2, padding=1) -- models/CustomLayers.py:158-165
 *   (== conv3x3 -> avg_pool2 of :166-168); also the data gradient of sgx_conv4x4s2_up.
 *   H,W = input size.  y[b,oy,ox,n] = act(bias[n] + sum_{ky,kx,k} x[b,2oy+ky-1,2ox+kx-1,k] * w[ky*4+kx][n][k])    */
int sgx_conv4x4s2_down(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin,
                       int Cout, int act, int dtype, void* stream);
/* sgx_conv4x4s2_up: fused upscale+conv, F.conv_transpose2d(x, W4, stride=2, padding=1) -- models/CustomLayers.py:143-152
 *   (== nearest-up -> conv3x3 of :153-154 with the kernel flipped); also the data gradient of
 *   sgx_conv4x4s2_down.  H,W = input (coarse) size, output is 2H x 2W.
 *   y[b,iy,ix,n] = sum over (oy,ky),(ox,kx) with 2oy+ky-1=iy, 2ox+kx-1=ix of x[b,oy,ox,k] * w[ky*4+kx][n][k]      */
int sgx_conv4x4s2_up(const void* x, const void* w, void* y, int B, int H, int W, int Cin, int Cout, int dtype,
                     void* stream);
/* Any of the three convolutions with the kernel generation named by the caller (A/B probes and parity tests of both).
 *   geo 0: sgx_conv3x3, 1: sgx_conv4x4s2_down, 2: sgx_conv4x4s2_up (H, W = input size; geo 2 takes no bias / activation);
 *   variant 0: first-generation kernel (16x16 MFMA tiles, register-staged single LDS stage; any shape / dtype);
 *   variant 4 / 8: second-generation bf16 kernel (32x32x16 MFMA, LDS-DMA double-buffered stages; the stride-2 convolution
 *   as four polyphase 2x2 convolutions, the transposed one with its four output-parity classes in one block) with 4- / 8-wave
 *   blocks; needs Cin % 32 == 0, Cout % 32 == 0 (64 for geo 0) and a tile-grid width % 32 == 0 (SGX_EUNSUPPORTED otherwise).
 *   The three entry points above choose by themselves.                                                               */
int sgx_conv_variant(int geo, const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                     int act, int dtype, int variant, void* stream);
/* Round 6: split-K for the bf16 stride-2 launches that leave most of the chip idle (the 512-channel conv1_down layers at 16x16 -> 8x8 and
 * 8x8 -> 4x4 of a small batch: 32-128 blocks, each walking 16 K-chunks behind a global-load latency).  sgx_conv_splitk_ws_bytes: 0 = the shape
 * does not split (call sgx_conv3x3 / sgx_conv4x4s2_down / sgx_conv4x4s2_up; always 0 for geo 0 and 2, whose split forms were measured no better
 * and are not built), else the bytes of fp32 partials [ksplit][output pixel][Cout] sgx_conv_splitk needs.  sgx_conv_splitk: geo 1 =
 * sgx_conv4x4s2_down's convolution (models/CustomLayers.py:160-171; bias and act as there, mask NULL), the reduction over input channels split
 * over ksplit <= 8 blocks, the partials summed in a fixed order by a second launch.  Other geometries: SGX_EUNSUPPORTED. */
size_t sgx_conv_splitk_ws_bytes(int geo, int B, int H, int W, int Cin, int Cout, int dtype);
int sgx_conv_splitk(int geo, const void* x, const void* w, const float* bias, void* y, const void* mask, int B, int H, int W, int Cin, int Cout,
                    int act, int dtype, void* ws, size_t ws_bytes, void* stream);

/* Host-only query: the launch configuration a convolution of this shape resolves to (geo 0: 3x3, 1: 4x4s2 down,
 * 2: 4x4s2 up; H,W = input size).  cfg5 = {KC, TH, TW, pixels per block, output-channel sub-tiles}: the template
 * arguments of conv_kernel<T, KC, geo, TH, TW, BP, CT> as rocprofv3 prints them.  geo 2 answers for the per-class
 * transposed kernel; geo 3: the 4x4s2 up convolution as its launch runs it -- the bf16 launch without deep K-chunks
 * runs the all-class kernel (printed as geo 3), whose configuration differs; every other launch: as geo 2.          */
int sgx_conv_config(int geo, int B, int H, int W, int Cin, int Cout, int dtype, int* cfg5);
/* sgx_pack_weight: runtime weight scaling + operand packing (`self.weight * self.w_mul` and the 3x3 -> 4x4 kernel
 * synthesis of models/CustomLayers.py:146-150,159-162) in one launch.  w: parameter [O][I][3][3] fp32.
 * Writes BOTH operand packs of the layer in the activation dtype: fwd[taps][O][Ipad] (the layer's convolution) and
 * adj[taps][Ipad][O] (its data gradient; 3x3 taps reversed).  Ipad >= I zero-pads the input-channel axis.
 *   S : scale*w                      -> sgx_conv3x3 / adj: sgx_conv3x3
 *   D : 0.25*scale*sum4shifts(w)     -> sgx_conv4x4s2_down / adj: sgx_conv4x4s2_up
 *   U : scale*sum4shifts(w)          -> sgx_conv4x4s2_up / adj: sgx_conv4x4s2_down    (fused upscale, input >= 64)
 *   UF: as U on the spatially flipped kernel (== nearest-up -> conv3x3 of the non-fused branch)       */
enum { SGX_PACK_S = 0, SGX_PACK_D = 1, SGX_PACK_U = 2, SGX_PACK_UF = 3 };
int sgx_pack_weight(const float* w, void* fwd, void* adj, int O, int I, int Ipad, int mode, float scale, int dtype,
                    void* stream);
/* the same for n parameters in ONE launch (all stale weights of a network after its optimizer step).  table: device
 * array of n rows of SGX_PACK_ROW 64-bit words  [w, fwd, adj, O, I, Ipad, mode, scale as fp32 bits, first block, blocks],
 * rows sorted by first block, blocks = sgx_pack_weight_blocks(O, Ipad), total_blocks = their sum; all packs in `dtype`. */
#define SGX_PACK_ROW 10
int sgx_pack_weight_blocks(int O, int Ipad);          /* blocks one parameter needs (32 x 32 channel tiles) */
int sgx_pack_weight_multi(const void* table, int n, int total_blocks, int dtype, void* stream);
/* weight gradients in the PARAMETER layout dW[O][I][3][3] (fp32): MFMA pixel-reduction into split partials (ws), then
 * one finishing kernel that sums the splits and applies the adjoint of sgx_pack_weight (autograd of F.conv2d /
 * F.conv_transpose2d w.r.t. weight composed with the reference's weight arithmetic).
 *   sgx_wgrad3x3_param : y = conv3x3(x, pack_S(w)):  x has Cx channels, dy has Cdy.  adjoint=1: the launch was the
 *                        layer's DATA-GRADIENT convolution (x: O channels, dy: Ipad channels) -- second-order path (R1).
 *   sgx_wgrad4x4s2_param: fine/coarse = the stride-2 pair's high/low resolution tensors (H,W = fine size);
 *                        mode D: coarse has O channels, fine has I;  mode U/UF: coarse has I, fine has O.
 *   db (nullable, fp32 [O]): also the bias gradient sum_{b,h,w} dy[.,o] (EqualizedConv2d bias, CustomLayers.py:178),
 *                        from the same pass over dy (one extra MFMA against a tile of ones) -- only where dy is the
 *                        O-channel side: adjoint=0 / mode D; otherwise SGX_EINVAL.
 *   accumulate           bit 0: dW += result, bit 1: db += result (a parameter used by several passes of one backward --
 *                        D on real and fake images, the R1 double backward -- accumulates in the finishing kernel
 *                        instead of a separate add per contribution).                                               */
size_t sgx_wgrad_ws_bytes(int taps, int B, int H, int W, int Ck, int Cn);
/* Host-only query: what a weight-gradient call of this shape and workspace will launch (taps 9: sgx_wgrad3x3_param, 16: sgx_wgrad4x4s2_param; H, W, Ck = Cx /
 * Cfine, Cn = Cdy / Ccoarse as those take them).  The launchers run the same plan.  out[SGX_WGRAD_PLAN_INTS] = {generation 1 / 2; TH, TW, BP, NSUB, KSUB, TR:
 * the template arguments of wgrad_kernel<T, geo, ...> as rocprofv3 prints them (generation 2: the pixel tile TH x TW = BP, NSUB 0, KSUB = the kernel's KBW,
 * 16 for wgrad16_s_kernel); pixel splits; the splits the finishing launch reads (0: no finishing launch, the gradient kernel writes dW / db itself);
 * pre-reduction 0 / 1; the finishing kernel's EPB}.  Returns the call's error code: 0, SGX_EUNSUPPORTED, SGX_EWORKSPACE. */
#define SGX_WGRAD_PLAN_INTS 11
int sgx_wgrad_plan(int taps, int B, int H, int W, int Ck, int Cn, int dtype, size_t ws_bytes, int* out);
int sgx_wgrad3x3_param(const void* x, const void* dy, float* dW, float* db, void* ws, size_t ws_bytes, int B, int H, int W,
                       int Cx, int Cdy, int adjoint, float scale, int O, int I, int accumulate, int dtype, void* stream);
int sgx_wgrad4x4s2_param(const void* fine, const void* coarse, float* dW, float* db, void* ws, size_t ws_bytes, int B, int H,
                         int W, int Cfine, int Ccoarse, int mode, float scale, int O, int I, int accumulate, int dtype,
                         void* stream);

/* ---------------------------------------------------------------- memory-bound layer pieces
 * y = act(x + bscale*bias[c])               bias after blur / avgpool: models/CustomLayers.py:178-179; Blocks.py:142,146
 *   bscale = the layer's b_mul (lrmul; 0.01 in the mapping network, models/CustomLayers.py:94-95,101-102)           */
int sgx_bias_act(const void* x, const float* bias, float bscale, void* y, size_t npix, int C, int act, int dtype,
                 void* stream);
/* dx = scale * dy * (y > 0 ? 1 : slope)     autograd of nn.LeakyReLU(0.2) (slope 0.2) / torch.relu (slope 0); y is the
 * activation OUTPUT.  scale (1 = none; scale_dev != NULL: read from device memory instead) folds the fade-in coefficient of
 * the branch the activation sits on (x = alpha*straight + (1-alpha)*residual, models/GAN.py:427) into the same pass    */
int sgx_lrelu_bwd(const void* dy, const void* y, void* dx, size_t n, float slope, float scale, const float* scale_dev, int dtype,
                  void* stream);
/* sgx_lrelu_bwd with y given as sign bits (1 bit per element, bits[i] = the 8 channels of 16-byte vector i); bf16 */
int sgx_lrelu_bwd_bits(const void* dy, const void* bits, void* dx, size_t n, float slope, float scale, const float* scale_dev, int dtype,
                       void* stream);
/* The newest discriminator block's tail in one kernel (models/Blocks.py:143-146 + models/GAN.py:425-427): the stride-2 convolution,
 * its bias and LeakyReLU, and the fade-in lerp with the residual branch:  y = alpha * lrelu(conv(x) + bias) + beta * resid  (resid shaped
 * like y; the lerp is applied to the bf16-rounded activation, exactly as sgx_axpby on the stored tensor).  bits [B][H/2][W/2][Cout/8]:
 * the sign bits of the activation -- its LeakyReLU-backward mask (sgx_lrelu_bwd_bits); the activation itself is not stored.
 * _ok: 1 if the shape has the variant (bf16, second-generation stride-2 kernel), else sgx_conv4x4s2_down + sgx_axpby. */
int sgx_conv4x4s2_down_fade_ok(int B, int H, int W, int Cin, int Cout, int dtype);
int sgx_conv4x4s2_down_fade(const void* x, const void* w, const float* bias, const void* resid, float alpha, float beta, const float* ab_dev,
                            void* y, void* bits, int B, int H, int W, int Cin, int Cout, int dtype, void* stream);
/* Round 5: the same with the residual branch resid = from_rgb(pimg) (models/GAN.py:423-427: the 1x1 convolution of the DOWN-SAMPLED image)
 * evaluated in the store: resid[p][c] = bf16((rb[c] * bs1) * bs2 + (r * (ws * wr[c][0]) + g * (ws * wr[c][1])) + b * (ws * wr[c][2])), (r, g, b) =
 * pimg[p] -- sgx_rgb_in's arithmetic, bit for bit; pimg fp32 [B][H/2][W/2][3], wr = from_rgb.weight [Cout][3], ws = its w_mul (x the
 * residual's prescale), rb = from_rgb.bias or NULL.  sgx_fade_rgb_bwd is the backward of that tail in ONE pass over g = dL/dy:
 * gy = (alpha g) slope(bits) (bit for bit sgx_lrelu_bwd_bits), dwr / drb (written, or accumulated per bit 0 / 1 of acc; NULL = skipped) =
 * beta ws sum_p g pimg resp. beta bs sum_p g, and (gpimg != NULL) gpimg[p][j] = beta ws sum_c g[p][c] wr[c][j]; alpha / beta from the call
 * or ab_dev[0], ab_dev[1]; ws: sgx_fade_rgb_bwd_ws_bytes.  bf16, C in {32, 64, 128}. */
int sgx_conv4x4s2_down_fade_rgb(const void* x, const void* w, const float* bias, const float* pimg, const float* wr, float ws, const float* rb,
                                float bs1, float bs2, float alpha, float beta, const float* ab_dev, void* y, void* bits, int B, int H, int W,
                                int Cin, int Cout, int dtype, void* stream);
size_t sgx_fade_rgb_bwd_ws_bytes(size_t npix, int C);
int sgx_fade_rgb_bwd(const void* g, const void* bits, const float* pimg, const float* wr, float ws, float bs, float alpha, float beta,
                     const float* ab_dev, void* gy, float* dwr, float* drb, int acc, float* gpimg, void* wsbuf, size_t ws_bytes, size_t npix, int C,
                     int dtype, void* stream);    /* ab_dev (nullable): [alpha, beta] in device memory instead (graph replay) */
/* Round 6: the parameter-gradient half on its own -- after a sgx_fade_rgb_bwd call with dwr = drb = NULL (which leaves the block partials in
 * wsbuf), on any stream ordered behind it: the step accumulates EVERY .grad on one side stream (two backward branches of the D step run on
 * different streams and both reach from_rgb of the residual branch). */
int sgx_fade_rgb_bwd_finish(const void* wsbuf, size_t ws_bytes, size_t npix, int C, float ws, float bs, float beta, const float* ab_dev,
                            float* dwr, float* drb, int acc, void* stream);
/* Round 6: the adjoint of sgx_fade_rgb_bwd's data half (gy, gpimg as functions of g) -- what the R1 double backward needs of this tail -- in one
 * pass: out = bf16(t1 + t2), t1 = bf16((alpha ggy) slope(bits)) (sgx_lrelu_bwd_bits on ggy), t2 = bf16(sgx_rgb_in(ggp; wr, ws)) [ab_dev: then
 * bf16(beta t2)]: the roundings of the three passes it replaces are kept, the result is theirs bit for bit.  ggy or ggp may be NULL.  A host
 * beta rides in ws (pass 1).  bf16, C in {32, 64, 128}. */
int sgx_fade_rgb_bwd2(const void* ggy, const float* ggp, const void* bits, const float* wr, float ws, float alpha, float beta, const float* ab_dev,
                      void* out, size_t npix, int C, int dtype, void* stream);
/* out = alpha*a + beta*b (b may be NULL)    fade-in lerp: models/GAN.py:202,427,586                                 */
int sgx_axpby(const void* a, const void* b, void* out, float alpha, float beta, size_t n, int dtype, void* stream);
/* same with the coefficients read from device memory (alpha_dev[0], beta_dev[0]): the fade-in alpha changes every
 * iteration (models/GAN.py:744), so a captured hipGraph of the step must not bake it into kernel arguments */
int sgx_axpby_dev(const void* a, const void* b, void* out, const float* alpha_dev, const float* beta_dev, size_t n, int dtype,
                  void* stream);
/* depthwise [1,2,1]x[1,2,1]/16 blur, zero pad   BlurLayer: models/CustomLayers.py:251-276 (self-adjoint)           */
int sgx_blur3x3(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
/* "LeakyReLU(0.2) then blur" (discriminator block, models/Blocks.py:140-142) with the activation folded into the blur pass:
 * mode 0: y = blur(x);  1: y = blur(lrelu(x))  [forward];  2: y = blur(x) * slope(z)  [backward: z = the pre-activation];
 * 3: y = blur(x * slope(z))  [backward of mode 2 w.r.t. x: the R1 double backward].  slope(z) = z > 0 ? 1 : 0.2 */
int sgx_blur3x3_act(const void* x, const void* z, void* y, int B, int H, int W, int C, int mode, int dtype, void* stream);
/* modes 2 / 3 with z as SIGN BITS: bits[pixel][C/8] bytes, bit j of byte v = (z[8v + j] > 0), as sgx_conv3x3_signbits writes them:
 * the backward passes of the block read 1 bit per mask element instead of 16 (bf16 only). */
int sgx_blur3x3_bits(const void* x, const void* bits, void* y, int B, int H, int W, int C, int mode, int dtype, void* stream);
/* BlurLayer with any other filter (models/CustomLayers.py:251-276: kernel = outer(f,f) [/sum] [flipped], F.conv2d with
 * groups=C, padding (K-1)//2):  y[oy][ox] = sum_{i,j} taps[i*K+j] * x[oy+i-pad][ox+j-pad], zero outside, K <= 7.
 * taps_host: K*K floats in HOST memory (copied into the launch).  x: [B][IH][IW][C], y: [B][OH][OW][C] with
 * OH <= IH+2*pad-K+1.  The adjoint is the same call with the taps flipped, pad' = K-1-pad and the sizes swapped.      */
int sgx_blur_kxk(const void* x, void* y, const float* taps_host, int K, int pad, int B, int IH, int IW, int OH, int OW, int C,
                 int dtype, void* stream);
/* Input pipeline on the device: uint8 images -> NHWC activations, (v/255 - 0.5)/0.5 in fp32 -- torchvision's
 * ToTensor + Normalize((.5,.5,.5),(.5,.5,.5)) of data/transforms.py:20-33; flip[b] != 0 mirrors image b horizontally
 * (RandomHorizontalFlip, decision drawn by the caller; NULL: none).  src: [B][H][W][3] bytes, or [B][3][H][W] if src_chw.
 * W must be a multiple of 4.                                                                                          */
int sgx_images_u8_to_nhwc(const void* src, void* dst, const int* flip, int B, int H, int W, int src_chw, int dtype, void* stream);
/* y = scale * (2x2 block sum)   scale .25: AvgPool2d(2) models/GAN.py:382,423; Downscale2d CustomLayers.py:60-64   */
int sgx_pool2(const void* x, void* y, int B, int H, int W, int C, float scale, int dtype, void* stream);
/* y = scale * nearest_up2(x)    Upscale2d CustomLayers.py:27-36; F.interpolate(scale_factor=2) models/GAN.py:173     */
int sgx_up2(const void* x, void* y, int B, int H, int W, int C, float scale, int dtype, void* stream);
/* Round 6: y = a + scale * nearest-up(x), a and y shaped [B][2H][2W][C] -- the adjoint of the 2x2 pool AND the sum with the other gradient of
 * a tensor that feeds both a full-resolution branch and a pooled one (the discriminator's image: models/GAN.py:423-427), one pass.     */
int sgx_up2_add(const void* x, const void* a, void* y, int B, int H, int W, int C, float scale, int dtype, void* stream);
/* out[c] = scale * sum_p x[p][c]  (fp32 out)        bias gradient                                                    */
size_t sgx_colsum_ws_bytes(size_t npix, int C);
int sgx_colsum(const void* x, float* out, float scale, void* ws, size_t ws_bytes, size_t npix, int C, int dtype,
               void* stream);

/* 1x1 RGB convolutions; images are fp32 [p][3].  The weight is read IN PLACE from the parameter: element (j = rgb
 * channel, c = feature channel) is w[j*sj + c*sc] * wscale (wscale = w_mul); from_rgb parameters are [C][3][1][1]
 * (sj=1, sc=3), to_rgb parameters are [3][C][1][1] (sj=C, sc=1).
 *   sgx_rgb_in : y[p][c] = bias[c] + sum_j img[p][j]*W(j,c)      from_rgb: models/GAN.py:358-359,377-378,425-426
 *   sgx_rgb_out: img[p][j] = bias[j] + sum_c x[p][c]*W(j,c)      to_rgb:   models/GAN.py:157,167,199-200
 *   sgx_rgb_wgrad: dw[j*sj + c*sc] = wscale * sum_p img[p][j]*f[p][c]   (gradient in the parameter layout)          */
int sgx_rgb_in(const float* img, const float* w, int sj, int sc, float wscale, const float* bias, void* y, size_t npix,
               int C, int dtype, void* stream);
int sgx_rgb_out(const void* x, const float* w, int sj, int sc, float wscale, const float* bias, float* img, size_t npix,
                int C, int dtype, void* stream);
/* Round 6: y = add + sgx_rgb_in(img) (no bias; add and y shaped [npix][C] of `dtype`): to_rgb's data gradient joined with the gradient the
 * forked activation got from its other consumer (models/GAN.py:199-202 under fade-in), one pass, one rounding.                          */
int sgx_rgb_in_add(const float* img, const float* w, int sj, int sc, float wscale, const void* add, void* y, size_t npix, int C, int dtype,
                   void* stream);
size_t sgx_rgb_wgrad_ws_bytes(size_t npix, int C);
/* The same 1x1 layers for images that are not RGB (csrc/imgconv.hip): J image channels, images fp32 [p][J], the weight read in place
 * with element (j, c) at w[j*sj + c*sc] * wscale (from_rgb [C][J][1][1]: sj=1, sc=J; to_rgb [J][C][1][1]: sj=C, sc=1).  J = 1, 2, 4
 * (num_channels of a grayscale / two-channel / RGBA model) and 8 (the conditional discriminator's from_rgb over [RGBA image, label
 * embedding], models/GAN.py:326-330, and its adjoint).  C % 4 == 0 (fp32) / C % 8 == 0 (bf16), anything else is
 * SGX_EUNSUPPORTED before any launch; img aligned to 4 J bytes (16 for J = 8), activations to 16.
 *   sgx_img_in : y[p][c] = bias[c] + wscale * sum_j img[p][j]*W(j,c)     from_rgb forward, to_rgb data gradient:
 *                                                                        models/GAN.py:358-359,377-378 (adjoint of :157,167)
 *   sgx_img_out: img[p][j] = bias[j] + wscale * sum_c x[p][c]*W(j,c)     to_rgb forward, from_rgb data gradient, the R1 inner gradient:
 *                                                                        models/GAN.py:157,167 (adjoint of :358-359,377-378)
 *   sgx_img_wgrad: dw[j*sj + c*sc] = wscale * sum_p img[p][j]*f[p][c]    both layers' weight gradient, in the parameter layout; fp64
 *                  partials per block finished in a fixed order (no atomics): the same bits at every run.  ws: sgx_img_wgrad_ws_bytes. */
int sgx_img_in(const float* img, const float* w, int J, int sj, int sc, float wscale, const float* bias, void* y, size_t npix, int C, int dtype,
               void* stream);
int sgx_img_out(const void* x, const float* w, int J, int sj, int sc, float wscale, const float* bias, float* img, size_t npix, int C, int dtype,
                void* stream);
size_t sgx_img_wgrad_ws_bytes(size_t npix, int J, int C);
int sgx_img_wgrad(const float* img, const void* f, float* dw, int J, int sj, int sc, float wscale, void* ws, size_t ws_bytes, size_t npix, int C,
                  int dtype, void* stream);
/* sgx_images_u8_to_nhwc for J = 1..4 channels (data/transforms.py:20-33 on grayscale / RGBA data): src [B][H][W][J] bytes, or [B][J][H][W]
 * if src_chw; the same arithmetic in the same order, so J = 3 gives the bits of the 3-channel entry point.  Any W (a multiple of 4 takes
 * the vector kernel). */
int sgx_images_u8_to_nhwc_c(const void* src, void* dst, const int* flip, int B, int H, int W, int J, int src_chw, int dtype, void* stream);
/* real images at the current depth with the fade-in blend (models/GAN.py:575-586): out = alpha * x + beta *
 * nearest_up2(avgpool2(x)) on fp32 [B][H][W][3] in one pass; ab_dev as in sgx_rgb_out_fade. */
int sgx_downsample_fade_rgb(const float* x, float* out, int B, int H, int W, float alpha, float beta, const float* ab_dev, void* stream);
/* DiffAugment (Zhao et al., NeurIPS 2020) of the discriminator's input: fp32 [B][H][W][3] images, policy_bits a subset of
 * 1 = color, 2 = translation, 4 = cutout, applied in that order; u: DEVICE fp32 [B][7] uniform draws in [0,1) per image.
 *   color: b = u0 - 0.5, s = 2 u1, c = u2 + 0.5;  L x = c s (x - m_x) + c (m_x - M_x) + M_x (m_x: mean over the 3 channels of a
 *          pixel, M_x: mean over the image), the DiffAugment brightness / saturation / contrast chain in closed form.
 *   translation: sh = int(H/8 + 0.5), tx = min(floor(u3 (2 sh + 1)), 2 sh) - sh (ty from u4 and W), the product in fp32;
 *          y[i][j] = x[i + tx][j + ty] inside the image, 0 outside.
 *   cutout: ch = int(H/2 + 0.5), ox = min(floor(u5 (H + 1 - ch%2)), H - ch%2) (oy from u6 and W); rows [ox - ch/2, ox - ch/2 + ch) x
 *          the same columns of the output are 0.
 * adjoint = 0: y = Mask(Shift(L x + b)) (b only if with_bias);  adjoint = 1: y = L(Shift^T(Mask x)) (the transpose of the linear part).
 * Gathers only (x != y), no atomics: bit-reproducible.  ws: sgx_diffaug_ws_bytes(B, H, W) bytes, read only when color is on (the
 * per-image sums).  Replaces DiffAugment's rand_brightness / rand_saturation / rand_contrast / rand_translation / rand_cutout.   */
size_t sgx_diffaug_ws_bytes(int B, int H, int W);
int sgx_diffaug(const float* x, float* y, const float* u, int B, int H, int W, int policy_bits, int adjoint, int with_bias, void* ws,
                size_t ws_bytes, void* stream);
/* Adaptive discriminator augmentation (Karras et al., NeurIPS 2020) on the DiffAugment kernels: every op is applied to an image with
 * probability p, and p is steered on the device from r_t = E[sign(D(real))] towards a target.
 *   state: DEVICE fp32 [8] = { p, sum of signs, images counted, calls since the last update, last r_t, updates made, 0, 0 }.
 * sgx_ada_gates: gu DEVICE fp32 [B][3] uniforms in [0,1);  img_bits[b] (int32 [B]) = policy_bits & (1 [gu[b][0] < p] | 2 [gu[b][1] < p] |
 *   4 [gu[b][2] < p]) with p = state[0] read on the device and strict < in fp32: p = 0 gates nothing, p = 1 everything.  The bits are
 *   made once per D evaluation; every later pass of that evaluation (adjoint, linear part, R1 double backward) reads them, never p.
 * sgx_diffaug_gated: sgx_diffaug with image b transformed under (policy_bits & img_bits[b]) instead of one policy for the batch;
 *   policy_bits (the union) only decides whether the sum pass is launched; workspace as for sgx_diffaug.  An image whose bits are 0 is
 *   copied bit-exactly (forward and adjoint); an image without the colour bit does no arithmetic on its values (gathers and zeros).
 * sgx_ada_update: one block.  S = sum over b of sign(real_logits[b]) (+1 / -1; 0 for +-0 and NaN), summed as an integer and converted
 *   to fp32.  With every product and sum rounded to fp32 on its own:  state[1] += S;  state[2] += B;  state[3] += 1;  and when state[3]
 *   >= interval:  r_t = state[1] / state[2];  p = min(max(p + sign(r_t - target) * (adjust_per_image * state[2]), 0), 1) (the sign by
 *   comparing r_t with target: 0 when equal);  state[4] = r_t;  state[5] += 1;  state[1..3] = 0.  adjust_per_image = 1 / (ada_kimg *
 *   1000) as computed by the caller.  B <= 2^24.  Replaces the augment pipe's p buffer and the training loop's host-side heuristic. */
int sgx_ada_gates(const float* gu, const float* state, int policy_bits, int* img_bits, int B, void* stream);
int sgx_diffaug_gated(const float* x, float* y, const float* u, const int* img_bits, int B, int H, int W, int policy_bits, int adjoint,
                      int with_bias, void* ws, size_t ws_bytes, void* stream);
int sgx_ada_update(const float* real_logits, int B, float* state, float target, float adjust_per_image, int interval, void* stream);
/* Pixel blitting, the first augmentation group of the ADA paper, fused into the gather of the kernels above: policy_bits a subset of
 * 1 = color, 8 = xflip, 16 = rot90, 2 = translation, 4 = cutout, applied in that order.  u: DEVICE fp32, row b at u + b * u_stride
 * (u_stride >= 9): u0..u6 as for sgx_diffaug, and
 *   xflip: f = min(floor(2 u7), 1);  rot90: k = min(floor(4 u8), 3), the products in fp32; an op that is absent from the policy or
 *          gated off for the image gives f = 0 / k = 0 whatever its uniform is.
 *   orientation G = Rot^k o Flip, in torch terms on [3][H][W]:  G(x) = rot90(flip(x, [2]) if f else x, k, [1, 2]);  with N = H = W
 *          flip: out[i][j] = in[i][W-1-j];  k = 1: out[i][j] = in[j][N-1-i];  k = 2: out[i][j] = in[N-1-i][N-1-j];
 *          k = 3: out[i][j] = in[N-1-j][i].  G permutes the pixels, so G^T = G^-1 = Flip o Rot^-k.
 * adjoint = 0: y = Mask(Shift(G(L x + b))) (b only if with_bias);  adjoint = 1: y = L(G^T(Shift^T(Mask x))).  The colour stays innermost
 * (it commutes with G in exact arithmetic), so both per-image sums are those of sgx_diffaug, summed in its order, and an image with
 * f = 0 and k = 0 comes out bit-identical to sgx_diffaug / sgx_diffaug_gated under the same first seven draws.  As gathers:
 *   forward: output (i, j) -> cutout test at (i, j) -> shifted position (i + tx, j + ty), tested against the image -> the source
 *          pixel G^-1 of that position in x;
 *   adjoint: output (i, j) -> (a, b) = G(i, j) -> source (a - tx, b - ty) in x, tested against the image and the cutout there.
 * img_bits == NULL: the policy for every image; else image b is transformed under (policy_bits & img_bits[b]) as in sgx_diffaug_gated.
 * rot90 needs H == W (SGX_EINVAL, nothing launched); xflip works for any H, W.  x != y; workspace as sgx_diffaug_ws_bytes, read only
 * when color is on.  One apply launch per call, gathers only, no atomics: bit-reproducible.
 * sgx_ada_gates_n: sgx_ada_gates for n_ops <= 5 gate uniforms per image, row b at gu + b * gu_stride (gu_stride >= n_ops): column g gates
 *   policy bit 1 << g (1 color, 2 translation, 4 cutout, 8 xflip, 16 rot90), the same strict fp32 < against state[0] read on the device;
 *   policy_bits < 2^n_ops.  With the row strides one [B][14] draw serves both entries without a copy: u = r, u_stride = 14;
 *   gu = r + 9, gu_stride = 14.  Replaces the xflip, rot90 and integer-translation steps of the augment pipe's pixel blitting. */
int sgx_diffaug_blit(const float* x, float* y, const float* u, int u_stride, const int* img_bits, int B, int H, int W, int policy_bits,
                     int adjoint, int with_bias, void* ws, size_t ws_bytes, void* stream);
int sgx_ada_gates_n(const float* gu, int gu_stride, int n_ops, const float* state, int policy_bits, int* img_bits, int B, void* stream);
/* The general geometric transformations, the second augmentation group of the ADA paper: policy_bits a subset of 32 = scale,
 * 64 = rotate, 128 = aniso, applied in that order AFTER the ops above, composed per image into one affine map and applied by one
 * bilinear resample of fp32 [B][H][W][3] images.  u: DEVICE fp32, row b at u + b * u_stride (u_stride >= 5), five uniforms in [0,1):
 *   z_s = clamp(sqrt(-2 ln(1 - u0)) cos(2 pi u1), -3, 3);  s = 2^(0.2 z_s) when scale is on for the image, else 1
 *   theta = 2 pi (u2 - 0.5) when rotate is on, else 0
 *   z_a built like z_s from u3 and u4;  a = 2^(0.2 z_a) when aniso is on, else 1
 *   T = Rot(theta) diag(s a, s / a),  Rot(theta) = [cos -sin; sin cos],  acting on (column, row) about the centre c = ((W-1)/2, (H-1)/2)
 * (fp32, every product, quotient and difference rounded on its own; the precise logf / cosf / sinf / exp2f / sqrtf).  An op is on for
 * an image when its bit is in policy_bits and either gu == NULL or its gate uniform is strictly below p = state[0] read on the device:
 * gu row b at gu + b * gu_stride (gu_stride >= 3), columns 0..2 gating scale, rotate, aniso; gu and state are both given or both NULL.
 * sgx_ada_geom_matrix: one launch writes mat[b][0..3] = T^-1 and mat[b][4..7] = T (row major) of every image, fp32 [B][8].  An image
 *   whose three ops are all off gets exactly (1,0,0,1, 1,0,0,1): that row is the identity flag -- the resample copies such an image
 *   bit for bit.  Made once per D evaluation; the forward, the adjoint and the R1 double backward read the table, never p.
 * sgx_ada_geom: with s_p = c + T^-1 (p - c) for the pixel p = (column j, row i) and w(s, t) = max(0, 1 - |s_x - t_x|) max(0, 1 - |s_y - t_y|),
 *   adjoint = 0:  y(p) = sum over the taps t = floor(s_p) + {0,1}^2 inside the image of w(s_p, t) x(t); taps outside contribute zero
 *                 (the padding value of the integer translation), a pixel without a tap inside is +0;
 *   adjoint = 1:  y(q) = sum over the pixels p of the image of w(s_p, q) x(p), as a gather: the candidates p are the integers of the
 *                 bounding box of c + T (q - c + (-1,1)^2), at most 7 x 7 of them (the clamp of z at +-3 gives |T| entries <= 2.3).
 *   s_p and w are computed as  s_x = c_x + (m0 d_x + m1 d_y),  s_y = c_y + (m2 d_x + m3 d_y),  d = p - c,  and as written above, every
 *   product and sum rounded to fp32 on its own, by the same expression in both directions: the adjoint's coefficients are the forward's
 *   bit for bit (as fp32 matrices the two are exact transposes), and a float32 restatement reproduces them exactly.  Accumulation is
 *   acc += w * v, both roundings in fp32, taps in the order (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1), candidates row by row.
 *   x != y, any H, W >= 1, no workspace, gathers only, no atomics: bit-reproducible.  With W % 4 == 0 and 16-byte aligned bases
 *   a block resamples a 32 x 32 tile (and copies an identity image with 16-byte loads and stores).  Replaces the augment pipe's isotropic scale, arbitrary rotation and anisotropic scale (with bilinear
 *   taps instead of its band-limited filters; zero padding here, its reflection padding in sgx_ada_geom_reflect).
 * sgx_ada_geom_reflect: the same resample under the same table (sgx_ada_geom_matrix is shared) with REFLECTION padding.  Per axis of
 *   length N >= 2 a tap index t is valid iff -(N-1) <= t <= 2 (N-1) -- one reflection period, np.pad(mode="reflect") with pad N-1 --
 *   and a valid tap reads the pixel r(t) = -t for t < 0, 2 (N-1) - t for t > N-1, t otherwise.  The weight is taken at the UNREFLECTED
 *   t; a tap beyond one period contributes zero (the paper likewise clamps its margin to N-1 and samples zeros beyond it).
 *   adjoint = 0:  y(p) = sum over the valid taps t = floor(s_p) + {0,1}^2 of w(s_p, t) x(r(t)), taps in sgx_ada_geom's order; a pixel
 *                 with no valid tap is +0;
 *   adjoint = 1:  y(q) = sum_p sum over the valid taps t of p with r(t) = q of w(s_p, t) x(p), as a gather with no atomics.  Per axis
 *                 the pixel index q has up to three pre-images under r: q itself, -q when q >= 1, 2 (N-1) - q when q <= N-2 (distinct,
 *                 all inside the period), so up to nine unreflected positions q' per pixel.  For each q' the candidate box of
 *                 sgx_ada_geom's adjoint is walked with q' in place of q in both the box centre and the weight.  Summation order:
 *                 the mirrors row-major -- the row's (q, -q, 2 (H-1) - q) outer, the column's inner -- and within a mirror the
 *                 candidates row by row, into ONE fp32 accumulator that starts at +0.
 *   s_p, w and acc += w * v are sgx_ada_geom's expressions, so the adjoint's coefficients are the forward's bit for bit, and an
 *   image whose taps all stay inside the image gets sgx_ada_geom's bits in both directions.  An identity row is a bit-for-bit copy.
 *   x != y; H, W >= 2 (SGX_EINVAL below that); the other rejections are sgx_ada_geom's.  No workspace, no atomics, nothing written
 *   outside y.  With W % 4 == 0 and 16-byte aligned bases a block resamples a 32 x 32 tile, else a thread one pixel.
 * sgx_ada_geom_reflect_plan: host-only, what sgx_ada_geom_reflect will launch (the entry executes the same plan).  aligned: x and y are
 *   16-byte aligned.  out[SGX_ADA_GEOM_REFLECT_PLAN_INTS]: the number of launches (1), the kernel (0 ada_geom_reflect_px_kernel<ADJ>,
 *   1 ada_geom_reflect_tile_kernel<ADJ>), ADJ, grid x, grid y (= B), tiles of 32 x 32 pixels per row of tiles (0 for the px kernel);
 *   the block is 256 threads, no dynamic LDS.  Returns 0, or what the entry returns for these arguments (SGX_EINVAL: B outside
 *   1..65535, H or W < 2, a NULL out; SGX_EUNSUPPORTED: 3 H W >= 2^31); out is zeroed on every error but a NULL out. */
int sgx_ada_geom_matrix(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, float* mat, int B,
                        void* stream);
int sgx_ada_geom(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* stream);
int sgx_ada_geom_reflect(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* stream);
#define SGX_ADA_GEOM_REFLECT_PLAN_INTS 6
int sgx_ada_geom_reflect_plan(int B, int H, int W, int adjoint, int aligned, int* out);
/* The colour transformations, the third augmentation group of the ADA paper: policy_bits a subset of 256 = brightness, 512 = contrast,
 * 1024 = lumaflip, 2048 = hue, 4096 = saturation, applied in that order AFTER the ops above, composed per image into one affine map of
 * the RGB vector of fp32 [B][H][W][3] images.  u: DEVICE fp32, row b at u + b * u_stride (u_stride >= 8), eight uniforms in [0,1); with
 * z(ua, ub) = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3):
 *   b = 0.2 z(u0, u1) when brightness is on for the image, else 0
 *   c = 2^(0.5 z(u2, u3)) when contrast is on, else 1
 *   sigma = 1 - 2 min(floor(2 u4), 1) when lumaflip is on (-1 for u4 >= 0.5), else 1
 *   theta = 2 pi (u5 - 0.5) when hue is on, else 0
 *   s = 2^(z(u6, u7)) when saturation is on, else 1
 * With v = (1,1,1)/sqrt(3), P = v v^T and K = (1/sqrt(3)) [0 -1 1; 1 0 -1; -1 1 0] (the cross-product matrix of v) the map is the paper's
 * composition Sat Hue Luma Contrast Brightness of each pixel's RGB vector x:
 *   y = M x + t,   M = c [sigma P + s (cos(theta) (I - P) + sin(theta) K)],   t = c sigma b (1,1,1).
 * M is circulant, rows (D L U), (U D L), (L U D):  D = a + 2 (d/3),  L = (a - d/3) - e,  U = (a - d/3) + e  with  a = (c sigma)/3,
 * d = (c s) cos(theta),  e = ((c s) sin(theta)) * 0.57735027  (fp32, every product, quotient, sum and difference rounded on its own as
 * bracketed; the precise logf / cosf / sinf / exp2f / sqrtf; cos = 1 and sin = 0 exactly when hue is off; t = (c sigma) * b).  Pixels
 * that the earlier stages zeroed (the padding of the translation and of the resample, the cutout) are transformed like any other and
 * come out as t.  An op is on for an image when its bit is in policy_bits and either gu == NULL or its gate uniform is strictly below
 * p = state[0] read on the device: gu row b at gu + b * gu_stride (gu_stride >= 5), columns 0..4 gating brightness, contrast, lumaflip,
 * hue, saturation; gu and state are both given or both NULL.
 * sgx_ada_color_matrix: one launch writes mat[b][0..8] = M (row major) and mat[b][9..11] = t of every image, fp32 [B][12].  Exact rows:
 *   an image with all five ops off gets exactly (1,0,0, 0,1,0, 0,0,1, 0,0,0): that row is the identity flag -- the pass copies such an
 *   image bit for bit; an image without a flip (lumaflip off, or on with sigma = 1), with hue and saturation off gets exactly c on the
 *   diagonal and +0 off it (a branch, not 1/3 + 2/3); with theta = 0 (hue off) e is +0, so L == U bit for bit: a flip alone gives a
 *   symmetric row.  Made once per D evaluation; the forward, the linear part, the adjoint and the R1 double backward read the table,
 *   never p.
 * sgx_ada_color: x != y, any H, W >= 1, one pass over the batch;
 *   adjoint = 0:  y_k = ((M_k0 x_0 + M_k1 x_1) + M_k2 x_2) (+ t_k when with_bias)
 *   adjoint = 1:  y_k = ((M_0k x_0 + M_1k x_1) + M_2k x_2); with_bias must be 0
 *   every product and sum rounded to fp32 on its own in that order, so a float32 restatement reproduces the output bit for bit and the
 *   adjoint's coefficients are the forward's.  An image whose row compares equal to the identity row is copied instead, bit for bit
 *   (-0, infinities and NaN payloads included, which 1 x + 0 x' would not preserve).  No workspace, no atomics, nothing written
 *   outside y.  With H W % 4 == 0 and 16-byte aligned bases a lane owns four consecutive pixels (three 16-byte loads and stores),
 *   else one. */
int sgx_ada_color_matrix(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, float* mat, int B,
                         void* stream);
int sgx_ada_color(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, int with_bias, void* stream);
/* Image-space filtering, the fourth augmentation group of the ADA paper: policy bit 8192 = imgfilter, applied AFTER the colour ops
 * above (after them in the canonical order) to fp32 [B][H][W][3] images; pixels that the earlier stages zeroed are filtered like any others.
 * The filter bank is constant, 4 bands x 43 taps, built once in fp64 on the host:
 *   lo = [(1 - sqrt 3), (3 - sqrt 3), (3 + sqrt 3), (1 + sqrt 3)] / (4 sqrt 2)  (the sym2 low-pass),  hi[k] = lo[k] (-1)^k,
 *   lo2 = (lo * reverse(lo)) / 2,  hi2 = (hi * reverse(hi)) / 2  (7 taps each);  fb starts as the 4 x 1 column (1,0,0,0)^T; for i = 1, 2, 3:
 *   zero-stuff every row (length n -> 2 n - 1), convolve every row with lo2, add hi2 to the centre seven taps of row i (row lengths
 *   1 -> 7 -> 19 -> 43); taps with |v| < 1e-12 are set to exactly 0.  Every row is symmetric about tap 21, the rows have 37, 37, 15 and
 *   5 non-zero taps, the four rows sum to the unit impulse at tap 21, fb[0] sums to 1 and the other rows to 0.  The kernels hold the
 *   rows rounded to fp32 as half-rows fbh[4][22], fbh[i][j] = fb[i][21 + j]: the symmetry is structural.
 * u: DEVICE fp32, row b at u + b * u_stride (u_stride >= 8), eight uniforms in [0,1); with the variate of the groups above,
 * z(ua, ub) = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3), the band gains start from g = (1,1,1,1) and for band i = 0..3 in order:
 *   t = (1,1,1,1);  t[i] = 2^z(u[2i], u[2i+1]) when the band is on for the image, else 1;  t <- t / sqrt(mean(t^2));  g <- g t elementwise
 * (the paper's power-preserving normalisation with imgfilter_std = 1 and band strengths (1,1,1,1); fp32: n = sqrt(0.25 (3 + t_i t_i)),
 * g_k <- g_k * ((k == i ? t_i : 1) / n), every product, sum and quotient rounded on its own, the precise logf / cosf / exp2f / sqrtf; a
 * band that is off gives n = 1 and t = (1,1,1,1) exactly).  Band i is on when imgfilter is in policy_bits and either gu == NULL (all four
 * on) or its gate uniform is strictly below p = state[0] read on the device: gu row b at gu + b * gu_stride (gu_stride >= 4), columns
 * 0..3 gating the bands on their own, as the paper does; gu and state are both given or both NULL.
 * sgx_ada_filter_matrix: one launch writes the half-row c[j] = ((g_0 fbh[0][j] + g_1 fbh[1][j]) + g_2 fbh[2][j]) + g_3 fbh[3][j],
 *   j = 0..21, of every image, fp32 [B][22]; the filter is h[k] = c[|k - 21|].  An image whose four bands are all off (and every image
 *   when policy_bits lacks 8192) gets (1, 0, ..., 0) by a branch, not by the sum:
 *   that row is the identity flag -- the passes copy such an image bit for bit.  Made once per D evaluation; the forward, the adjoint
 *   and the R1 double backward read the table, never p.
 * sgx_ada_filter: per image and per channel y = A_v A_h x, along an axis of length N
 *     (A x)[i] = sum_{k = 0..42} h[k] x[refl_N(i + k - 21)],
 *   refl whole-sample reflection continued periodically: with P = 2 (N - 1) and m = q mod P (non-negative), refl = m if m < N, else
 *   P - m -- np.pad(mode="reflect") for any pad width; defined for N >= 2, so H < 2 or W < 2 is refused.  At N >= 22 a sample has at
 *   most 3 padded positions folding onto it, at N = 4 it has 15, at N = 2 it has 22.
 *   adjoint = 1:  y = A_h^T A_v^T x as a gather, no atomics:
 *     (A^T g)[j] = sum_{q in [-21, N + 20], refl(q) = j} sum_{i in [0, N)} h[q - i + 21] g[i],   h = 0 outside 0..42.
 *   The op has no bias, so its linear part is itself.  Every output of one axis is computed as
 *     acc = c[0] v(0);  acc = fma(c[j], v(+j) + v(-j), acc) for j = 1..21   (fp32, the sum rounded, then one fused multiply-add)
 *   with v(d) = x[refl(i + d)] in the forward and, in the adjoint, the zero-extended g at q + d, the q of one j summed in ascending
 *   order -- by every kernel, so the launch paths agree bit for bit.  One axis per launch: the forward filters along W into the
 *   workspace and then along H, the adjoint along H and then along W.  ws: sgx_ada_filter_workspace_bytes(B, H, W) = 12 B H W bytes
 *   (the image between the two axes), 16-byte aligned, apart from x and y; x != y.  With W % 4 == 0, 16-byte aligned x and y and
 *   H, W >= 44 a block stages a tile (16 rows x 64 pixels, or 64 rows x 64 floats) and its 21-sample halo through LDS, the reflection
 *   applied while staging, and a lane filters four consecutive outputs; else one output float per thread, any number of reflections.
 *   An image whose row compares equal to the identity row is copied instead, bit for bit (-0, infinities and NaN payloads included).
 * sgx_ada_filter_plan: host-only, what sgx_ada_filter will launch (the entry executes the same plan).  aligned: x and y are 16-byte
 *   aligned.  out[SGX_ADA_FILTER_PLAN_INTS]: [0] the number of launches (2), then six ints per launch, in launch order: the kernel
 *   (0 ada_filter_px_kernel<AXIS, ADJ>, 1 ada_filter_tile_kernel<AXIS, ADJ>), AXIS (0 along W, 1 along H), ADJ, grid x, grid y (= B),
 *   tiles per row of tiles (0 for the general kernel); every block is 256 threads, no launch has dynamic LDS.  Returns 0, or what the
 *   entry returns for these arguments (SGX_EINVAL: B outside 1..65535, H or W < 2, a NULL out; SGX_EUNSUPPORTED: 3 H W >= 2^31); out is
 *   zeroed on every error but a NULL out. */
int sgx_ada_filter_matrix(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, float* mat, int B,
                          void* stream);
size_t sgx_ada_filter_workspace_bytes(int B, int H, int W);
int sgx_ada_filter(const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* ws, size_t ws_bytes, void* stream);
#define SGX_ADA_FILTER_PLAN_INTS 13
int sgx_ada_filter_plan(int B, int H, int W, int adjoint, int aligned, int* out);
/* Image-space corruptions, the last augmentation group of the ADA paper: policy_bits a subset of 16384 = noise, 32768 = imgcutout,
 * applied in that order AFTER the filter above (last in the canonical order) to fp32 [B][H][W][3] images, as ONE pointwise pass
 *   y = M (x + sigma n),   n a standard normal field, M the diagonal 0/1 mask of one rectangle per image
 * (DiffAugment's own cutout, bit 4, is a different op: square, integer centre, applied before the geometric and colour stages; this
 * one leaves true zeros at D's input).  u: DEVICE fp32, row b at u + b * u_stride (u_stride >= 6), six uniforms in [0,1); an op is on
 * for an image when its bit is in policy_bits and either gu == NULL or its gate uniform is strictly below p = state[0] read on the
 * device: gu row b at gu + b * gu_stride (gu_stride >= 2), column 0 gating noise, column 1 the cutout, each on its own; gu and state
 * are both given or both NULL.
 * sgx_ada_corrupt_table: one launch writes tab[b] = (sigma, k0, k1, x0, x1, y0, y1, 0) of every image, fp32 [B][8].  With
 *   z(ua, ub) = clamp(sqrt(-2 ln(1 - ua)) cos(2 pi ub), -3, 3), the variate of the groups above:
 *   noise on:   sigma = 0.1f * fabsf(z(u0, u1))  (the paper's noise_std = 0.1 half-normal, with the clamp of z);
 *               k0 = min((uint32)(u2 * 16777216.0f), 16777215), k1 the same from u3: the field's key, stored as floats (exact: < 2^24)
 *   noise off:  sigma = k0 = k1 = +0
 *   cutout on:  with cx = u4 (columns), cy = u5 (rows), every product, sum and difference rounded to fp32 on its own:
 *               a = cx * W,  q = 0.25f * W,  x0 = max(0, (int)floorf((a - q) - 0.5f) + 1),  x1 = min(W, (int)ceilf((a + q) - 0.5f)),
 *               y0, y1 the same from cy and H; stored as floats.  The cut pixels are rows y0 <= i < y1 by columns x0 <= j < x1 (none
 *               when x0 >= x1 or y0 >= y1): the paper's mask |(j + 0.5) / W - cx| < cutout_size / 2 with cutout_size = 0.5, up to fp32
 *               rounding at the rectangle's edge
 *   cutout off: x0 = x1 = y0 = y1 = +0
 *   An image with both ops off (and every image when policy_bits is 0) gets the all-zero row exactly.  H, W >= 1.  Made once per D
 *   evaluation; the forward, the linear part and the R1 double backward read the table, never p.
 * sgx_ada_corrupt: x != y, any H, W >= 1 (3 H W >= 2^31: SGX_EUNSUPPORTED), B in 1..65535, one launch, no workspace, no atomics, nothing
 *   written outside y.
 *   mode 0, the forward:  a cut pixel is +0 in all three channels; elsewhere y = x + sigma * n when sigma != 0 (the product rounded to
 *           fp32, then the sum: no contraction) and the bits of x when sigma == 0
 *   mode 1, the linear part, which is its own adjoint (A = A^T = M):  a cut pixel is +0, elsewhere the bits of x (-0, infinities and
 *           NaN payloads included)
 *   An image whose rectangle is empty and whose sigma == 0 is copied bit for bit in both modes.  The noise of image b: for the flat
 *   element e = (i W + j) 3 + c let q = e >> 2, r = e & 3 and
 *     (o0, o1, o2, o3) = Philox4x32-10(counter (q, 0, 0, 0), key (k0, k1))      multipliers 0xD2511F53, 0xCD9E8D57; key increments
 *                                                                               0x9E3779B9, 0xBB67AE85
 *     for m = 0, 1:  ua = (o_2m >> 8) 2^-24,  ub = (o_2m+1 >> 8) 2^-24,  rad = sqrtf(-2 logf(1 - ua)),  (s, c) = sincospif(2 ub),
 *                    n_2m = rad c,  n_2m+1 = rad s
 *   element e takes n_r: no clamp, |n| <= sqrt(48 ln 2) ~ 5.77.  Nothing of the field is stored; two calls under one table give the
 *   same bits.  With H W % 4 == 0 and 16-byte aligned bases a lane owns four consecutive pixels of the image's flat pixel order (three
 *   16-byte loads and stores, the counters 3 g .. 3 g + 2 of its group g), else one pixel; both take a normal from the same function
 *   and agree bit for bit.  No Philox round and no transcendental runs for an image or a mode that needs none.
 * sgx_ada_corrupt_plan: host-only, what sgx_ada_corrupt will launch (the entry executes the same plan).  aligned: x and y are 16-byte
 *   aligned.  out[SGX_ADA_CORRUPT_PLAN_INTS]: the number of launches (1), the kernel (0 ada_corrupt_px_kernel<MODE>,
 *   1 ada_corrupt_vec_kernel<MODE>), MODE, grid x, grid y (= B); the block is 256 threads, no dynamic LDS.  Returns 0, or what the entry
 *   returns for these arguments (SGX_EINVAL: B outside 1..65535, H or W < 1, a mode outside 0, 1, a NULL out; SGX_EUNSUPPORTED:
 *   3 H W >= 2^31); out is zeroed on every error but a NULL out. */
int sgx_ada_corrupt_table(const float* u, int u_stride, const float* gu, int gu_stride, const float* state, int policy_bits, int H, int W,
                          float* tab, int B, void* stream);
int sgx_ada_corrupt(const float* x, float* y, const float* tab, int B, int H, int W, int mode, void* stream);
#define SGX_ADA_CORRUPT_PLAN_INTS 5
int sgx_ada_corrupt_plan(int B, int H, int W, int mode, int aligned, int* out);
/* Host-only query: what the image pass `entry` (SGX_AUG_PLAN_DIFFAUG / _GATED / _BLIT / _GEOM / _COLOR for sgx_diffaug / sgx_diffaug_gated /
 * sgx_diffaug_blit / sgx_ada_geom / sgx_ada_color) will launch for B images of H x W.  The entry points execute the same plan.  aligned:
 * both image bases are 16-byte aligned.  policy_bits is read for the first three entries only, with_bias for the colour pass only.
 * out[SGX_AUG_PLAN_INTS]: [0] the number of launches (1 or 2), then ten ints per launch, in launch order:
 *   +0  the kernel: 0 diffaug_sum_kernel<P, MODE, GATED>, 1 diffaug_apply_kernel<P, ADJ, GATED>, 2 diffaug_blit_sum_kernel<P, MODE>,
 *       3 diffaug_blit_row_kernel<P, ADJ>, 4 diffaug_blit_tile_kernel<ADJ>, 5 ada_geom_px_kernel<ADJ>, 6 ada_geom_tile_kernel<ADJ>,
 *       7 ada_color_px_kernel<ADJ, BIAS>, 8 ada_color_vec_kernel<ADJ, BIAS>
 *   +1  P, pixels per lane (1 or 4);  +2  MODE of the two sum kernels (0 the input itself, 2 the adjoint's gather), ADJ (0 / 1) of the
 *       others;  +3  GATED;  +4  BIAS -- each 0 for a kernel without that template argument
 *   +5  grid x, +6 grid y (= B); every block is 256 threads, no launch has dynamic LDS
 *   +7  nparts: partial sums per image (the workspace is 4 B nparts bytes: sgx_diffaug_ws_bytes);  +8  tiles of 32 x 32 pixels per row of
 *       tiles (the two tile kernels);  +9  H W (the colour kernels) -- the geometry arguments the kernel receives, 0 where it takes none
 * A policy with colour launches the sum pass, then the apply pass.  Returns 0, or what the entry itself returns for these arguments
 * (SGX_EINVAL: B outside 1..65535, H or W < 1, policy bits outside the entry's ops, rot90 with H != W, the colour adjoint with a bias;
 * SGX_EUNSUPPORTED: 3 H W >= 2^31), or SGX_EINVAL for an unknown entry or a NULL out.  out is zeroed on every error but the last. */
enum { SGX_AUG_PLAN_DIFFAUG = 0, SGX_AUG_PLAN_GATED = 1, SGX_AUG_PLAN_BLIT = 2, SGX_AUG_PLAN_GEOM = 3, SGX_AUG_PLAN_COLOR = 4 };
#define SGX_AUG_PLAN_INTS 21
int sgx_aug_plan(int entry, int B, int H, int W, int policy_bits, int adjoint, int with_bias, int aligned, int* out);
/* the generator's output in one pass: img = alpha * to_rgb(x) + beta * nearest_up2(low) (models/GAN.py:199-202 with the 1x1
 * convolution commuted in front of the upsample): low = [B][H/2][W/2][3] fp32.  ab_dev != NULL: alpha, beta = ab_dev[0], ab_dev[1]
 * read on the device (fade-in coefficient of a captured step graph). */
int sgx_rgb_out_fade(const void* x, const float* w, int sj, int sc, float wscale, const float* bias, const float* low, float alpha,
                     float beta, const float* ab_dev, float* img, int B, int H, int W, int C, int dtype, void* stream);
int sgx_rgb_wgrad(const float* img, const void* f, float* dw, int sj, int sc, float wscale, void* ws, size_t ws_bytes,
                  size_t npix, int C, int dtype, void* stream);

/* ---------------------------------------------------------------- generator layer epilogue
 * LayerEpilogue (models/CustomLayers.py:219-248) = NoiseLayer (:191-200) -> LeakyReLU -> nn.InstanceNorm2d (:233,
 * eps 1e-5, biased variance) -> StyleMod (:210-216), with the conv's post-blur bias (:178-179) folded in:
 *   p = x + bias[c] + nw[c]*noise[b,hw];  a = lrelu(p);  xh = (a - mean[b,c]) * rstd[b,c]
 *   y = xh * (style[b,c] + 1) + style[b,C+c]
 * bias may be NULL.  mean/rstd ([B][C] fp32) are outputs of fwd and inputs of bwd.
 * bwd returns dx, dstyle[B][2C], dnw[C], dbias[C] (dbias may be NULL).
 * flags select the stages the module was built with (LayerEpilogue's use_* arguments, :224-246): SGX_EPI_ACT = the
 * LeakyReLU, SGX_EPI_NORM = the instance norm (off: mean 0 / rstd 1 are written and the backward drops the statistics
 * terms).  use_noise=False is nw = 0, use_styles=False is style = 0 (both exact).  The default is ACT|NORM.           */
enum { SGX_EPI_ACT = 1, SGX_EPI_NORM = 2 };
size_t sgx_gepi_ws_bytes(int B, int HW, int C);
/* pre_part (may be NULL): the instance-norm statistics pass was already done by the kernel that PRODUCED x -- pre_npart
 * partial (sum a, sum a^2) pairs per (image, channel), double [B][pre_npart][C][2] (sgx_blur3x3_stats, sgx_conv3x3_stats):
 * the epilogue then reads the tensor once (apply pass) instead of twice. */
int sgx_gepi_fwd(const void* x, const float* bias, const float* noise, const float* nw, const float* style, void* y,
                 float* mean, float* rstd, void* ws, size_t ws_bytes, const double* pre_part, int pre_npart, int B, int HW,
                 int C, int flags, int dtype, void* stream);
/* Host-only query: what sgx_gepi_fwd / sgx_gepi_bwd / sgx_gepi_stats (entry SGX_GEPI_PLAN_FWD / _BWD / _STATS) will launch for this shape;
 * pre: producer partials given (pre_part != NULL) or not; the workspace is taken as sufficient.  The launchers execute the same plan.
 * out[SGX_GEPI_PLAN_INTS], the kernels in launch order being [0] alone, or [1], [3], [4], [12] and, in the backward, gepi_fin_bwd2:
 *   [0]  one launch for the whole direction: 0 no, 1 gepi_small_fwd / _bwd<T, 256, 2>, 2 <T, 512, 4> (the backward: + gepi_fin_bwd2)
 *   [1]  the reduction pass runs: gepi_pass<T, 0> (forward, statistics) / gepi_pass<T, 1> (backward)
 *   [2]  the finalize reads the producer's partials instead of that pass's
 *   [3]  gepi_fin_stats (forward, statistics) / gepi_fin_bwd1 (backward): 0 none, 1 a launch of its own, 2 the same, also writing the
 *        coefficient table of the short-lived apply kernel, 3 folded into the apply kernel
 *   [4]  the apply kernel: 0 none (statistics), 1 gepi_apply<T> / gepi_pass<T, 2, [5]>, 2 the short-lived blocks gepi_apply1<T> / gepi_bwd2s<T>
 *   [5]  its accesses carry the nontemporal hint
 *   [6..10]  the geometry of gepi_pass / gepi_apply: channel vectors and pixel rows per block, rows per thread, pixels per chunk, chunks per image
 *   [11] gepi_bwd2s: blocks per image;  [12] rows gepi_rows_prereduce leaves of their partials (0: it does not run)
 *   [13], [14]  gepi_fin_bwd2 sums [13] x [14] partial rows per channel
 * Returns the entry point's error code for the shape: 0, SGX_EINVAL, SGX_EUNSUPPORTED. */
enum { SGX_GEPI_PLAN_FWD = 0, SGX_GEPI_PLAN_BWD = 1, SGX_GEPI_PLAN_STATS = 2 };
#define SGX_GEPI_PLAN_INTS 15
int sgx_gepi_plan(int entry, int B, int HW, int C, int flags, int pre, int dtype, int* out);
/* y = blur3x3(x) (the generator's upscale-conv -> blur, models/CustomLayers.py:176-177, Blocks.py:63-65) with the statistics
 * pass of the LayerEpilogue that follows (:232-233 after :224-229) folded into the store: part receives the per-block partial
 * sums of a = act(y + bias[c] + nw[c]*noise[b,p]) and a^2 (y as stored), sgx_blur3x3_stats_nparts(...) blocks per image.
 * bias may be NULL; act: SGX_ACT_NONE | SGX_ACT_LRELU. */
int sgx_blur3x3_stats_nparts(int B, int H, int W, int C, int dtype);
/* y = conv3x3(x, pack) (no bias, no activation: the generator's conv1, models/Blocks.py:86, whose bias the epilogue adds) with
 * the same statistics out of the convolution's store epilogue: one partial per (image, pixel tile).  sgx_conv3x3_stats_nparts:
 * tiles per image, or 0 when the shape has no fused variant (then: sgx_conv3x3 + the plain sgx_gepi_fwd).  bf16 only. */
int sgx_conv3x3_stats_nparts(int B, int H, int W, int Cin, int Cout, int dtype);
/* sgx_conv3x3 that also writes the sign bits of its output (the discriminator block's conv0, models/Blocks.py:139-140, whose
 * pre-activation is the LeakyReLU-backward mask): bits = [B][H][W][Cout/8] bytes.  _ok: 1 if the shape has the variant (bf16). */
int sgx_conv3x3_signbits_ok(int B, int H, int W, int Cin, int Cout, int dtype);
int sgx_conv3x3_signbits(const void* x, const void* w, const float* bias, void* y, void* bits, int B, int H, int W, int Cin, int Cout,
                         int act, const void* mask, int dtype, void* stream);
/* y = blur3x3(conv_transpose4x4s2(x, pack)) [* slope(mask)] in one kernel: the transposed convolution and the BlurLayer that
 * follows it -- generator conv0_up -> blur (models/CustomLayers.py:143-152,176-177) and, with mask = the pre-activation z, the
 * discriminator's backward through "LeakyReLU -> blur -> conv1_down" (models/Blocks.py:140-145: the adjoint of the stride-2
 * convolution is this transposed one, the blur is self-adjoint, slope(z) = z > 0 ? 1 : 0.2).  mask: [B][2H][2W][Cout] or NULL.
 * The kernel applies the UNNORMALISED [1,2,1]x[1,2,1] filter: the caller packs the weights with scale / 16.
 * sgx_conv4x4s2_up_blur_ok: 1 if the shape has the fused kernel (bf16), else run sgx_conv4x4s2_up + sgx_blur3x3(_act). */
int sgx_conv4x4s2_up_blur_ok(int B, int H, int W, int Cin, int Cout, int dtype);
int sgx_conv4x4s2_up_blur(const void* x, const void* w, void* y, const void* mask, int B, int H, int W, int Cin, int Cout,
                          int dtype, void* stream);
/* Round 5: the same operation as ONE 3x3 stride-1 convolution over the coarse grid to the four output parity classes, stored depth-to-space
 * (blur o transposed-convolution is a 6x6 stride-2 transposed kernel = 3x3 taps per class; the blur's zero padding of the FINE grid is
 * restored at the image border by correction taps).  Replaces conv_transpose2d + BlurLayer (models/CustomLayers.py:143-152,175-177) and, in
 * the discriminator's backward, the adjoint of LeakyReLU -> blur -> conv1_down (models/Blocks.py:140-146) with the mask as sign bits.
 *   sgx_pack_upblur : the layer's parameter w [O][I][3][3] (mode SGX_PACK_U / _UF: an up layer's own convolution, adjoint = 0; SGX_PACK_D:
 *                     the data gradient of a down layer, adjoint = 1; scale = w_mul / 16, the blur's normalisation) -> wc bf16 [9][4N][K] + [22][2N][K],
 *                     (N, K) = (O, I) resp. (I, O): 9 composite taps + 22 border-correction tiles, composed in fp32 and rounded once.
 *   sgx_conv_upblur : y[B][2H][2W][Cout] = blur3x3(conv_transpose(x)) [* slope(bits)], bits [B][2H][2W][Cout/8] or NULL.  bf16, Cin = 32,
 *                     Cout = 16, W % 32 == 0 (sgx_conv_upblur_ok); other shapes: sgx_conv4x4s2_up_blur or the separate passes. */
int sgx_pack_upblur(const float* w, void* wc, int O, int I, int mode, int adjoint, float scale, void* stream);
int sgx_conv_upblur_ok(int B, int H, int W, int Cin, int Cout, int dtype);
int sgx_conv_upblur(const void* x, const void* wc, void* y, const void* maskbits, int B, int H, int W, int Cin, int Cout, int dtype, void* stream);
/* the same with the mask given as SIGN BITS of z, bits[B][2H][2W][Cout/8] as sgx_conv3x3_signbits / sgx_rgbconv_fwd write them */
int sgx_conv4x4s2_up_blur_bits(const void* x, const void* w, void* y, const void* bits, int B, int H, int W, int Cin, int Cout,
                               int dtype, void* stream);
int sgx_conv3x3_stats(const void* x, const void* w, void* y, const float* ebias, const float* noise, const float* nw, double* part,
                      size_t part_bytes, int B, int H, int W, int Cin, int Cout, int dtype, void* stream);

/* ---- the discriminator's first layer pair at the current resolution as ONE 3-channel convolution (round 4).
 * Discriminator.forward applies from_rgb -- a 1x1 EqualizedConv2d with NO activation (models/GAN.py:353,413-427) -- and then the
 * block's conv0 (3x3), LeakyReLU and blur (models/Blocks.py:137-142).  The two linear maps compose into a 3x3 convolution of the
 * RGB image:  W'[o][j][tap] = s0 sr sum_i W0[o][i][tap] Wr[i][j];  from_rgb's bias br reaches conv0 only through taps that fall
 * inside the image (conv0 zero-pads from_rgb's OUTPUT), T[o][tap] = s0 bscale sum_i W0[o][i][tap] br[i], carried by a 4th input
 * channel that is 1 inside the image.  img, gi: fp32 [B][H][W][3];  w0: conv0.weight [C][C][3][3], s0 = its w_mul;  wr:
 * from_rgb.weight [C][3][1][1], sr = its w_mul;  br: from_rgb.bias (bscale = its b_mul) or NULL;  b0: conv0.bias * b_mul or NULL.
 * bf16 activations, C in {16, 32}, H % 16 == 0, W % 64 == 0 (sgx_rgbconv_ok); other shapes: sgx_rgb_in + sgx_conv3x3 + sgx_blur3x3_act.
 *   sgx_rgbconv_pack : wf [3][C][16] (fp16 values in 2-byte elements: the forward kernels take fp16 operands) and wd [3][16][C] (bf16):
 *                      the operand packs of the forward / image-gradient kernels.
 *   sgx_rgbconv_fwd  : epi 1: y = blur3x3(lrelu(conv(img) + b0)) and bits[pixel][C/8] = sign bits of the pre-activation (the
 *                      LeakyReLU-backward mask, as sgx_conv3x3_signbits writes them; may be NULL);  epi 0: y = conv(img) (no b0).
 *                      ones: 1 = with from_rgb's bias channel, 0 = without (the adjoint's own backward under R1's double backward).
 *                      epi 0 (ones must be 0) scales every 16x64 tile by a power of two taken from the largest magnitude of the tile and
 *                      its halo, so its accuracy is relative to that maximum at any magnitude from 2^-126 up; fp32-denormal inputs are
 *                      outside the contract (a tile that holds nothing else is convolved unscaled and may come out as zeros).
 *   sgx_rgbconv_dgrad: gi = the gradient w.r.t. img given gz = the gradient w.r.t. the pre-activation (R1, models/Losses.py:197-211;
 *                      the generator step, models/GAN.py:640-655).
 *   sgx_rgbconv_wgrad: gradients of all four parameters from (img, gz) by the chain rule through the composition, written -- or, per
 *                      bit of `acc` (1: dw0, 2: db0, 4: dwr, 8: dbr), accumulated -- in the parameters' own layouts; NULL outputs
 *                      are skipped; ones = 0: no bias terms (db0 and dbr must be NULL).  ws: sgx_rgbconv_wgrad_ws_bytes. */
int sgx_rgbconv_ok(int B, int H, int W, int C, int dtype);
int sgx_rgbconv_pack(const float* w0, float s0, const float* wr, float sr, const float* br, float bscale, void* wf, void* wd, int C,
                     void* stream);
int sgx_rgbconv_fwd(const float* img, const void* wf, const float* b0, void* y, void* bits, int B, int H, int W, int C, int epi, int ones,
                    int dtype, void* stream);
/* process-wide A/B and probe state of sgx_rgbconv_fwd's epi 1 kernel (tests, tools/rgbconv_probe.py; initial values from
 * SGX_RGBCONV_FWD / SGX_RGBCONV_NIT, read once): fwd_variant 0 row-streaming (default), 1 / 2 the LDS-tile kernel with persistent
 * blocks / one tile per block, -1 = the default;  nit 1..8 = six-row steps per row block, 0 = chosen by launch size;  dbg: profiling
 * ablations of the row-streaming kernel (4 no output stores, 8 no sign bits -- wrong results by design), 0 = none. */
int sgx_rgbconv_tune(int fwd_variant, int nit, int dbg);
int sgx_rgbconv_dgrad(const void* gz, const void* wd, float* gi, int B, int H, int W, int C, int dtype, void* stream);
/* Host-only query: what sgx_rgbconv_pack / _fwd / _dgrad / _wgrad (entry SGX_RGBCONV_PLAN_PACK / _FWD / _DGRAD / _WGRAD) will launch for
 * this shape of bf16 activations under the current sgx_rgbconv_tune state.  The entry points execute the same plan.  B, H, W are not
 * read for the pack, epi only for the forward.  out[SGX_RGBCONV_PLAN_INTS]:
 *   [0]  the kernel: 0 rgbconv_pack_kernel, 1 rgbconv_fwd_kernel<[1], [2]> (the LDS-tile forward: epi 0, or variant 1 / 2),
 *        2 rgbconv_fwdblur_kernel<[1]> (epi 1, variant 0), 3 rgbconv_dgrad_kernel<[1]>,
 *        4 rgbconv_wgrad_kernel<[1]>, followed by rgbconv_wfinish_kernel and rgbconv_chain_kernel
 *   [1]  CB = C / 16;  [2] EPI: the forward's epi, 0 for the other entries
 *   [3]  that kernel's grid (256-thread blocks; wgrad: the number of block partials in the workspace);  [4] its dynamic LDS in bytes
 *   [5..7]  its geometry arguments: strips of 14 columns per row, row blocks per image, six-row steps per row block (fwdblur);  strips,
 *        row blocks of 32 rows, 0 (dgrad);  tiles per row, tile rows per image, tiles in all (the LDS-tile forward, wgrad);  0 (pack)
 *   [8]  the grid of rgbconv_wfinish_kernel, [9] of rgbconv_chain_kernel (wgrad; else 0)
 *   [10] the resident blocks per CU a persistent grid was sized with, [3] = ceil8(min([7], [10] * compute units)): the occupancy
 *        the runtime reports for rgbconv_fwd_kernel (1..4; 1 where there is no device), 3 for wgrad; 0 for a grid that is not persistent
 * Returns 0; SGX_EUNSUPPORTED for a shape sgx_rgbconv_ok refuses (the pack: C other than 16 or 32); SGX_EINVAL for an unknown entry,
 * an epi other than 0 or 1, or a NULL out.  out is zeroed on every error but the last. */
enum { SGX_RGBCONV_PLAN_PACK = 0, SGX_RGBCONV_PLAN_FWD = 1, SGX_RGBCONV_PLAN_DGRAD = 2, SGX_RGBCONV_PLAN_WGRAD = 3 };
#define SGX_RGBCONV_PLAN_INTS 11
int sgx_rgbconv_plan(int entry, int B, int H, int W, int C, int epi, int* out);
size_t sgx_rgbconv_wgrad_ws_bytes(int B, int H, int W, int C);
int sgx_rgbconv_wgrad(const float* img, const void* gz, int ones, const float* w0, float s0, const float* wr, float sr, const float* br,
                      float bscale, float* dw0, float* db0, float* dwr, float* dbr, int acc, void* ws, size_t ws_bytes, int B, int H, int W,
                      int C, int dtype, void* stream);
int sgx_blur3x3_stats(const void* x, void* y, const float* bias, const float* noise, const float* nw, double* part,
                      size_t part_bytes, int B, int H, int W, int C, int act, int dtype, void* stream);
int sgx_gepi_bwd(const void* dy, const void* x, const float* bias, const float* noise, const float* nw,
                 const float* style, const float* mean, const float* rstd, void* dx, float* dstyle, float* dnw,
                 float* dbias, void* ws, size_t ws_bytes, int B, int HW, int C, int flags, int dtype, void* stream);

/* ---------------------------------------------------------------- small fp32 pieces
 * PixelNormLayer on [B][C] rows: y = x * rsqrt(mean_c(x^2) + 1e-8)      models/CustomLayers.py:22-23                 */
int sgx_pixelnorm_fwd(const float* x, float* y, int B, int C, void* stream);
int sgx_pixelnorm_bwd(const float* dy, const float* x, float* dx, int B, int C, void* stream);
/* StddevLayer (models/CustomLayers.py:294-305), group = min(4,B), strided groups (sample i with i+M, i+2M, i+3M).
 *   fwd: y[b][hw][0..C) = x, y[b][hw][C] = stat[b % M], y[..][C+1..Cpad) = 0;   stat[m] = mean_{c,hw} sqrt(var_g + 1e-8)
 *   bwd: dx = dy[..][0..C) + (sum_{g,hw} dy[g*M+m][hw][C]) / (C*HW) * d / (G * s)
 *   bwd2 (second order, for R1): given ggx = cotangent of dx, returns its contribution to grad wrt dy (ddy) and x (gx) */
int sgx_mbstd_fwd(const void* x, void* y, int B, int HW, int C, int Cpad, int dtype, void* stream);
int sgx_mbstd_bwd(const void* dy, const void* x, void* dx, int B, int HW, int C, int Cpad, int dtype, void* stream);
int sgx_mbstd_bwd2(const void* ggx, const void* dy, const void* x, void* ddy, void* gx, int B, int HW, int C, int Cpad,
                   int dtype, void* stream);
/* R1 penalty head (models/Losses.py:210): out[0] = sum(x^2) over n fp32 values (deterministic two-stage reduce), and
 * its backward out = alpha * s[0] * x with the upstream scalar s on the device.                                      */
size_t sgx_sumsq_ws_bytes(void);
int sgx_sumsq_f32(const float* x, size_t n, void* ws, size_t ws_bytes, float* out, void* stream);
int sgx_scale_dev_f32(const float* x, const float* s, float alpha, float* out, size_t n, void* stream);
/* Logistic loss heads (models/Losses.py:213-229: mean softplus(fake) + mean softplus(-real); generator :227-229: mean softplus(-fake)),
 * times `scale` (1 / world size under data parallelism): loss[0] and the derivative w.r.t. every logit (g_fake [n_fake], g_real
 * [n_real]) from ONE launch instead of ~9 elementwise / reduction launches forward and as many backward.  generator != 0: real /
 * g_real are ignored (n_real must be 0).  fp32 logits.                                                                           */
int sgx_logistic_loss(const float* fake, int n_fake, const float* real, int n_real, float scale, int generator, float* loss,
                      float* g_fake, float* g_real, void* stream);
/* C[M][N] = alpha * op(A) * op(B) (+ beta*C), row-major fp32, MFMA f32 16x16x4.  EqualizedLinear
 * (models/CustomLayers.py:99-103: F.linear(x, W*w_mul)) and its gradients.  ta/tb: 0 = as stored, 1 = transposed:
 *   ta=0: A is [M][K], ta=1: A is [K][M];  tb=0: B is [K][N], tb=1: B is [N][K].
 * Alignment: 4 bytes is enough for every pointer of the GEMM and the three sgx_linear_* calls.  The 16-byte operand loads (and the
 * outer-product kernel for K <= 4) are taken only where the operand they read is 16-byte aligned; a pointer 4 bytes off gets the
 * scalar loads of the same k, and the same bits.                                                                      */
size_t sgx_gemm_ws_bytes(int M, int N, int K);
/* Host-only query: what sgx_gemm_f32 (fuse 0) or one of the three sgx_linear_* calls will launch for this shape.  The launcher executes
 * the same plan.  fuse: bit 0 = an activation mask on A (sgx_linear_bwd_data / _param with y_act), bit 1 = bias, activation or db fused
 * into the launch;  ws_bytes: the workspace held, 0 for NULL (the sgx_linear_* calls have none);  align: bit 0 = A and the mask are
 * 16-byte aligned, bit 1 = B is, bit 2 = C is.  out[SGX_GEMM_PLAN_INTS]:
 *   [0]  the kernel: 0 gemm_outer_kernel (K <= 4, B as stored, N % 4 == 0, nothing fused, B and C aligned), 1 gemm_f32_kernel<1>,
 *        2 gemm_f32_kernel<8> (a split's K of 512 or more)
 *   [1]  K splits; above 1 the partials go to the workspace and gemm_splitk_reduce follows (never with bit 1 of fuse or a short workspace)
 *   [2..4]  that kernel's grid x, y, z;  [5] the grid of gemm_splitk_reduce, 0 when unsplit
 *   [6]  the 16-byte operand loads the tile kernel may take: bit 0 = of A (and the mask), bit 1 = of B (0 for the outer-product kernel)
 * Returns 0, or SGX_EINVAL for a shape that is not positive. */
#define SGX_GEMM_PLAN_INTS 7
int sgx_gemm_plan(int M, int N, int K, int ta, int tb, int fuse, size_t ws_bytes, int align, int* out);
int sgx_gemm_f32(const float* A, const float* Bm, float* C, int M, int N, int K, int ta, int tb, float alpha,
                 void* ws, size_t ws_bytes, void* stream);
/* EqualizedLinear (models/CustomLayers.py:64-103) of the mapping network and the style affines, three launches:
 *   sgx_linear_fwd      : y[B][N] = act(w_mul * x[B][K] W[N][K]^T + b_mul * bias)        (bias nullable)
 *   sgx_linear_bwd_data : gx[B][K] = w_mul * gz W,  gz = gy * slope(y_act) (y_act nullable: no activation)
 *   sgx_linear_bwd_param: dW[N][K] = w_mul * gz^T x,  db[N] = b_mul * sum_b gz            (db nullable)           */
int sgx_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int N, int K, float w_mul, float b_mul,
                   int act, void* stream);
int sgx_linear_bwd_data(const float* gy, const float* y_act, const float* w, float* gx, int B, int N, int K, float w_mul,
                        void* stream);
int sgx_linear_bwd_param(const float* gy, const float* y_act, const float* x, float* dw, float* db, int B, int N, int K, float w_mul,
                         float b_mul, void* stream);
/* All style affines (StyleMod.lin, models/CustomLayers.py:203-216) of one generator forward in one launch, two for the
 * backward.  lm: layer-major dlatents [L][B][D] fp32.  table: G rows of SGX_STYLE_ROW 64-bit words
 *   [W (fp32 [N][D]), bias (fp32 [N] or 0), N, y offset in elements (= B * sum of earlier N), first tile (16 outputs per
 *    tile), w_mul as fp32 bits, b_mul as fp32 bits, layer index into lm];  total_tiles = sum of ceil(N/16).
 * y / gy: flat, group g at its offset as [B][N_g].  glm: [L][B][D] (rows of layers without a group are not written).
 * dw: flat [sum N][D], db: flat [sum N] (nullable).  B <= 32, D % 64 == 0 (SGX_EUNSUPPORTED otherwise).
 * sgx_style_fwd reads lm and the weight rows with 16-byte loads: lm must be 16-byte aligned (SGX_EINVAL otherwise), and so must every W
 * in the table, which lives in device memory and is not checked.  The two backward calls need 4-byte alignment only. */
#define SGX_STYLE_ROW 8
int sgx_style_fwd(const float* lm, const void* table, float* y, int G, int B, int D, int total_tiles, void* stream);
int sgx_style_bwd_data(const float* gy, const void* table, float* glm, int G, int B, int D, int max_n, void* stream);
int sgx_style_bwd_param(const float* gy, const float* lm, const void* table, float* dw, float* db, int G, int B, int D,
                        int total_tiles, void* stream);

/* ---- the generator's LAST layer epilogue inside to_rgb (round 4).  The last LayerEpilogue of the synthesis network feeds only to_rgb
 * (models/GAN.py:199-202 after models/Blocks.py:87-88 / models/CustomLayers.py:219-248): instead of writing x2 = StyleMod(InstanceNorm(
 * lrelu(y + bias + nw noise))) and reading it back in the 1x1 convolution, to_rgb reads the convolution's output y and applies the
 * epilogue per element on the fly.  Default stack only (activation + instance norm + style; flags = SGX_EPI_ACT | SGX_EPI_NORM).
 *   sgx_gepi_stats    : mean / rstd [B][C] of the epilogue (the statistics half of sgx_gepi_fwd; pre_part as there).
 *   sgx_rgb_out_epi   : img = alpha * (wscale W x2 + rbias) + beta * nearest_up2(low)   (low may be NULL: then beta is ignored)
 *   sgx_rgb_wgrad_epi : dw = scale * sum_p g[p][j] x2[p][c] in the parameter's layout, db[j] = bscale * sum_p g[p][j] (db nullable);
 *                       g = the image gradient [B][HW][3] fp32.  ws: sgx_rgb_wgrad_epi_ws_bytes.
 * The data gradient is sgx_rgb_in (g -> d x2) followed by sgx_gepi_bwd on y, as for the separate ops. */
int sgx_gepi_stats(const void* x, const float* bias, const float* noise, const float* nw, float* mean, float* rstd, void* ws, size_t ws_bytes,
                   const double* pre_part, int pre_npart, int B, int HW, int C, int flags, int dtype, void* stream);
int sgx_rgb_out_epi(const void* y, const float* ebias, const float* noise, const float* nw, const float* style, const float* mean,
                    const float* rstd, const float* w, int sj, int sc, float wscale, const float* rbias, const float* low, float alpha, float beta,
                    const float* ab_dev, float* img, int B, int H, int W, int C, int dtype, void* stream);    /* ab_dev as above */
size_t sgx_rgb_wgrad_epi_ws_bytes(int B, int HW, int C);
int sgx_rgb_wgrad_epi(const void* y, const float* g, const float* ebias, const float* noise, const float* nw, const float* style, const float* mean,
                      const float* rstd, float* dw, float* db, int sj, int sc, float scale, float bscale, void* ws, size_t ws_bytes, int B, int HW,
                      int C, int dtype, void* stream);

/* ---------------------------------------------------------------- optimizer step (multi-tensor, fp32)
 * torch.optim.Adam step (models/GAN.py:529-533, 616-618, 652) over n tensors described by DEVICE arrays of
 * pointers/sizes.  Per tensor t (torch keeps a step count per parameter; parameters of inactive resolutions have
 * no gradient and are not listed): step_sizes[t] = lr / (1 - beta1^step_t), bc2_sqrts[t] = sqrt(1 - beta2^step_t).
 *   g = grad*grad_scale[0];  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= step_size * m / (sqrt(v)/bc2_sqrt + eps)
 * grad_scale (device scalar, may be NULL) is the global-norm clip coefficient (models/GAN.py:651).
 * update_average EMA (models/__init__.py:31-36): tgt = beta*tgt + (1-beta)*src.                                      */
int sgx_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                   const int64_t* sizes, int n, float beta1, float beta2, float eps, const float* step_sizes,
                   const float* bc2_sqrts, const float* grad_scale, void* stream);
int sgx_ema_multi(float* const* tgt, const float* const* src, const int64_t* sizes, int n, float beta, void* stream);
/* nn.utils.clip_grad_norm_ (models/GAN.py:651) without a host sync: out[0] = sum over all tensors of sum(g^2),
 * out[1] = min(1, max_norm / (sqrt(out[0]) + 1e-6)); pass out+1 as grad_scale of sgx_adam_multi.
 * partial: caller scratch of n*32 doubles.                                                                            */
int sgx_gradnorm_clip_coef(const float* const* grads, const int64_t* sizes, int n, float max_norm, double* partial,
                           float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGX_H */
