/*
 * smpq.h — C-ABI of libsmpq.so, the MI355X-native (gfx950) semilayer mixed-precision
 * quantized convolution library.
 *
 * Plain pointers and sizes only (no torch types). Every device pointer is owned by the
 * caller (PyTorch's caching allocator on the Python side); the library never allocates
 * device memory and keeps no pointer past a call. Every kernel is enqueued on the HIP
 * stream passed in (Python passes torch.cuda.current_stream().cuda_stream), nothing blocks
 * the host except the *_host entry points. Return value: 0 on success, a negative SMPQ_E_*
 * code otherwise; smpq_last_error() holds a thread-local message.
 *
 * Reference interfaces replaced (kenm-28/Semilayer-Wise-Mixed-Precision-Quantization):
 *   smpq_quantize_channels[_host]  functions.py:25-43 quantize_wgt, applied per output channel
 *                                  as functions.py:9-23 channel_wise_quantizationperchan does
 *                                  (called from resnet50_main.py:189-197, functions.py:504-512)
 *   smpq_pack_weights              (new) fake-quantized fp32 weight -> int8 codes + per-channel
 *                                  step/offset; feeds the conv below (the reference keeps the
 *                                  fake-quantized fp32 weight in nn.Conv2d, resnet.py:22-30)
 *   smpq_conv2d_fwd                nn.Conv2d forward on the fake-quantized weight
 *                                  (resnet.py:22-30 via resnet.py:57,60,99,103,107) fused with
 *                                  the eval BatchNorm / ReLU / residual add that follow it in
 *                                  BasicBlock.forward (resnet.py:55-68) / Bottleneck.forward
 *                                  (resnet.py:97-116)
 *   smpq_act_absmax                (new) per-image activation range for the activation quantizer
 *   smpq_act_quantize              (new) activation quantizer (the reference keeps fp32 activations;
 *                                  int16/int24 codes reproduce them within the stated tolerance)
 *   smpq_softmax_xent              per-batch body of functions.py:84-129 evaluate_acc_loss_softmax
 *                                  (output.max(1), CrossEntropyLoss, Softmax(dim=1), :113-121)
 *   smpq_kl_rows                   functions.py:131-149 KLdiv (per-image sum_c n*log(n/o), :140-146)
 *   smpq_avgpool_fc                avgpool + flatten + fc of ResNet._forward_impl (resnet.py:216-218),
 *                                  batch-invariant (sharded logits == single-GPU logits, bitwise)
 */
#ifndef SMPQ_H_
#define SMPQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMPQ_ABI_VERSION 7

/* status codes */
#define SMPQ_OK 0
#define SMPQ_E_INVALID (-1)  /* bad argument / unsupported configuration */
#define SMPQ_E_SHAPE (-2)    /* shape the kernels do not support */
#define SMPQ_E_BITS (-3)     /* bit-width outside {1..8} */
#define SMPQ_E_RANGE (-4)    /* a channel's codes span more than 256 levels */
#define SMPQ_E_CONSTANT (-5) /* constant channel: the reference raises ZeroDivisionError */
#define SMPQ_E_HIP (-6)      /* a HIP runtime call failed */
#define SMPQ_E_INEXACT (-7)  /* weights are not on the recorded quantization grid */

typedef void* smpq_stream_t; /* hipStream_t */

int smpq_abi_version(void);
const char* smpq_last_error(void);
/* SHA-256 (hex) of the sources, headers and compiler flags this library was built from;
 * __graft_entry__.build() rebuilds whenever the tree's hash differs from it. */
const char* smpq_build_stamp(void);

/* Rounding semantics of functions.py:41 `t / scale` (scale a Python float), which depend on
 * where the reference's tensor lives:
 *   SMPQ_QSEM_CPU     torch on the CPU: IEEE fp32 division t / fp32(scale)
 *   SMPQ_QSEM_DEVICE  torch on the GPU: t * fp32(1.0 / scale) (reciprocal of the double scale,
 *                     rounded once; tests/golden/quant_kat_device.npz, produced by torch on an
 *                     MI355X, pins it) */
#define SMPQ_QSEM_CPU 0
#define SMPQ_QSEM_DEVICE 1

/* Fake-quantize channels of w in place, bit-exactly as functions.py:25-43 executes under
 * `semantics` (SMPQ_QSEM_*).
 *   w          device fp32 [cout][k_elems] (one output channel per row)
 *   bits       device int8 [cout]; 0 leaves the channel untouched
 *   scale_out  device fp32 [cout]; receives fp32(scale) of the quantization applied
 *   status     device int32 [1], caller-zeroed; set to (lowest constant channel)+1, whatever order
 *              the channels' workgroups run in (an atomic minimum over the non-zero reports)
 * On that error every non-constant channel of the call is quantized all the same (its scale_out
 * written) and the constant channels are left untouched with their scale_out unwritten: the channels
 * run in parallel and none waits for another. (The host twin below stops at the first constant
 * channel instead, as the reference's loop does.) */
int smpq_quantize_channels_ex(float* w, int cout, int k_elems, const int8_t* bits,
                              float* scale_out, int32_t* status, int semantics, smpq_stream_t stream);

/* smpq_quantize_channels_ex with SMPQ_QSEM_CPU (ABI v1 entry point, kept). */
int smpq_quantize_channels(float* w, int cout, int k_elems, const int8_t* bits,
                           float* scale_out, int32_t* status, smpq_stream_t stream);

/* Host-memory twin of smpq_quantize_channels (same arithmetic, native C++), used when the
 * weight lives in host memory (the reference quantizes CPU tensors of fresh models, e.g.
 * functions.py:504-512 right after resnet.resnet50(...) at :528). Returns SMPQ_E_CONSTANT on
 * the lowest constant channel, which the error message names (channels before it are already
 * quantized, that channel and every later one untouched, as in the reference loop). */
int smpq_quantize_channels_host_ex(float* w, int cout, int k_elems, const int8_t* bits,
                                   float* scale_out, int semantics);

/* smpq_quantize_channels_host_ex with SMPQ_QSEM_CPU (ABI v1 entry point, kept). */
int smpq_quantize_channels_host(float* w, int cout, int k_elems, const int8_t* bits,
                                float* scale_out);

/* Pack fake-quantized weights into the conv kernel's layout.
 *   w       device fp32 [cout][cin][kh][kw] (fake-quantized, values fl32(m * step))
 *   step    device fp32 [cout] quantization step (scale_out of the quantizer)
 *   codes   device int8 [cout][kh][kw][cin]   m - offset, in [-128, 127]
 *   offset  device int32 [cout]
 *   status  device int32 [2], caller-zeroed: [0] += channels not on the grid,
 *           [1] += channels whose codes span > 256 levels */
int smpq_pack_weights(const float* w, int cout, int cin, int kh, int kw, const float* step,
                      int8_t* codes, int32_t* offset, int32_t* status, smpq_stream_t stream);

/* General weight packer for smpq_conv2d_fwd_ex: `wlimbs` int8 planes codes[wlimbs][cout][K].
 *   step     device fp32 [cout] recorded quantization step, 0 = never quantized (may be NULL
 *            when wlimbs == 2: every channel then uses 16-bit fixed point)
 *   wlimbs   1: exact int8 codes (m - offset) of quantized channels (status[0]/[1] report
 *            channels that cannot be coded); 2 / 3: exact codes of quantized channels that fit
 *            16 / 24 bits, per-channel fixed point (max|w| / 32512 or / 8323072) for the others
 *            (status[2] counts them)
 *   cin      a multiple of 64 (K = kh*kw*cin, ordered [kh][kw][cin]); the <= 4-channel stem is
 *            packed by smpq_pack_weights_s2d_ex
 *   offset   device int32 [cout] (wlimbs == 1), wscale device fp32 [cout]: the per-channel weight
 *            step the codes are in (= step for exact channels)
 *   status   device int32 [3], caller-zeroed */
int smpq_pack_weights_ex(const float* w, int cout, int cin, int kh, int kw, const float* step,
                         int wlimbs, int8_t* codes, int32_t* offset, float* wscale, int32_t* status,
                         smpq_stream_t stream);

/* Per-image absolute maximum, accumulated with atomicMax into absmax[n] (caller zeroes). */
int smpq_act_absmax(const float* x, int n, int64_t per_image, float* absmax,
                    smpq_stream_t stream);

/* Activation quantizer: q = clamp(rne(x * QMAX_L / absmax[img]), +-QMAX_L) with
 * QMAX_1 = 127, QMAX_2 = 32512, QMAX_3 = 8323072, written as `limbs` balanced base-256 int8
 * digit planes (q = sum_l 256^l * plane_l), each plane laid out like x.
 *   x        device fp32, n images of per_image elements (per_image % 8 == 0)
 *   absmax   device fp32 [n] (from smpq_act_absmax or a conv's y_absmax)
 *   out      device int8 [limbs][n * per_image] */
int smpq_act_quantize(const float* x, int n, int64_t per_image, const float* absmax, int limbs,
                      int8_t* out, smpq_stream_t stream);

/* MaxPool2d(3, stride 2, pad 1) (resnet.py:147) on NHWC fp32 [n][h][w][c] (c % 4 == 0), fused
 * with the activation quantizer of its output: `limbs` int8 planes [n][ho][wo][c] with the
 * per-image range absmax (the pool input's max; equal to the output's for ReLU outputs).
 * out_f32: optional fp32 NHWC pooled output (NULL to skip). */
int smpq_maxpool_quantize(const float* x, int n, int h, int w, int c, const float* absmax, int limbs,
                          int8_t* out, float* out_f32, smpq_stream_t stream);

/* Quantized conv forward (implicit GEMM on int8 MFMA), NHWC.
 *   xq         device int8 [limbs][n][h][w][cin] digit planes from smpq_act_quantize; cin % 64 == 0
 *   x_absmax   device fp32 [n]: the per-image range xq was quantized with
 *   codes/offset/cout/kh/kw: from smpq_pack_weights (offset may be NULL when all zero)
 *   col_scale  device fp32 [cout]: y = conv_real * col_scale[c] + col_shift[c]
 *              (col_scale = step * bn_gamma / sqrt(var+eps), col_shift = bn_beta - mean * ...)
 *   residual   device fp32 NHWC [n][ho][wo][cout] added after the affine, or NULL
 *   relu       0/1, applied last
 *   limbs      activation code width in int8 limbs: 1 (int8), 2 (int16), 3 (int24)
 *   y          device fp32 NHWC [n][ho][wo][cout]
 *   y_absmax   device fp32 [n] (caller-zeroed), receives max|y| per image, or NULL
 *   tile_cfg   block tile configuration (smpq_conv2d_tile_config), or -1 for the built-in choice
 *   cout % 16 == 0, and every activation / output plane below 2 GiB (32-bit buffer offsets:
 *   SMPQ_E_SHAPE otherwise; the Python layer splits such batches). ABI v4: the register-staged
 *   kernel family of v1-v3 (and with it cin == 4) is gone; tile configurations are numbered from 0
 *   in the LDS-DMA family. */
int smpq_conv2d_fwd(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                    const int8_t* codes, const int32_t* offset, int cout, int kh, int kw,
                    int stride, int pad, const float* col_scale, const float* col_shift,
                    const float* residual, int relu, int limbs, float* y, float* y_absmax,
                    int tile_cfg, smpq_stream_t stream);

/* smpq_conv2d_fwd with weight limbs (1, 2, or 3 with limbs == 3): codes [wlimbs][cout][K] from
 * smpq_pack_weights_ex. col_scale must include the per-channel weight step (wscale) of the
 * packer. */
int smpq_conv2d_fwd_ex(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                       const int8_t* codes, int wlimbs, const int32_t* offset, int cout, int kh,
                       int kw, int stride, int pad, const float* col_scale, const float* col_shift,
                       const float* residual, int relu, int limbs, float* y, float* y_absmax,
                       int tile_cfg, smpq_stream_t stream);

/* smpq_conv2d_fwd_ex that can also (or only) emit the NEXT conv's activation limb planes:
 *   y          fp32 NHWC output, or NULL when only yq is wanted
 *   yq         int8 [limbs][n*ho*wo][cout] planes of q = clamp(rne(y * QMAX / yq_range)), or NULL
 *   yq_range   static per-layer range (> 0) of the output quantizer (calibrated by the caller)
 *   overflow   device int32 [1]: set to 1 when some |y| > yq_range (values are then clamped; the
 *              caller re-runs with dynamic ranges)
 *   residual_q int8 [limbs][n*ho*wo][cout] limb planes of the residual (e.g. the block input as
 *              written by the previous conv's yq), dequantized as residual_range/QMAX * q; NULL
 *              when `residual` (fp32) or no residual is used */
int smpq_conv2d_fwd_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                      const int8_t* codes, int wlimbs, const int32_t* offset, int cout, int kh,
                      int kw, int stride, int pad, const float* col_scale, const float* col_shift,
                      const float* residual, int relu, int limbs, float* y, float* y_absmax,
                      int8_t* yq, float yq_range, int32_t* overflow, const int8_t* residual_q,
                      float residual_range, int tile_cfg, smpq_stream_t stream);

/* smpq_conv2d_fwd_q with a second copy of the same codes in the K-major layout
 * codes_kmajor [wlimbs][K/64][cout][64] (smpq_weights_kmajor; round 3): the LDS-DMA tile
 * configurations then stage every weight piece from whole cache lines (the 64-B K slices of 16
 * consecutive output channels are one contiguous KiB) instead of 16 half lines — 6-21 % faster
 * on the MFMA-heavy convs. Results are bitwise those of smpq_conv2d_fwd_q. codes (row-major) is
 * still required (the v3 signature is kept); codes_kmajor may be NULL. */
int smpq_conv2d_fwd_q_km(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                         const int8_t* codes, const int8_t* codes_kmajor, int wlimbs, const int32_t* offset,
                         int cout, int kh, int kw, int stride, int pad, const float* col_scale,
                         const float* col_shift, const float* residual, int relu, int limbs, float* y,
                         float* y_absmax, int8_t* yq, float yq_range, int32_t* overflow,
                         const int8_t* residual_q, float residual_range, int tile_cfg, smpq_stream_t stream);

/* ABI 7: a Bottleneck's conv3 (+ limb-plane identity, ReLU) chained with the NEXT block's conv1
 * (ReLU) in one launch (resnet.py:111-113, then :99-101 of the next block): the second conv reads
 * the first one's output tile from LDS instead of HBM. Both outputs and the overflow flag are
 * bitwise those of two smpq_conv2d_fwd_q calls. 3 activation limbs, exact weight codes (no offsets):
 *   xq, x_absmax, n, h, w, cin          conv3's input, as smpq_conv2d_fwd_q (1x1, stride 1, pad 0)
 *   codes1 [cout1][cin], col_scale1, col_shift1 [cout1]        conv3 (+ its folded BN)
 *   residual_q [3][n*h*w][cout1], residual_range               the identity's limb planes
 *   yq1 [3][n*h*w][cout1], yq1_range    conv3's output limb planes (the next block's identity)
 *   y1_absmax [n]                       per-image range conv1 reads them with (what a separate
 *                                       conv1 launch gets as x_absmax)
 *   codes2 [cout2][cout1], col_scale2, col_shift2 [cout2]      the next block's conv1
 *   yq2 [3][n*h*w][cout2], yq2_range    conv1's output limb planes
 *   overflow                            int32 [1]: set when either output exceeded its range
 * Built for (cin, cout1, cout2) = (64, 256, 64) and (64, 256, 128), the ResNet-50 layer1 blocks and
 * layer 1's last conv3 with layer 2's first conv1 (smpq_conv2d_pair_supported); other calls return
 * SMPQ_E_INVALID. */
int smpq_conv2d_pair_supported(int cin, int cout1, int cout2, int limbs);
int smpq_conv2d_pair_fwd(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                         const int8_t* codes1, int cout1, const float* col_scale1, const float* col_shift1,
                         const int8_t* residual_q, float residual_range, int8_t* yq1, float yq1_range,
                         const float* y1_absmax, const int8_t* codes2, int cout2, const float* col_scale2,
                         const float* col_shift2, int8_t* yq2, float yq2_range, int32_t* overflow,
                         smpq_stream_t stream);

/* ABI 7: the general form of the Bottleneck tail chain. conv3 (exact codes; offset1 = its weight
 * offsets or NULL) with its identity from ONE of
 *   residual_q / residual_range        the identity's limb planes, as smpq_conv2d_pair_fwd, or
 *   ds_xq [3][n*ds_h*ds_w][ds_cin], ds_x_absmax [n], ds_codes [3][cout1][ds_cin] (ds_wlimbs = 3:
 *   24-bit fixed point from smpq_pack_weights_ex), ds_col_scale / ds_col_shift [cout1], ds_range
 *                                      the block's 1x1 downsample (stride ds_stride) whose output
 *                                      pixels are conv3's, computed in the same tiles: its clamped
 *                                      output codes (what a
 *                                      smpq_conv2d_fwd_q launch with emit range ds_range writes) are
 *                                      conv3's residual and are never written; overflow covers them,
 * and optionally (codes2 != NULL) the next block's conv1 on conv3's output as smpq_conv2d_pair_fwd
 * (no offsets). Every output and the overflow flag are bitwise those of the separate launches.
 * Built: conv3 64 -> 256 with the next conv1 256 -> 64 or 256 -> 128 (smpq_conv2d_chain_supported), and conv3
 * with a fused downsample and no second conv for the first blocks of R50's layers 1-3 (64 -> 256 /
 * ds 64 / stride 1, 128 -> 512 / ds 256 / 2, 256 -> 1024 / ds 512 / 2: smpq_conv2d_chain_ds_supported);
 * other calls return SMPQ_E_INVALID. */
int smpq_conv2d_chain_supported(int cin, int cout1, int cout2, int limbs);
int smpq_conv2d_chain_ds_supported(int cin, int cout1, int ds_cin, int ds_stride, int limbs);
int smpq_conv2d_chain_fwd(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                          const int8_t* codes1, const int32_t* offset1, int cout1, const float* col_scale1,
                          const float* col_shift1, const int8_t* residual_q, float residual_range,
                          const int8_t* ds_xq, const float* ds_x_absmax, int ds_h, int ds_w, int ds_cin,
                          int ds_stride, const int8_t* ds_codes, int ds_wlimbs,
                          const float* ds_col_scale, const float* ds_col_shift, float ds_range, int8_t* yq1,
                          float yq1_range, const float* y1_absmax, const int8_t* codes2, int cout2,
                          const float* col_scale2, const float* col_shift2, int8_t* yq2, float yq2_range,
                          int32_t* overflow, smpq_stream_t stream);

/* codes [wlimbs][cout][K] (K % 64 == 0, 16-B aligned) -> out [wlimbs][K/64][cout][64], the K-major
 * copy smpq_conv2d_fwd_q_km reads. */
int smpq_weights_kmajor(const int8_t* codes, int wlimbs, int cout, int K, int8_t* out, smpq_stream_t stream);

/* 3x3 / stride 2 / pad 1 max pool (resnet.py:147) directly on int8 limb planes
 * x [limbs][n][h][w][c] -> out [limbs][n][ho][wo][c], c % 16 == 0 (static-range mode: the codes of
 * one activation share one step, so the max of the codes is the code of the max — exact). */
int smpq_maxpool_limbs(const int8_t* x, int n, int h, int w, int c, int limbs, int8_t* out, smpq_stream_t stream);

/* ---- space-to-depth stem (the 7x7 / stride 2 / pad 3 conv1 of resnet.py:143) -------------------
 * The stem runs as a 4x4 / stride 1 conv over 16-channel "space-to-depth" pixels (each a 2x2
 * block of the image with up to 4 channels), so every 64-byte K step of the int8 GEMM is one
 * tap row of whole 16-byte pixels (tests/test_gpu.py checks it against an exact emulation of the
 * 7x7/2/3 conv on the quantized image).
 *
 * smpq_image_quantize_s2d: x fp32 NCHW [n][c <= 4][h][w] (h, w >= 2) ->
 *   out int8 [limbs][n][ceil(h/2)][ceil(w/2)][16], channel (dy*2 + dx)*4 + ci = x[ci][2i + dy][2j + dx]
 *   quantized with the per-image absmax as smpq_act_quantize does (zero for ci >= c and past an
 *   odd h or w: the conv's own zero padding).
 * smpq_pack_weights_s2d_ex: w fp32 [cout][cin <= 4][7][7] -> codes int8 [wlimbs][cout][256] (K order
 *   [ty][tx][dy][dx][ci], original tap (2 ty + dy - 1, 2 tx + dx - 1), zero outside 7x7) with scale
 *   wscale [cout]: channels with a recorded quantization step (step[c] > 0; step may be NULL) as
 *   exact codes, the others in per-channel fixed point (wlimbs 2 / 3 = 16 / 24 bits) — the rules of
 *   smpq_pack_weights_ex; status[3] as there. smpq_pack_weights_s2d = the same with step NULL.
 * smpq_stem_conv_s2d_q: as smpq_conv2d_fwd_q with the stem geometry (h, w = the ORIGINAL image
 *   size; output [n][ceil(h/2)][ceil(w/2)][cout] NHWC), no residual; cout % 16 == 0; tile_cfg one
 *   of the tile configs with 64 output channels per block, or -1. */
int smpq_image_quantize_s2d(const float* x, int n, int c, int h, int w, const float* absmax, int limbs,
                            int8_t* out, smpq_stream_t stream);
int smpq_pack_weights_s2d_ex(const float* w, int cout, int cin, const float* step, int wlimbs, int8_t* codes,
                             float* wscale, int32_t* status, smpq_stream_t stream);
int smpq_pack_weights_s2d(const float* w, int cout, int cin, int wlimbs, int8_t* codes, float* wscale,
                          int32_t* status, smpq_stream_t stream);
int smpq_stem_conv_s2d_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, const int8_t* codes,
                         int wlimbs, int cout, const float* col_scale, const float* col_shift, int relu,
                         int limbs, float* y, float* y_absmax, int8_t* yq, float yq_range, int32_t* overflow,
                         int tile_cfg, smpq_stream_t stream);

/* Fused stem, static-range mode: conv1 7x7/2/3 + bn1 + ReLU + maxpool 3x3/2/1 (resnet.py:143-147,
 * ResNet.forward resnet.py:206-209) in one launch, on smpq_image_quantize_s2d planes and
 * smpq_pack_weights_s2d codes -> the POOLED output's limb planes yq [limbs][n][h/4][w/4][64]
 * (h, w = the original image size). Bitwise identical to smpq_stem_conv_s2d_q (relu = 1, yq with
 * the same range, y = NULL) followed by smpq_maxpool_limbs; *overflow is set to 1 when a conv
 * output exceeded the range (then clamped). smpq_stem_pool_supported returns 1 for the shapes it
 * handles: cout == 64, h and w multiples of 4, w <= 224, (limbs, wlimbs) in {(3,3), (2,2), (1,2)};
 * otherwise use the two-launch path. */
int smpq_stem_pool_supported(int n, int h, int w, int cout, int limbs, int wlimbs);
int smpq_stem_pool_s2d_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, const int8_t* codes,
                         int wlimbs, int cout, const float* col_scale, const float* col_shift, int limbs,
                         int8_t* yq, float yq_range, int32_t* overflow, smpq_stream_t stream);

/* AdaptiveAvgPool2d(1) + flatten + fc (ResNet._forward_impl resnet.py:216-218; modules built at
 * resnet.py:162-163) on the last block's NHWC fp32 output x [n][hw][c]: pooled[n][c] = (fp32 sum
 * over the hw pixels) / hw, the division by hw correctly rounded (not a multiply by 1 / hw);
 * logits[n][nout] = pooled . fc_w[nout][c] (+ fc_b[nout]) in fp32. Guaranteed: the order of every
 * sum is fixed by hw and c alone (today: the pixels in order; the dot product as four partial sums
 * over quarters of c, added in quarter order), never by n, nout or the other images, so an image's
 * logits are the same bits whatever batch or data-parallel shard it runs in; and the bias is added
 * last, in one rounded fp32 addition, so the logits with a bias are bitwise the logits without it
 * + fc_b. The order itself is not part of the contract: each pooled feature is within
 * (hw + 1) u (sum |x|) / hw and each logit within (hw + c + 2) u (sum_k P_k |w_k| + |b|) of the
 * exact value, u = 2^-24, P_k = (sum over pixels |x_k|) / hw (tests/tail_ref.py). pooled_ws: device
 * fp32 [n][c] (workspace, holds the pooled features afterwards); fc_b may be NULL; c % 4 == 0. */
int smpq_avgpool_fc(const float* x, int n, int hw, int c, const float* fc_w, const float* fc_b, int nout,
                    float* pooled_ws, float* logits, smpq_stream_t stream);

/* Tile configurations of smpq_conv2d_fwd (for autotuning): count, and BM (pixels) x BN (output
 * channels) / threads. Every configuration gives bitwise-identical results. */
int smpq_conv2d_num_tile_configs(void);
int smpq_conv2d_tile_config(int cfg, int* bm, int* bn, int* threads);

/* Kernel family of a tile configuration:
 *   SMPQ_TILE_LDS_DMA          LDS-DMA loader; cin % 64 == 0, cout % 16 == 0, every operand and
 *                              output plane < 2 GiB
 *   SMPQ_TILE_LDS_DMA_K128     as SMPQ_TILE_LDS_DMA with 128-wide K steps: also cin % 128 == 0
 *   SMPQ_TILE_HALO3X3          (ABI 5) halo-patch 3x3 kernel: 3x3 / stride 1 / pad 1 convs with
 *                              cin % 64 == 0, cout % 64 == 0, one weight limb, 2 or 3 activation
 *                              limbs, static-range limb-plane output with ReLU (yq set,
 *                              relu != 0; y, y_absmax, residual NULL), optionally with a
 *                              limb-plane residual_q (round 6) — other calls return
 *                              SMPQ_E_INVALID.
 *                              Its configurations follow the LDS-DMA ones; BM = the tile's pixels
 *                              (TH x TW of one image), BN = 64.
 *   SMPQ_TILE_RESIDENT1X1      (ABI 6) weight-stationary 1x1 tiles: 1x1 / pad 0 convs with cin
 *                              64 .. 1024 (per configuration: smpq_conv2d_tile_supported), cout a
 *                              multiple of the slab (BN = 64 / 128 / 256), 3 activation limbs,
 *                              static-range limb-plane output (yq set; y, y_absmax, residual NULL);
 *                              3 weight limbs without ReLU or residual_q (the downsamples), 1 weight
 *                              limb with ReLU and optionally residual_q (both with or without weight
 *                              offsets), or neither (no offsets) — other calls return
 *                              SMPQ_E_INVALID. A persistent workgroup keeps its slab's weight limbs
 *                              in registers and walks pixel tiles; BM = pixels per tile, BN = the
 *                              slab. Configurations follow the halo ones.
 *   SMPQ_TILE_RESIDENT1X1_W    (ABI 7, appended) the same four geometries for the 1x1 convs of a
 *                              model under search: 1x1 / stride 1 / pad 0 convs with 3 activation
 *                              limbs and 3 weight limbs (24-bit fixed point), cin 64 .. 512 (per
 *                              configuration: smpq_conv2d_tile_supported), cout a multiple of the
 *                              slab, no weight offsets, ReLU on, static-range limb-plane output
 *                              (yq set; y, y_absmax, residual NULL), with or without residual_q —
 *                              other calls return SMPQ_E_INVALID. Configurations follow the
 *                              SMPQ_TILE_RESIDENT1X1 ones; tile_cfg = -1 never picks one.
 * (negative: error code). Values 0 and 1 were the register-staged family (ABI <= 3, removed). */
#define SMPQ_TILE_LDS_DMA 2
#define SMPQ_TILE_LDS_DMA_K128 3
#define SMPQ_TILE_HALO3X3 4
#define SMPQ_TILE_RESIDENT1X1 5
#define SMPQ_TILE_RESIDENT1X1_W 6
int smpq_conv2d_tile_kind(int cfg);

/* 1 if tile configuration cfg can run a conv of this shape and these limb counts (the rules the
 * launch applies: loader family, K-step width, accumulator budget, LDS per CU), else 0. Every
 * supported configuration gives bitwise-identical results. */
int smpq_conv2d_tile_supported(int cfg, int cin, int cout, int kh, int kw, int limbs, int wlimbs);

/* Workspace the conv needs (none today; kept for ABI stability). */
size_t smpq_conv2d_workspace_bytes(int n, int h, int w, int cin, int cout, int kh, int kw,
                                   int stride, int pad, int limbs);

/* ---- evaluation reductions (functions.py:84-149) ---------------------------------------------
 * smpq_softmax_xent: one batch of logits [rows][cols] fp32 with int64 labels [rows]:
 *   probs  fp32 [rows][cols] softmax = exp(x - max) / sum (functions.py:117), or NULL
 *   stats  double [4], ACCUMULATED (+=): [0] batch-mean cross entropy (criterion(output, y),
 *          :116 — one term per call, as loss_sum += loss at :121), [1] rows whose first maximal
 *          class equals the label (output.max(1), :114), [2] rows, [3] batches (+1)
 *   row_ws fp32 workspace [2 * rows]; afterwards row_ws[row] is the row's loss
 *          log(sum) + max - x[label] (NaN for a label outside [0, cols)) and row_ws[rows + row] is
 *          1.0 when the row's first maximal class equals its label, else 0.0
 * smpq_kl_rows: stats double [2] += {sum over rows of sum_c p_ref * log(p_ref / p), rows}
 *   (functions.py:140-146; KLdiv = stats[0] / stats[1]); row_ws fp32 [rows], afterwards the rows'
 *   sums. The terms follow IEEE arithmetic as the reference's do: p = 0 where p_ref > 0 makes the
 *   row +inf, and p_ref = 0 makes it NaN (0 * log 0), whatever p is there.
 * Rows are reduced in a fixed order in double: results do not depend on launch timing. A label
 * outside [0, cols) makes that row's loss NaN (the reference raises), and with it stats[0]; the
 * other rows' row_ws entries and stats[1..3] are unaffected. */
int smpq_softmax_xent(const float* logits, const int64_t* labels, int rows, int cols, float* probs,
                      double* stats, float* row_ws, smpq_stream_t stream);
int smpq_kl_rows(const float* p_ref, const float* p, int rows, int cols, double* stats, float* row_ws,
                 smpq_stream_t stream);

/* ---- content fingerprints (cache validation; smpq/engine.py) ------------------------------------
 * smpq_fingerprint: out[t] = sum_i H(w_i, i) mod 2^64 over the ceil(nbytes[t] / 4) 32-bit words of
 *   tensor t (device pointers ptrs[t], 4-B aligned, a device array; a partial last word is
 *   zero-padded), for t < ntensors; the work is split into
 *   nchunks chunks of smpq_fingerprint_chunk_words() words: chunk c covers tensor chunk_tensor[c]
 *   from word chunk_word[c] (device arrays). out (device uint64 [ntensors]) is overwritten.
 *   H(w, i) = fmix32(w ^ i*0x9E3779B9) | fmix32(w ^ (i*0x85EBCA6B + 0xC2B2AE35)) << 32, fmix32 = the
 *   MurmurHash3 finalizer (all arithmetic mod 2^32): injective in w for each i, so any single-word
 *   change changes the fingerprint, and structured multi-word changes cancel with p ~ 2^-64.
 * smpq_fingerprint_compare: *flag |= 1 if a[i] != b[i] for some i < n (device arrays).
 * smpq_fingerprint_host: the same sum over nbytes bytes of host memory.
 * Used to detect in-place writes through `.data` (functions.py:22, resnet50_main.py:191) that
 * leave a Parameter's version counter unchanged. */
long long smpq_fingerprint_chunk_words(void);
int smpq_fingerprint(const void* const* ptrs, const int64_t* nbytes, int ntensors, const int32_t* chunk_tensor,
                     const int64_t* chunk_word, int nchunks, uint64_t* out, smpq_stream_t stream);
int smpq_fingerprint_compare(const uint64_t* a, const uint64_t* b, int n, int32_t* flag, smpq_stream_t stream);
uint64_t smpq_fingerprint_host(const void* p, int64_t nbytes);

/* ---- bit-packed weight store, format "smpq-packed/1" (normative) ---------------------------------
 * The fake-quantized fp32 weights the search produces (functions.py:9-43) are exact multiples of
 * their channel's step, so a b-bit channel needs b bits per weight, not 32: the in-memory snapshot
 * the search's save / rollback uses (resnet50_main.py:212, :233-234) and the on-disk export
 * (smpq/checkpoint.py snapshot / restore_ / save_packed / load_packed). Bit-exact both ways.
 *
 * One fp32 weight viewed as [cout][k], k = cin*kh*kw in the tensor's own [cin][kh][kw] order, is
 * stored as five per-channel arrays and a payload of 32-bit words:
 *   qbits    int8  [cout]    verbatim copy of the conv's metadata
 *   step     fp32  [cout]    verbatim copy of the conv's metadata
 *   mode     int8  [cout]    0 = raw; 1..8 = packed with that many bits per code
 *   base     int32 [cout]    smallest code m of the channel; 0 for raw channels
 *   word_off int64 [cout+1]  offsets into the payload in 32-bit words: the exclusive prefix sum of
 *                            the per-channel word counts (word_off[0] = 0, word_off[cout] = total)
 * Channel c is PACKED with b = qbits[c] when all of these hold, and RAW otherwise:
 *   1. 1 <= b <= 8;
 *   2. step[c] is finite and > 0;
 *   3. every value v of the channel is finite;
 *   4. m = rintf(v / step) (IEEE fp32 division, round half to even) satisfies |m| <= 2^23;
 *   5. the bit pattern of fl32((float)m * step), m taken as the integer code, equals the bit
 *      pattern of v (bits, not floats: a -0.0 weight is off-grid, since the code 0 gives +0.0);
 *   6. max m - min m <= 2^b - 1.
 * Raw therefore covers never-quantized channels (the stem, the downsample convs), a channel whose
 * codes span 2^b + 1 levels after the quantizer's rounding (functions.py:41 ties), and a channel
 * that is off its grid by one ulp.
 * Payload: every channel starts on a word boundary at word_off[c].
 *   packed   ceil(k*b / 32) words; code u_i = m_i - base occupies bits [i*b, (i+1)*b) of the
 *            channel's little-endian bit stream, stream bit j being bit j % 32 of word j / 32;
 *            unused high bits of the last word are zero
 *   raw      k words: the IEEE bit patterns of the values
 * Unpacking: w_i = fl32((float)(base + u_i) * step), one rounded multiply with no contraction,
 * which condition 5 makes bitwise the original; raw channels copy their words back.
 *
 * Entry points (caller-owned pointers, the caller's stream, no allocation; k <= 2^26; payload
 * and every array naturally aligned):
 *   smpq_bitpack_plan   applies the six conditions: mode, base and words[c] = the channel's payload
 *                       word count (int32 [cout]); one workgroup per channel
 *   smpq_bitpack_store  writes exactly the words word_off plans (each once, no atomics) and
 *                       nothing else; mode / base as planned for this w and step
 *   smpq_bitpack_load   payload -> w; an element reads the one or two words holding its code (the
 *                       second only when the code straddles it), never past word_off[cout]
 * The *_host twins are native C++ with the same arithmetic, for weights in host memory. The
 * caller guarantees mode in 0..8 and a word_off consistent with mode and k
 * (checkpoint.load_packed validates a file before any kernel runs). */
int smpq_bitpack_plan(const float* w, int cout, int k, const int8_t* qbits, const float* step, int8_t* mode,
                      int32_t* base, int32_t* words, smpq_stream_t stream);
int smpq_bitpack_store(const float* w, int cout, int k, const int8_t* mode, const int32_t* base, const float* step,
                       const int64_t* word_off, uint32_t* payload, smpq_stream_t stream);
int smpq_bitpack_load(const uint32_t* payload, int cout, int k, const int8_t* mode, const int32_t* base,
                      const float* step, const int64_t* word_off, float* w, smpq_stream_t stream);
int smpq_bitpack_plan_host(const float* w, int cout, int k, const int8_t* qbits, const float* step, int8_t* mode,
                           int32_t* base, int32_t* words);
int smpq_bitpack_store_host(const float* w, int cout, int k, const int8_t* mode, const int32_t* base,
                            const float* step, const int64_t* word_off, uint32_t* payload);
int smpq_bitpack_load_host(const uint32_t* payload, int cout, int k, const int8_t* mode, const int32_t* base,
                           const float* step, const int64_t* word_off, float* w);

/* ---- uint8 images through a per-channel table (normative) ----------------------------------------
 * After Resize / CenterCrop / ToTensor / Normalize every pixel is one of 256 fp32 values per
 * channel, so an evaluation set can be kept on the device as the uint8 it came from and replayed
 * bit for bit (smpq/batches.py ResidentSet). Values are looked up, never recomputed.
 *
 * Data layout
 *   A table is float lut[c][256] with 1 <= c <= 4. Every row is finite and strictly increasing
 *   under `<`. Images are contiguous [n][c][hw]: x in fp32, u in uint8, same indexing;
 *   ch(i) = (i / hw) % c is the channel of element i.
 * smpq_u8lut_decode(u, n, c, hw, lut, x, stream)
 *   x[i] = lut[ch(i)][u[i]]. Every element of x is written. Nothing else is written. u may start
 *   at any byte and x at any multiple of 4 (views into larger buffers); 16-byte accesses are used
 *   where both allow them and never straddle a channel plane. Stores are temporal.
 * smpq_u8lut_encode(x, n, c, hw, lut, u, bad, stream)
 *   For every element, u[i] is the largest v with lut[ch][v] <= x[i]. If there is no such v, or
 *   x[i] is NaN, u[i] = 0. An element is ON THE GRID when the bit pattern of lut[ch][u[i]] equals
 *   that of x[i] (bits, not floats: -0.0 against a +0.0 entry is off the grid). *bad (uint32,
 *   zeroed by the caller) is increased by the number of off-grid elements: one atomic per
 *   workgroup after a wave / workgroup reduction. Every byte of u is written, on the grid or not.
 * smpq_u8lut_encode_host / smpq_u8lut_decode_host
 *   Native twins with the same semantics for host memory. They validate the table and return
 *   SMPQ_E_INVALID on a row that is not finite or not strictly increasing. The device entry
 *   points cannot validate without a sync, so they trust the table (smpq.ops validates it).
 * Sizes and return codes
 *   n, c, hw >= 1, c <= 4 and n * c * hw < 2^31; anything else is SMPQ_E_SHAPE before a launch.
 *   Null or misaligned pointers are SMPQ_E_INVALID. Caller-owned pointers, the caller's stream,
 *   no allocation. */
int smpq_u8lut_decode(const uint8_t* u, int n, int c, int hw, const float* lut, float* x, smpq_stream_t stream);
int smpq_u8lut_encode(const float* x, int n, int c, int hw, const float* lut, uint8_t* u, uint32_t* bad,
                      smpq_stream_t stream);
int smpq_u8lut_decode_host(const uint8_t* u, int n, int c, int hw, const float* lut, float* x);
int smpq_u8lut_encode_host(const float* x, int n, int c, int hw, const float* lut, uint8_t* u, uint32_t* bad);

/* ---- trial row patch: one output channel of a packed weight operand, in place (normative) -------
 * A per-channel sensitivity trial (smpq/sensitivity.py) asks what the loss would be with ONE output
 * channel c of a conv quantized to b bits. With wlimbs >= 2 smpq_pack_weights_ex codes every row
 * independently of all others (no conv-wide offset, a per-channel shift), so the trial overwrites
 * that row of the operand with exactly what the normal path (smpq_quantize_channels_ex on the
 * weight, then smpq_pack_weights_ex with the recorded step, then the BN fold) would have packed,
 * and puts the saved bytes back afterwards. The fp32 weight is only read.
 *
 * Operand (K = kh*kw*cin, cin % 64 == 0, K <= SMPQ_TRIAL_MAX_K):
 *   codes      int8 [wlimbs][cout][K], k = tap*cin + ci, tap = r*kw + q (smpq_pack_weights_ex)
 *   codes_km   int8 [wlimbs][K/64][cout][64], the K-major copy (smpq_weights_kmajor), or NULL when
 *              the caller keeps none; byte (l, c, k) lives at ((l*(K/64) + k/64)*cout + c)*64 + k%64
 *   wscale     fp32 [cout]; col_scale fp32 [cout] = fl32(wscale * bn_a), bn_a fp32 [cout] the BN
 *              factor folded onto the weight scale (ones without a BN)
 * Save area: SMPQ_TRIAL_SAVE_HEADER + wlimbs*K bytes, 4-byte aligned: float[0] = wscale[c],
 *   float[1] = col_scale[c] (header bytes 8..15 unused), then the row's code bytes, limb-major
 *   (byte l*K + k). It is written FIRST, on every call that passes validation.
 * Arithmetic of the new row, per element t of w[c] (IEEE fp32 / double, no contraction):
 *   1. mn, mx = min / max of the row. mx == mn (a constant channel, where the reference raises
 *      ZeroDivisionError): status[0] = 1 and no operand byte is written (the save area holds the
 *      current row, so a restore is harmless).
 *   2. the quantizer of smpq_quantize_channels_ex: scale = ((double)mx - mn) / (2^b - 1),
 *      z = rint(mn / scale), s = (float)scale, d = t / s (SMPQ_QSEM_CPU) or t * (float)(1 / scale)
 *      (SMPQ_QSEM_DEVICE), v = fl32((rintf(d + (float)z) - (float)z) * s).
 *   3. the coder of smpq_pack_weights_ex for wlimbs >= 2 with step s, WMAX = 32512 (wlimbs 2) or
 *      8323072 (wlimbs 3): the row is ON THE GRID when s > 0 and every v has m = rintf(v / s) with
 *      fl32(m * s) == v and |m| <= WMAX. On the grid: sh = the largest shift <= 8*(wlimbs - 1) with
 *      (max|m| << sh) <= WMAX (0 when max|m| == 0), code = m << sh, wscale = ldexpf(s, -sh).
 *      Off the grid (fixed point): wscale = max|v| / WMAX (1 when max|v| == 0),
 *      code = clamp(rint((double)v / wscale), -WMAX, WMAX).
 *   4. digits: wlimbs balanced base-256 digits, low first: d = ((m + 128) & 255) - 128,
 *      m = (m - d) >> 8; the last digit is what remains.
 *   5. wscale[c] and col_scale[c] = fl32(wscale[c] * bn_a[c]) are written last.
 * One workgroup of 256 threads; plain vector stores; status is int32 [1], caller-zeroed.
 * smpq_trial_row_restore writes the save area back to both code layouts and the two scalars.
 * The *_host twins are native C++ with the same arithmetic over the row-major codes (no K-major
 * copy) for host memory.
 * Return codes, before any launch or write: SMPQ_E_INVALID for a null pointer (codes_km alone may
 * be NULL), wlimbs outside 2..3, channel outside [0, cout), semantics not SMPQ_QSEM_*, a
 * misaligned save area or non-positive sizes; SMPQ_E_SHAPE for cin % 64 != 0 or
 * K > SMPQ_TRIAL_MAX_K; SMPQ_E_BITS for bits outside 1..16. */
#define SMPQ_TRIAL_MAX_K 4608
#define SMPQ_TRIAL_SAVE_HEADER 16
int smpq_trial_row_patch(const float* w, int cout, int cin, int kh, int kw, int channel, int bits, int semantics,
                         int wlimbs, const float* bn_a, int8_t* codes, int8_t* codes_km, float* wscale,
                         float* col_scale, void* save, int32_t* status, smpq_stream_t stream);
int smpq_trial_row_restore(int cout, int K, int channel, int wlimbs, int8_t* codes, int8_t* codes_km, float* wscale,
                           float* col_scale, const void* save, smpq_stream_t stream);
int smpq_trial_row_patch_host(const float* w, int cout, int cin, int kh, int kw, int channel, int bits, int semantics,
                              int wlimbs, const float* bn_a, int8_t* codes, float* wscale, float* col_scale,
                              void* save, int32_t* status);
int smpq_trial_row_restore_host(int cout, int K, int channel, int wlimbs, int8_t* codes, float* wscale,
                                float* col_scale, const void* save);

/* ---- trial rows patch: n output channels of one packed operand at once (normative) --------------
 * A semilayer trial (smpq/sensitivity.py semilayer_table) quantizes a subset of ONE conv's output
 * channels. Row i of the call patches channel channels[i] at bits[i] bits exactly as
 * smpq_trial_row_patch would (steps 1-5 above, the same operand layouts and limits), in one launch
 * of n workgroups of 256 threads, one per row; plain vector stores.
 *   channels, bits  int32 [n], device arrays (host arrays for the *_host twins), 1 <= n <= cout
 *   save            n slots of SMPQ_TRIAL_SAVE_HEADER + wlimbs*K bytes (a multiple of 16, as
 *                   K % 64 == 0), slot i at save + i * that, each with the single-row layout;
 *                   4-byte aligned. Every slot is written first, before its row's operand bytes.
 *   status          int32 [n], caller-zeroed: status[i] = 1 for a constant row, whose operand bytes
 *                   stay as they are and whose slot holds the current row; the other rows are
 *                   patched regardless.
 * The channels must be pairwise distinct: distinct channels own distinct code bytes in both
 * layouts, distinct scalars and distinct slots, so no workgroup reads what another writes and
 * nothing is ordered across workgroups. For the device entry points that, each channel's range
 * and each bit-width are THE CALLER'S DUTY (the lists live in device memory; smpq/ops.py checks
 * them on the host before the upload). A device entry outside [0, cout) or 1..16 is skipped with
 * status[i] = 2 instead of written out of bounds; duplicates are undefined. The *_host twins check
 * all three themselves before any write: SMPQ_E_INVALID for a channel out of range or listed twice,
 * SMPQ_E_BITS for a bit-width outside 1..16.
 * smpq_trial_rows_restore writes every slot back (both code layouts and the two scalars).
 * Return codes, before any launch or write: those of smpq_trial_row_patch, and SMPQ_E_INVALID for
 * a null channels or bits pointer or n outside 1..cout. */
int smpq_trial_rows_patch(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                          const int32_t* bits, int n, int semantics, int wlimbs, const float* bn_a, int8_t* codes,
                          int8_t* codes_km, float* wscale, float* col_scale, void* save, int32_t* status,
                          smpq_stream_t stream);
int smpq_trial_rows_restore(int cout, int K, const int32_t* channels, int n, int wlimbs, int8_t* codes,
                            int8_t* codes_km, float* wscale, float* col_scale, const void* save,
                            smpq_stream_t stream);
int smpq_trial_rows_patch_host(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                               const int32_t* bits, int n, int semantics, int wlimbs, const float* bn_a, int8_t* codes,
                               float* wscale, float* col_scale, void* save, int32_t* status);
int smpq_trial_rows_restore_host(int cout, int K, const int32_t* channels, int n, int wlimbs, int8_t* codes,
                                 float* wscale, float* col_scale, const void* save);

/* ---- trial rows patch, exact8 operands: rows of a fully quantized conv's operand (normative) -----
 * A conv whose every channel is quantized is packed by smpq_pack_weights_ex with wlimbs == 1: one
 * int8 plane, a per-channel offset that the conv kernels read from memory at run time, wscale = the
 * recorded step. That coder too reads nothing but the row itself (its codes, offset[c], wscale[c]),
 * so a search trial that RE-quantizes some channels of such a conv (smpq/search.py) overwrites
 * their rows in place, as smpq_trial_rows_patch does for wlimbs >= 2, with exactly what
 * smpq_quantize_channels_ex on the weight, smpq_pack_weights_ex(wlimbs = 1) with the new steps and
 * the BN fold would have left there. The fp32 weight is only read.
 *
 * Operand (K = kh*kw*cin, cin % 64 == 0, K <= SMPQ_TRIAL_MAX_K):
 *   codes      int8 [1][cout][K], k = tap*cin + ci; codes_km int8 [1][K/64][cout][64] or NULL
 *   offset     int32 [cout], or NULL for an operand packed without offsets (the conv kernels then
 *              run without them, so a row that needs one cannot be patched: status 4)
 *   wscale, col_scale, bn_a   as for smpq_trial_row_patch
 *   channels, bits, status    int32 [n] as for smpq_trial_rows_patch, bits within 1..8
 *   save       n slots of SMPQ_TRIAL_SAVE_HEADER + K bytes, 4-byte aligned, slot i at save + i * that:
 *              float[0] = wscale[c], float[1] = col_scale[c], the int32 at byte 8 = offset[c] (0 when
 *              offset == NULL), bytes 12..15 unused, then the row's K code bytes. A slot is written
 *              FIRST, before its row's operand bytes.
 * Arithmetic of row c at b bits (IEEE fp32 / double, no contraction):
 *   1-2. steps 1 and 2 of smpq_trial_row_patch: the row's min / max, the constant row (status 1),
 *      the quantizer under both semantics, giving s and the quantized values v.
 *   3. the wlimbs == 1 coder of smpq_pack_weights_ex with step s: the row is ON THE GRID when s > 0
 *      and every v has m = rintf(v / s) with fl32(m * s) == v and |m| <= 32512. mmin / mmax = the
 *      smallest / largest m. Off the grid, or mmax - mmin > 255: status 3 (the normal path would
 *      not pack this conv exact8).
 *   4. o = mmin + 128 when mmin < -128 or mmax > 127, else 0. o != 0 with offset == NULL: status 4.
 *   5. code = m - o, one int8, to both layouts; then offset[c] = o (when offset != NULL),
 *      wscale[c] = s, col_scale[c] = fl32(s * bn_a[c]).
 * status[i] (caller-zeroed): 0 patched; 1 constant row; 2 list entry out of range (a channel
 * outside [0, cout): nothing touched; a bit-width outside 1..8, since a wider row cannot be exact8:
 * the slot is written); 3; 4. On every nonzero status the row's operand bytes stay as they are, and
 * except for a channel out of range its slot holds the current row, so a restore is harmless.
 * One workgroup of 256 threads per row; plain vector stores; distinct channels own distinct bytes,
 * scalars and slots, so nothing is ordered across workgroups. Lists as for smpq_trial_rows_patch:
 * the device entry points leave range and distinctness to the caller (smpq/ops.py checks them
 * before the upload); the *_host twins check them first (SMPQ_E_INVALID; SMPQ_E_BITS for a
 * bit-width outside 1..8).
 * smpq_trial_rows_restore_x8 writes every slot back: both code layouts, offset[c] when
 * offset != NULL, the two scalars.
 * Return codes, before any launch or write: SMPQ_E_INVALID for a null pointer (codes_km and offset
 * may be NULL), non-positive sizes, n outside 1..cout, semantics not SMPQ_QSEM_*, a misaligned save
 * area; SMPQ_E_SHAPE for cin % 64 != 0 (restore: K % 64 != 0) or K > SMPQ_TRIAL_MAX_K. */
int smpq_trial_rows_patch_x8(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                             const int32_t* bits, int n, int semantics, const float* bn_a, int8_t* codes,
                             int8_t* codes_km, int32_t* offset, float* wscale, float* col_scale, void* save,
                             int32_t* status, smpq_stream_t stream);
int smpq_trial_rows_restore_x8(int cout, int K, const int32_t* channels, int n, int8_t* codes, int8_t* codes_km,
                               int32_t* offset, float* wscale, float* col_scale, const void* save,
                               smpq_stream_t stream);
int smpq_trial_rows_patch_x8_host(const float* w, int cout, int cin, int kh, int kw, const int32_t* channels,
                                  const int32_t* bits, int n, int semantics, const float* bn_a, int8_t* codes,
                                  int32_t* offset, float* wscale, float* col_scale, void* save, int32_t* status);
int smpq_trial_rows_restore_x8_host(int cout, int K, const int32_t* channels, int n, int8_t* codes, int32_t* offset,
                                    float* wscale, float* col_scale, const void* save);

/* ---- trial rows conv: a few output channels of one conv, into limb planes we hold (normative) -----
 * A per-channel trial of a block's LAST conv changes one channel of that conv's output, which is the
 * next block's input: a tensor the sensitivity table already keeps (smpq/suffix.py). Instead of
 * running the block again, smpq_trial_rows_conv_q computes the listed output channels of the conv
 * from its (patched) operand and writes them in place into the kept limb planes, after saving the
 * bytes it replaces; smpq_trial_rows_conv_restore puts those bytes back. Additions to ABI 7.
 *
 * The conv is smpq_conv2d_fwd_q in its static limb-plane output mode (y == NULL, yq and yq_range
 * given, no fp32 residual, no y_absmax) with ReLU on, wlimbs >= 2 and no offsets:
 *   xq [limbs][n][h][w][cin], x_absmax [n]; codes [wlimbs][cout][K] row-major (k = tap*cin + ci);
 *   col_scale, col_shift [cout]; residual_q [limbs][n*h*w][cout] with residual_range, or NULL;
 *   yq [limbs][n*h*w][cout], updated in place; yq_range > 0; overflow int32 [1].
 * Geometries: 1x1 / stride 1 / pad 0 and 3x3 / stride 1 / pad 1 (output pixels = input pixels,
 * M = n*h*w), cin % 64 == 0, K = kh*kw*cin <= SMPQ_TRIAL_MAX_K, cout % 16 == 0, limbs 2 or 3,
 * wlimbs 2 or 3 (3 with limbs == 3 only).
 *   channels  int32 [nrows], 1 <= nrows <= cout, pairwise distinct, device memory for the device
 *             entry point (range and distinctness are THE CALLER'S DUTY there, smpq/ops.py checks
 *             them before the upload; an entry outside [0, cout) is skipped); the *_host twins
 *             check the list themselves (SMPQ_E_INVALID)
 *   save      nrows slots of limbs*M bytes: slot i holds channel channels[i]'s old digit bytes,
 *             byte l*M + m for limb l of pixel m. Each byte is saved before it is overwritten.
 * Per listed channel c and output pixel m (image g), IEEE fp32, no contraction:
 *   1. acc_s = the exact int32 sum over k and over the limb pairs (la, lw) with la + lw - SMIN == s
 *      of x_digit_la(m, k) * w_digit_lw(c, k), SMIN = max(0, limbs + wlimbs - 4), for the
 *      NACC = limbs + wlimbs - 1 - SMIN values of s: the pairs with la + lw < SMIN are skipped, as
 *      the conv kernels skip them. A 3x3 tap outside the image contributes zero. The int32 bound is
 *      the conv's (K <= SMPQ_TRIAL_MAX_K).
 *   2. v = (float)acc_0 [* 256^SMIN when SMIN > 0], then v = fmaf((float)acc_s, 256^(SMIN + s), v)
 *      for s = 1 .. NACC-1.
 *   3. inv = QMAX / yq_range; z = fmaf(v, (x_absmax[g] * (1 / QMAX)) * (col_scale[c] * inv),
 *      col_shift[c] * inv); with a residual z = fmaf((float)r, (residual_range / QMAX) * inv, z),
 *      r = the residual's code at (m, c). QMAX = 32512 (limbs 2) or 8323072 (limbs 3).
 *   4. zr = rintf(z); overflow[0] is set to 1 when zr > QMAX, exactly when the conv would;
 *      code = min(max(zr, 0), QMAX), written as `limbs` balanced base-256 digits, low first.
 * These are the conv kernels' own operations (csrc/lds_dma.h lean_v1 / lean_zr / lean_clamp), so the listed
 * channels come out bit for bit as a full smpq_conv2d_fwd_q launch would write them; every other
 * byte of yq is left alone. Grid: (pixel tiles of 64) x rows, 256 threads, the row's wlimbs*K weight
 * bytes staged once in LDS, activations read in 16-byte pieces, v_dot4_i32_i8 accumulation; all
 * stores are plain vector stores.
 * Return codes, before any launch or write: SMPQ_E_INVALID for a null pointer (residual_q alone may
 * be NULL), limbs or wlimbs outside 2..3 (or wlimbs 3 with limbs 2), nrows outside 1..cout, a range
 * that is not > 0, xq or codes not 16-byte aligned; SMPQ_E_SHAPE for another geometry, non-positive
 * sizes, cin % 64 != 0, K > SMPQ_TRIAL_MAX_K, cout % 16 != 0 or n*h*w >= 2^31. */
int smpq_trial_rows_conv_q(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin, const int8_t* codes,
                           int wlimbs, int cout, int kh, int kw, int stride, int pad, const float* col_scale,
                           const float* col_shift, int limbs, const int8_t* residual_q, float residual_range,
                           const int32_t* channels, int nrows, int8_t* yq, float yq_range, int32_t* overflow,
                           void* save, smpq_stream_t stream);
/* pixels = n*h*w of the patched call; writes every slot back. */
int smpq_trial_rows_conv_restore(const int32_t* channels, int nrows, int limbs, int64_t pixels, int cout, int8_t* yq,
                                 const void* save, smpq_stream_t stream);
int smpq_trial_rows_conv_q_host(const int8_t* xq, const float* x_absmax, int n, int h, int w, int cin,
                                const int8_t* codes, int wlimbs, int cout, int kh, int kw, int stride, int pad,
                                const float* col_scale, const float* col_shift, int limbs, const int8_t* residual_q,
                                float residual_range, const int32_t* channels, int nrows, int8_t* yq, float yq_range,
                                int32_t* overflow, void* save);
int smpq_trial_rows_conv_restore_host(const int32_t* channels, int nrows, int limbs, int64_t pixels, int cout,
                                      int8_t* yq, const void* save);

/* Diagnostics: one v_mfma_i32_16x16x64_i8 with the kernel's fragment mapping.
 *   a [16][64] int8 row-major, b [16][64] int8 (b[col][k]), c [16][16] int32 row-major */
int smpq_debug_mfma_i8(const int8_t* a, const int8_t* b, int32_t* c, smpq_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SMPQ_H_ */
