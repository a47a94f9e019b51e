/*
 * dcvc_amd_ops.h - C ABI of the individual HIP kernels (libdcvc_amd.so).
 *
 * One entry point per device function the reference's proxies call
 *   /root/reference/src/layers/extensions/inference/def_cutlass.h:10-40     (fused conv ops)
 *   /root/reference/src/layers/extensions/inference/def_elementwise.h:10-78 (elementwise ops)
 * with at::Tensor replaced by (device pointer, leading dimension, sizes). All tensors are fp16
 * NHWC ("channels_last") on the current HIP device; `stream` is a hipStream_t (0 = default).
 * Nothing allocates or synchronises. Returns 0, or -1 with dcvc_last_error() set.
 */
#ifndef DCVC_AMD_OPS_H
#define DCVC_AMD_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* message of the last failing call on this thread (every dcvc_* entry point reports errors through it) */
#ifndef DCVC_LAST_ERROR_DECLARED
#define DCVC_LAST_ERROR_DECLARED
const char* dcvc_last_error(void);
#endif

/* flags for dcvc_conv1x1 */
#define DCVC_CONV_WSILU      1   /* y = wsilu(acc + bias)                     (conv1x1_bias_wsilu)            */
#define DCVC_CONV_CHUNK_ADD  2   /* sum of 4 adjacent output channels         (conv1x1_bias_wsilu_chunk_add)  */

/* def_cutlass.h:10-33: conv1x1_bias / _wsilu / _shortcut / _shortcut2 / _shortcut_with_quant /
 * _with_quant / _wsilu_chunk_add, selected by which optional pointers are non-NULL and `flags`.
 *   y[p][n] = fp16( ((acc + bias[n]) (wsilu) + r1[p][n] + r2[p][n]) * q[n] ), then * q2[n] in fp16.
 * x: [pixels][ldx] (first cin channels), w: [cout][cin], y: [pixels][ldy]. */
int dcvc_conv1x1(const void* x, int ldx, const void* w, const void* bias,
                 const void* r1, int ldr1, const void* r2, int ldr2,
                 const void* q, const void* q2, void* y, int ldy,
                 int pixels, int cin, int cout, int flags, void* stream);

/* def_cutlass.h:35-37 conv_bias: dense k x k conv (k in {2,3}), stride in {1,2}, zero padding.
 * w: [cout][k][k][cin] (tap-major re-layout of the PyTorch [cout][cin][k][k] weight). */
int dcvc_conv_kxk(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy,
                  int in_h, int in_w, int cin, int cout, int ksize, int stride, int pad,
                  void* stream);

/* def_cutlass.h:39-40 transposed_conv: 2x2, stride 2, no bias. w: [4 = dy*2+dx][cout][cin].
 * cout must be a multiple of 128 (a channel tile of the one launch must not straddle two output pixels): cout = 192 and
 * other such widths are rejected with an error, not computed (tests/test_gemm_matrix_gpu.py). */
int dcvc_tconv2x2(const void* x, int ldx, const void* w, void* y, int ldy,
                  int in_h, int in_w, int cin, int cout, void* stream);

/* def_cutlass.h:34 d3x3: depthwise 3x3, pad 1, no bias. w: [9][C]. */
int dcvc_dwconv3x3(const void* x, int ldx, const void* w, void* y, int ldy, int H, int W, int C,
                   void* stream);

/* def_elementwise.h: pad_and_unshuffle_8_cuda / pixel_shuffle_8_cuda / pixel_shuffle_2_cuda /
 * replicate_pad_cuda / slice_cuda / multiply_with_broadcast_cuda */
int dcvc_pad_unshuffle8(const void* x, int H, int W, int C3, void* out, int H8, int W8, void* stream);
int dcvc_shuffle8(const void* in, int ldin, int H8, int W8, int C3, int clamp, void* out, void* stream);
int dcvc_shuffle2(const void* in, int ldin, int H, int W, int C, void* out, int ldout, void* stream);
int dcvc_replicate_pad(const void* in, int ldin, int H, int W, int C, int pad_b, int pad_r,
                       void* out, int ldout, void* stream);
int dcvc_crop(const void* in, int ldin, int Win, void* out, int ldout, int H, int W, int C, void* stream);
int dcvc_mul_channel(const void* x, int ldx, const void* q, void* y, int ldy, int pixels, int C,
                     void* stream);
/* pad_unshuffle8 into a wider row: out [H8][W8][ldout], ldout >= 64 * C3 (the inter codecs write the source picture into a
 * channel slice of a concatenation buffer this way) */
int dcvc_pad_unshuffle8_ld(const void* x, int H, int W, int C3, void* out, int ldout, int H8, int W8, void* stream);
/* Every entry of this group and its batched form below refuse, before any launch (return < 0, dcvc_last_error names the
 * entry): null pointers, sizes <= 0, C not a multiple of 8, a leading dimension below the channel count, negative padding,
 * an output smaller than the picture and, on every side that the kernel moves 16 bytes at a time, a pointer that is not
 * 16-byte aligned or a leading dimension that is not a multiple of 8. */

/* Not part of the reference surface: batched forms for the intra batches. n (1..16) pictures back to back
 * on both sides, each with the per-picture geometry of the single form above; n = 1 is the single launch. The halo,
 * padding and edge replication of every picture stay inside it. crop_b also takes the input picture's height Hin.
 * conv_kxk_b / tconv2x2_b: in_h is one picture's height. */
int dcvc_dwconv3x3_b(const void* x, int ldx, const void* w, void* y, int ldy, int H, int W, int C, int n, void* stream);
int dcvc_conv_kxk_b(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy, int in_h, int in_w, int cin,
                    int cout, int ksize, int stride, int pad, int n, void* stream);
int dcvc_tconv2x2_b(const void* x, int ldx, const void* w, void* y, int ldy, int in_h, int in_w, int cin, int cout, int n,
                    void* stream);
int dcvc_pad_unshuffle8_b(const void* x, int H, int W, int C3, void* out, int H8, int W8, int n, void* stream);
int dcvc_shuffle8_b(const void* in, int ldin, int H8, int W8, int C3, int clamp, void* out, int n, void* stream);
int dcvc_replicate_pad_b(const void* in, int ldin, int H, int W, int C, int pad_b, int pad_r, void* out, int ldout, int n,
                         void* stream);
int dcvc_crop_b(const void* in, int ldin, int Hin, int Win, void* out, int ldout, int H, int W, int C, int n, void* stream);

/* ffn.0 + ffn.2 of a DepthConvBlock in one launch (layers_proxy.cpp:84-98: conv1x1_bias_wsilu_chunk_add
 * followed by conv1x1_bias_shortcut[2][_with_quant] with the block-internal tensor as first residual):
 *   out = W2 * chunk_add(WSiLU(W0 * x + b0)) + b2 + x [+ r2] [* q], rounded to fp16, [* q2].
 * c in {128, 256, 384}, cffn a multiple of 64; bit-identical to the two-launch sequence; y may alias x. */
int dcvc_ffn_fused(const void* x, int ldx, const void* w0, const void* b0, const void* w2, const void* b2,
                   const void* r2, int ldr2, const void* q, const void* q2, void* y, int ldy,
                   int pixels, int c, int cffn, void* stream);

/* A DepthConvBlock behind its depthwise conv in ONE launch (layers_proxy.cpp:81-98: conv1x1_bias_shortcut,
 * conv1x1_bias_wsilu_chunk_add, conv1x1_bias_shortcut[2][_with_quant]), optionally followed by dc.0 of the NEXT block of a
 * chain (conv1x1_bias_wsilu, layers_proxy.cpp:79):
 *   y1 = W3 * t2 + b3 + x;  y = (W2 * chunk_add(WSiLU(W0 * y1 + b0)) + b2 + y1 [+ x]) [* q] -> fp16 [* q2];
 *   t1n = WSiLU(W1n * y + b1n)   (when w1n != NULL).
 * t2 = depthwise output [pixels][ldt], x = block input [pixels][ldx], b3 = dc.3 bias with the depthwise bias folded in,
 * ci = inner width (cdc = cffn). Bit-identical to the separate launches; y may alias x when !shortcut.
 * The N-split kernel (round 3: activations in LDS, every wave owns a share
 * of the output channels and streams its weight fragments from a packed copy of w3 | w0 | w2 [| w1n] that this entry point
 * builds on EVERY call in stream-ordered temporaries - the codecs pack once at set_param time; callers that launch many
 * times use the handle form below).
 * (c, ci) in {(256, 256), (384, 384), (512, 512), (768, 768)} - full-width blocks - and {(512, 256), (256, 128)}: the
 * half-width `dcb2` blocks of the inter models (layers.py:128-159; w3 [c][ci], w0 [4 ci][c], w2 [c][ci], w1n [ci][c]).
 * Bit-identical to dcvc_dcb_tail and to the separate launches. */
int dcvc_dcb_nsplit(const void* t2, int ldt, const void* x, int ldx, const void* w3, const void* b3,
                    const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                    const void* w1n, const void* b1n, void* t1n, int ldt1, void* y, int ldy,
                    int pixels, int c, int ci, int shortcut, void* stream);
/* The same block as the LAST one of a chain, with the 1x1 conv that closes the chain inside the launch (round 6; the reference
 * launches conv1x1_bias / conv1x1_bias_with_quant behind the block: y_prior_fusion.conv.3 dmci_proxy.cpp:172-176,
 * y_spatial_prior.conv.3 dmci_proxy.cpp:196-199, decoder.conv2 dmc_ld_proxy.cpp:484-487, recon_head.head :499-503):
 *   yfin = (Wfin * y + bfin) [* qfin] -> fp16,  Wfin [nfin][c].
 * Returns an error for an (c, ci, nfin) the kernel has no variant of (dcvc_dcb_nsplit_fin_supported). Bit-identical to
 * dcvc_dcb_nsplit followed by dcvc_conv1x1(bias [, q]). */
int dcvc_dcb_nsplit_fin(const void* t2, int ldt, const void* x, int ldx, const void* w3, const void* b3,
                        const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                        const void* wfin, const void* bfin, const void* qfin, void* yfin, int ldyfin, int nfin,
                        void* y, int ldy, int pixels, int c, int ci, int shortcut, void* stream);
int dcvc_dcb_nsplit_fin_supported(int c, int ci, int nfin);
/* The same block WITH its depthwise 3x3 conv inside the launch (round 6; the reference launches d3x3 between dc.0 and dc.3,
 * layers_proxy.cpp:80-84, cutlass/d3x3.cu:443-446): t1 [pixels][ldt] = dc.0's output (what dcvc_dwconv3x3 would read), wdw = the
 * taps [9][ci] (tap major, as dcvc_dwconv3x3 takes them), width = the picture's width (pixels = rows x width, row-major). Behind
 * ffn.2 either dc.0 of the next block (w1n / b1n / t1n; t1n must not be t1) or a chain's closing conv (wfin ... nfin) or neither.
 * Returns an error for a (c, ci, pixels) the kernel has no such variant of (dcvc_dcb_nsplit_dw_supported: (256, 128); (384, 192) below
 * 12 800 pixels, where the workgroups take 32 pixels and LDS has room for the rows around them). Bit-identical to
 * dcvc_dwconv3x3 followed by dcvc_dcb_nsplit / dcvc_dcb_nsplit_fin. */
int dcvc_dcb_nsplit_dw(const void* t1, int ldt, const void* wdw, int width, const void* x, int ldx, const void* w3, const void* b3,
                       const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                       const void* w1n, const void* b1n, void* t1n, int ldt1,
                       const void* wfin, const void* bfin, const void* qfin, void* yfin, int ldyfin, int nfin,
                       void* y, int ldy, int pixels, int c, int ci, int shortcut, void* stream);
int dcvc_dcb_nsplit_dw_supported(int c, int ci, int pixels);

/* The two 1x1 convs in FRONT of a block's depthwise conv in one launch (round 6; the reference launches conv1x1_bias for the
 * adaptor, layers_proxy.cpp:73-77, then conv1x1_bias_wsilu for dc.0, :79):
 *   y = Wa * x + ba  (Wa [c][cin]);   t1 = WSiLU(W1 * y + b1)  (W1 [ci][c]).
 * Returns an error for a (cin, c, ci) the kernel has no variant of (dcvc_dcb_pair_supported). y must not alias x.
 * Bit-identical to dcvc_conv1x1(bias) followed by dcvc_conv1x1(bias, wsilu). */
int dcvc_dcb_pair(const void* x, int ldx, const void* wa, const void* ba, const void* w1, const void* b1,
                  void* y, int ldy, void* t1, int ldt1, int pixels, int cin, int c, int ci, void* stream);
int dcvc_dcb_pair_supported(int cin, int c, int ci);

/* Handle form: pack w3 | w0 | w2 (and w1n, or NULL) once - the packed copies are a snapshot of the weights at pack time -,
 * launch any number of times, free (synchronises the device the handle was packed on, whichever is current). `stream` of
 * _pack and of _packed may differ: _packed orders its stream behind the pack launches (an event recorded by _pack; only until
 * the event has been seen complete, and never on the pack stream itself). A stream that is being CAPTURED into a hipGraph must not
 * be the first to launch with a handle packed on another stream: pack and first launch belong in front of the capture.
 * with_next != 0 runs the next block's dc.0 inside the launch (the handle must have been packed with w1n). No reference counterpart: the reference's CUTLASS kernels read the
 * row-major matrices directly. */
int dcvc_dcb_nsplit_pack(const void* w3, const void* w0, const void* w2, const void* w1n, int c, int ci, void* stream,
                         void** handle);
int dcvc_dcb_nsplit_packed(const void* handle, const void* t2, int ldt, const void* x, int ldx, const void* b3,
                           const void* b0, const void* b2, const void* q, const void* q2, const void* b1n,
                           void* t1n, int ldt1, void* y, int ldy, int pixels, int shortcut, int with_next, void* stream);
int dcvc_dcb_nsplit_free(void* handle);

/* DepthConvBlockProxy::forward behind dc.0 (layers_proxy.cpp:79-98: d3x3, conv1x1_bias_shortcut,
 * conv1x1_bias_wsilu_chunk_add, conv1x1_bias_shortcut[2][_with_quant]) in one launch for the
 * half-width blocks of the inter models: t = dc.0 output [H*W][ldt]; dw = [9][cdc] tap-major depthwise
 * weights (NULL: t already is the depthwise output); x = block-internal input (residual of dc.3, and
 * of ffn.2 when shortcut != 0); c in {128, 256}, cdc <= 128, cffn: multiples of 64. Bit-identical to
 * the four-launch sequence; y may alias x. With w1 / b1 (dc.0 weights [cdc][c] and bias) non-NULL, dc.0
 * (conv1x1_bias_wsilu on x) runs inside the launch too and t is not read - the whole block behind an
 * optional adaptor in one launch; y must then NOT alias x (patches read their neighbours' input). */
int dcvc_dcb_tail(const void* w1, const void* b1, const void* t, int ldt, const void* dw, const void* x, int ldx,
                  const void* w3, const void* b3,
                  const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                  void* y, int ldy, int H, int W, int c, int cdc, int cffn, int shortcut, void* stream);
/* Batched form of dcvc_dcb_tail (intra batches): n (1..16) pictures of H x W back to back in t, x and y, each with its own
 * halo (the depthwise conv and dc.0 inside never read a neighbouring picture). Refuses, like the other _b forms, n outside
 * 1..16, null operands, non-positive sizes and leading dimensions below the channel counts. */
int dcvc_dcb_tail_b(const void* w1, const void* b1, const void* t, int ldt, const void* dw, const void* x, int ldx,
                    const void* w3, const void* b3,
                    const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                    void* y, int ldy, int H, int W, int c, int cdc, int cffn, int shortcut, int n, void* stream);

/* Debugging aid (no reference counterpart): device buffer [H*W][cdc] that receives dc.0's output from
 * the following dcvc_dcb_tail launches with dc.0 inside; NULL = off. */
int dcvc_dcb_tail_debug_buffer(void* device_buffer);

/* stream.cu:40-76 / 422-443: y = x * max(q, 0.5) or, with reciprocal != 0, y = x * fp16(1 / max(q, 0.5));
 * q is a tensor of the same shape (the inter models' per-element quantisation step). */
int dcvc_scale_clamped(const void* x, int ldx, const void* q, int ldq, void* y, int ldy, int pixels,
                       int C, int reciprocal, void* stream);

/* Picture I/O on the device, replacing the host-side numpy/scipy/torch chains of the harness.
 * test_video.py:69-123 get_src_frame (+ transforms.py:69-80 ycbcr420_to_444_np, order 0):
 *   y: u8 [H][W], uv: u8 [2][H/2][W/2] (device) -> x fp16 at pixel stride ldx (3 channels written):
 *   nearest chroma, x = fp16(fp16(v / 255) - 0.5). H, W positive and even, ldx >= 3, no NULL operand: refused otherwise.
 *   The same kernels as dcvc_pix_to_x / dcvc_x_to_pix at DCVC_PIX_YUV420P, 8 bits, behind separate plane pointers. */
int dcvc_yuv420_to_x(const void* y, const void* uv, int H, int W, void* x, int ldx, void* stream);
/* test_video.py:32-45 get_distortion and :356-363 (decoded-picture writer):
 *   x_hat fp16 [rows][row_pixels][3] -> top-left H x W picture; y16/uv16: fp16 planes in 0..255,
 *   y8/uv8: u8 planes (Y rounded half-to-even, U/V truncated as the reference does). Each of the four: NULL = skip;
 *   with all four NULL the call returns 0 without a launch. */
int dcvc_x_to_yuv420(const void* x_hat, int row_pixels, int H, int W, void* y16, void* uv16, void* y8,
                     void* uv8, void* stream);

/* High-bit-depth YUV420 (yuv420p10le and the like: uint16 samples of bit depth 9..16, max_val = 2^bit_depth - 1; DCVC-FM's
 * YUVReader / YUVWriter, video_reader.py:130-183, video_writer.py:86-130). H, W positive and even.
 *   y: u16 [H][W], uv: u16 [2][H/2][W/2] (device) -> x fp16 at pixel stride ldx >= 3 (3 channels written): nearest chroma,
 *   x = fp16(fp16(fp32(v) / fp32(max_val)) - 0.5), a correctly rounded division. Samples above max_val are not checked. */
int dcvc_yuv420p16_to_x(const void* y, const void* uv, int H, int W, int bit_depth, void* x, int ldx, void* stream);
/*   x_hat fp16 [rows][row_pixels][3] -> top-left H x W picture; dist32: fp32 [H][W] then [2][H/2][W/2], the distortion
 *   planes clamp(fp32(t) * max_val, 0, max_val) with t = fp16(x_hat + 0.5) (Y) or fp16(2 x 2 fp32 mean of it) (U, V), as
 *   dcvc_x_to_yuv420 before its * 255; yuv16: u16 samples in the same layout, rint(dist32) (half to even, all planes).
 *   NULL = skip. */
int dcvc_x_to_yuv420p16(const void* x_hat, int row_pixels, int H, int W, int bit_depth, void* dist32, void* yuv16, void* stream);

/* Other chroma formats (no reference counterpart beyond the arithmetic above: the same per-sample rules on other layouts).
 * One picture is contiguous, in file layout: Y [H][W], then Cb and Cr as planes [2][Hc][Wc] or, for DCVC_PIX_NV12,
 * interleaved [Hc][Wc][2]; Hc = H except for the two 4:2:0 layouts (H / 2), Wc = W for 4:4:4, else W / 2. bit_depth 8: u8
 * samples, max_val = 255; 9..16: u16 little-endian, max_val = 2^b - 1, LSB-aligned in the planar formats (yuv4xxp10le) and in
 * the high b bits for DCVC_PIX_NV12 (P010 / P012 / P016). H and W are positive and even for every format: odd 4:4:4 sides are
 * out of scope. Pictures whose H ceil(W / 8) does not fit a 32-bit thread index are refused ("picture too large"). */
#define DCVC_PIX_YUV420P 0
#define DCVC_PIX_YUV422P 1
#define DCVC_PIX_YUV444P 2
#define DCVC_PIX_NV12    3
/* samples per picture, H W + 2 Hc Wc; < 0 for a bad argument (host only) */
long long dcvc_pix_picture_samples(int fmt, int H, int W);
/*   src (device) -> x fp16 at pixel stride ldx >= 3 (3 channels written, the others untouched): per sample
 *   x = fp16(fp16(fp32(v) / fp32(max_val)) - 0.5), a correctly rounded division (dcvc_yuv420_to_x / dcvc_yuv420p16_to_x);
 *   chroma is nearest-neighbour, sample (h >> sub_h, w >> sub_w); P010 reads v >> (16 - b) and ignores the low bits.
 *   planar (optional): the picture as LSB-aligned planar samples, Y [H][W] then [2][Hc][Wc], u8 or u16 - the source as the
 *   metrics want it; a plain copy for the planar formats. x or planar may be NULL, not both. Samples above max_val are not
 *   checked. */
int dcvc_pix_to_x(const void* src, int fmt, int bit_depth, int H, int W, void* x, int ldx, void* planar, void* stream);
/*   x_hat fp16 [rows][row_pixels][3] -> top-left H x W picture. t = fp16(x_hat + 0.5) for Y; chroma t: the same (4:4:4),
 *   fp16((fp32(t_left) + fp32(t_right)) * 0.5f) (4:2:2), or fp16(sum * 0.25f) of the 2 x 2 block summed in fp32 in the order
 *   (0, 0), (0, 1), (1, 0), (1, 1) (4:2:0, as dcvc_x_to_yuv420). dist32: planar fp32 [H][W] then [2][Hc][Wc] - at 8 bits
 *   fp32 of dcvc_x_to_yuv420's fp16 planes (clamp(fp16(t * 255), 0, 255)), at 9..16 bits clamp(fp32(t) * max_val, 0, max_val).
 *   out: the samples in file layout, rint(dist32) (half to even) on every plane - except that DCVC_PIX_YUV420P and
 *   DCVC_PIX_NV12 at 8 bits truncate Cb / Cr as dcvc_x_to_yuv420 does (the reference writer's quirk, kept so that one stream
 *   decodes to the same samples in both 4:2:0 layouts; 4:2:2 and 4:4:4 have no reference writer and round). P010 stores
 *   s << (16 - b). Either output may be NULL; with both NULL the call returns 0 without a launch.
 * DCVC_PIX_YUV420P and DCVC_PIX_NV12 give the bits of dcvc_yuv420_to_x, dcvc_x_to_yuv420, dcvc_yuv420p16_to_x and
 * dcvc_x_to_yuv420p16, up to the layout: those four run the kernels of these two. */
int dcvc_x_to_pix(const void* x_hat, int row_pixels, int H, int W, int fmt, int bit_depth, void* dist32, void* out, void* stream);

/* Wire formats (no reference counterpart): the layouts capture cards, cameras and hardware decoders hand over,
 * converted to and from a carrier - the DCVC_PIX_* layout that holds the same samples at the same subsampling - in a pass of
 * its own in front of dcvc_pix_to_x and behind dcvc_x_to_pix. One picture, little-endian:
 *   DCVC_WIRE_NV21  Y [H][W], then [H/2][W/2][2] as Cr, Cb; 8 bits; carrier DCVC_PIX_NV12 (the pairs swapped)
 *   DCVC_WIRE_NV16  Y [H][W], then [H][W/2][2] as Cb, Cr; 8 bits, or 9..16: u16 with the value in the high b bits (P210)
 *   DCVC_WIRE_UYVY  [H][W/2] x (Cb, Y0, Cr, Y1) bytes; 8 bits
 *   DCVC_WIRE_YUY2  [H][W/2] x (Y0, Cb, Y1, Cr); 8 bits, or 9..16: u16 with the value in the high b bits (Y210 / Y212 / Y216)
 *   DCVC_WIRE_V210  rows of 128 ceil(W / 48) bytes; 6 pixels in four 32-bit words, three 10-bit fields each at bits 0-9, 10-19,
 *                   20-29: w0 = Cb0 Y0 Cr0, w1 = Y1 Cb2 Y2, w2 = Cr2 Y3 Cb4, w3 = Y4 Cr4 Y5; 10 bits
 * The last four have the carrier DCVC_PIX_YUV422P. `carrier` is one picture in the carrier's file layout, what dcvc_pix_to_x
 * takes and dcvc_x_to_pix writes: u8 at 8 bits, u16 above, LSB-aligned for DCVC_PIX_YUV422P.
 *   unpack: high-aligned samples are read as v >> (16 - b), v210 fields with & 1023; the low bits, bits 30-31, fields past W and
 *   the row padding are ignored. Samples above max_val are neither checked nor masked.
 *   pack: high-aligned samples are stored as (s << (16 - b)) & 0xFFFF, v210 fields as s & 1023; bits 30-31, the fields of a
 *   last group past W and the row padding are written as zero: every byte of dcvc_wire_picture_bytes is defined.
 *   pack(unpack(p)) == p for a p whose ignored bits are zero, unpack(pack(c)) == c for a c with samples <= max_val.
 * One launch per call on `stream`, no allocation, no host synchronisation. Refused before the launch (dcvc_last_error names
 * the wire entry): a NULL operand, an unknown format, a depth the format does not have, sides that are not positive and even,
 * a picture too large for 32-bit thread indices, source and destination ranges that overlap. */
#define DCVC_WIRE_NV21 0
#define DCVC_WIRE_NV16 1
#define DCVC_WIRE_UYVY 2
#define DCVC_WIRE_YUY2 3
#define DCVC_WIRE_V210 4
int       dcvc_wire_carrier(int wire);                                    /* DCVC_PIX_*, < 0: unknown; host only */
long long dcvc_wire_picture_bytes(int wire, int bit_depth, int H, int W); /* file bytes of one picture, < 0: refused; host only */
int dcvc_wire_unpack(const void* src, int wire, int bit_depth, int H, int W, void* carrier, void* stream);
int dcvc_wire_pack(const void* carrier, int wire, int bit_depth, int H, int W, void* dst, void* stream);

/* sample types of dcvc_msssim (U8, F16) and of dcvc_sse / dcvc_sse_ws / dcvc_msssim_range (all four; 2 is unassigned) */
#define DCVC_SAMPLE_U8  0
#define DCVC_SAMPLE_F16 1
#define DCVC_SAMPLE_U16 3
#define DCVC_SAMPLE_F32 4
/* metrics.py:27-91 calc_msssim on the GPU, one value per plane. n_planes planes of H x W samples (u8, or fp16 holding 0..255);
 * src and rec share the geometry (row_stride, plane_stride in samples). out: device memory, n_planes doubles, written
 * asynchronously on `stream`. fp64 after the load; 5 levels when both sides are >= 176, else 4; H or W < 88 -> error (the
 * reference asserts). A negative cs mean gives NaN, as numpy does. The workspace is a stream-ordered temporary. */
int dcvc_msssim(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H, int W,
                int row_stride, long long plane_stride, double* out, void* stream);
/* dcvc_msssim for samples in 0..data_range (any DCVC_SAMPLE_* type): C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2 in
 * fp64 (metrics.py calc_msssim's data_range argument). data_range = 255 gives dcvc_msssim's bits; data_range <= 0 -> error. */
int dcvc_msssim_range(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H, int W,
                      int row_stride, long long plane_stride, double data_range, double* out, void* stream);
/* dcvc_msssim_range on a caller-owned workspace of at least dcvc_msssim_workspace_bytes(n_planes, H, W) bytes (device memory,
 * 16-byte aligned, not touched by other work until the call's launches have run on `stream`): nothing is allocated, for a
 * caller that measures picture after picture, as dcvc_sse_ws is to dcvc_sse. The same bits as dcvc_msssim_range (and, at
 * data_range = 255, as dcvc_msssim). dcvc_msssim_workspace_bytes is 0 for what dcvc_msssim refuses. */
long long dcvc_msssim_workspace_bytes(int n_planes, int H, int W);
int dcvc_msssim_range_ws(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H, int W, int row_stride,
                         long long plane_stride, double data_range, double* out, void* workspace, long long workspace_bytes, void* stream);

/* RGB pictures on the device (BT.709: Kr, Kg, Kb = 0.2126, 0.7152, 0.0722; transforms.py:10-14). Every step rounds as the
 * reference's torch op on a GPU does: one fp32 operation each, and a tensor divided by a scalar is a * fp32(1 / b).
 * test_video.py:87-122 get_src_frame (png branch) + transforms.py:17-27 rgb2ycbcr:
 *   src: u8 RGB read at src[h * row_stride + w * pixel_stride + c * channel_stride] (bytes; packed HWC: 3W, 3, 1; planar CHW:
 *   W, 1, H*W) -> x fp16 at pixel stride ldx (3 channels written): x = fp16(fp16(clamp(ycbcr(v / 255), 0, 1)) - 0.5);
 *   planar: u8 [3][H][W] copy of the source (for the metrics). Either output may be NULL, not both. H, W positive and even;
 *   the strides must be positive and must not make two samples overlap. */
int dcvc_rgb_to_x(const void* src, long long row_stride, long long pixel_stride, long long channel_stride, int H, int W,
                  void* x, int ldx, void* planar, void* stream);
/* test_video.py:55-64 get_distortion (png branch) + transforms.py:53-66 ycbcr2rgb, and :366-370 (the PNG writer):
 *   x_hat fp16 [rows][row_pixels][3] -> top-left H x W picture; rgb16: fp16 [3][H][W] = clamp(fp16(clamp(rgb, 0, 1)) * 255,
 *   0, 255), the distortion planes; rgb8: packed u8 [H][W][3] = rint(rgb16) (half to even). NULL = skip. */
int dcvc_x_to_rgb(const void* x_hat, int row_pixels, int H, int W, void* rgb16, void* rgb8, void* stream);
/* dcvc_rgb_to_x / dcvc_x_to_rgb with the colour matrix and the range chosen (no reference counterpart beyond BT.709 / full
 * range). Layouts, NULL rules, the stride rules and stream order are those of the two entry points above. */
#define DCVC_MATRIX_BT601  0   /* Kr, Kg, Kb = 0.299,  0.587,  0.114  */
#define DCVC_MATRIX_BT709  1   /*              0.2126, 0.7152, 0.0722 */
#define DCVC_MATRIX_BT2020 2   /*              0.2627, 0.6780, 0.0593 (non-constant luminance) */
#define DCVC_RANGE_FULL    0
#define DCVC_RANGE_LIMITED 1
/* yuv_bit_depth (8..16) is the depth b of the YUV samples that x stands for: x = v / (2^b - 1) - 0.5, so the limited-range
 * levels (Y 16..235, C 16..240 at 8 bits, times s = 2^(b-8)) sit on x's scale at, with m = 2^b - 1,
 *   lo = 16 s / m, ry = 219 s / m, mid = 128 s / m, rc = 224 s / m, iy = m / (219 s), ic = m / (224 s),
 * each one division in double, then fp32. Full range ignores the depth (it is checked all the same). Every step below is
 * one fp32 operation and every constant the fp32 value of the double expression written:
 *   r, g, b = u8 * (1.0f / 255.0f);  y = (Kr r + Kg g) + Kb b
 *   pb = (0.5 (b - y)) * (1.0f / fp32(1 - Kb));  pr = (0.5 (r - y)) * (1.0f / fp32(1 - Kr))
 *   full: Y = y, Cb = pb + 0.5, Cr = pr + 0.5;  limited: Y = y * ry + lo, Cb = pb * rc + mid, Cr = pr * rc + mid
 *   x_k = fp16(fp32(fp16(clamp(., 0, 1))) - 0.5)
 * At DCVC_MATRIX_BT709 / DCVC_RANGE_FULL this is dcvc_rgb_to_x (the same kernel). Refused before any launch:
 * an unknown matrix or range, a depth outside 8..16, and everything dcvc_rgb_to_x refuses. */
int dcvc_rgb_to_x_cs(const void* src, long long row_stride, long long pixel_stride, long long channel_stride, int H, int W,
                     void* x, int ldx, void* planar, int matrix, int range, int yuv_bit_depth, void* stream);
/* The inverse, with the same constants:
 *   Y, Cb, Cr = fp32(fp16(fp32(x_k) + 0.5))
 *   full: y = Y, pb = Cb - 0.5, pr = Cr - 0.5;  limited: y = (Y - lo) * iy, pb = (Cb - mid) * ic, pr = (Cr - mid) * ic
 *   r = y + fp32(2 - 2 Kr) * pr;  b = y + fp32(2 - 2 Kb) * pb;  g = ((y - Kr r) - Kb b) * (1.0f / fp32(Kg))
 *   rgb16_k = clamp(fp16(fp32(fp16(clamp(., 0, 1))) * 255), 0, 255);  rgb8 = rint(rgb16) (half to even), NaN -> 0
 * At DCVC_MATRIX_BT709 / DCVC_RANGE_FULL this is dcvc_x_to_rgb (the same kernel). Over all 2^24 colours
 * dcvc_x_to_rgb_cs(dcvc_rgb_to_x_cs(c)) = c for every matrix, in full range and in limited range at every depth. */
int dcvc_x_to_rgb_cs(const void* x_hat, int row_pixels, int H, int W, void* rgb16, void* rgb8,
                     int matrix, int range, int yuv_bit_depth, void* stream);
/* 9..16-bit RGB pictures (rgb48: film scans, HDR stills, screen capture; no reference counterpart). Samples are
 * u16, LSB-aligned in 0..max_val = 2^bit_depth - 1; strides are in samples (packed HWC: 3W, 3, 1; planar CHW: W, 1, H*W). The
 * conversion is dcvc_rgb_to_x_cs's from the unit value on, which here is a true division:
 *   r, g, b = fp32(u16) / fp32(max_val), correctly rounded (as dcvc_yuv420p16_to_x; not a reciprocal multiply); samples above
 *   max_val are neither masked nor checked;  y, pb, pr, the levels and x_k as dcvc_rgb_to_x_cs
 *   planar16: u16 [3][H][W] copy of the source (for the metrics). Either output may be NULL, not both.
 * NULL rules, stride rules and stream order are dcvc_rgb_to_x_cs's. Refused before any launch, with the function's name in
 * the message: a bit depth outside 9..16 (8-bit pictures have one definition, dcvc_rgb_to_x_cs's), both outputs NULL, an
 * unknown matrix or range, a yuv_bit_depth outside 8..16, strides that are not positive or overlap, ldx < 3. */
int dcvc_rgb16_to_x_cs(const void* src, long long row_stride, long long pixel_stride, long long channel_stride,
                       int bit_depth, int H, int W, void* x, int ldx, void* planar16,
                       int matrix, int range, int yuv_bit_depth, void* stream);
/* The inverse: dcvc_x_to_rgb_cs up to t_k = fp16(clamp(rgb_k, 0, 1)), then
 *   dist32_k = clamp(fp32(t_k) * fp32(max_val), 0, max_val) (NaN passes through): fp32 [3][H][W], the distortion planes (fp16
 *   cannot hold a 10-bit sample);  rgb16u: packed u16 [H][W][3] = rint(dist32) (half to even), NaN -> 0.
 * Either output may be NULL, not both. Refused as above, and row_pixels < W. x is fp16, so above about 11 bits neighbouring
 * codes share an x: dcvc_x_to_rgb16_cs(dcvc_rgb16_to_x_cs(c)) = c holds for part of the colours only. */
int dcvc_x_to_rgb16_cs(const void* x_hat, int row_pixels, int H, int W, int bit_depth,
                       void* dist32, void* rgb16u, int matrix, int range, int yuv_bit_depth, void* stream);
/* metrics.py:10-24 calc_psnr's fp64 sum of squared differences, one value per plane: n_planes planes of H x W samples (u8,
 * fp16, u16 or fp32; DCVC_SAMPLE_*), src and rec sharing the geometry (row_stride, plane_stride in samples). out: device memory, n_planes
 * doubles, written asynchronously on `stream`. Per-workgroup partials reduced in a fixed order: the same bits on every run and
 * for every n_planes. The workspace is a stream-ordered temporary. */
int dcvc_sse(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H, int W, int row_stride,
             long long plane_stride, double* out, void* stream);
/* dcvc_sse with a workspace of the caller (device memory of at least dcvc_sse_workspace_bytes(n_planes, H, W) bytes, not
 * touched by other work until the call's launches have run on `stream`): nothing is allocated, for a caller that measures
 * picture after picture. The same bits as dcvc_sse. */
long long dcvc_sse_workspace_bytes(int n_planes, int H, int W);
int dcvc_sse_ws(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H, int W, int row_stride,
                long long plane_stride, double* out, void* workspace, long long workspace_bytes, void* stream);

/* The measurement behind scene-cut detection (no reference counterpart). x: the codec's input as
 * dcvc_yuv420_to_x, dcvc_yuv420p16_to_x and dcvc_rgb_to_x write it - fp16, pixel (r, c) at x + (r W + c) ldx halfs, luma in
 * channel 0 - so every source type is served. Per pixel L = clamp(rintf((float(x0) + 0.5f) * 255.f), 0, 255) in fp32, half
 * to even (an 8-bit source's luma sample, exactly).
 *   luma8_out: u8 [H][W] = L. sad_out: one uint64 on the device, 8-byte aligned = sum |L - prev_luma8| over H W pixels, an
 *   exact integer and the same bits on every run; prev_luma8 (u8 [H][W]) NULL: 0. Whatever *sad_out held is overwritten.
 * At most two launches on `stream`, no host synchronisation. Refused before anything is enqueued: NULL x, luma8_out or
 * sad_out; H, W or ldx below 1; a side above 16384; luma8_out == prev_luma8. */
int dcvc_luma_sad(const void* x, int ldx, int H, int W, const void* prev_luma8, void* luma8_out, void* sad_out, void* stream);

/* Picture hashes (no reference counterpart): CRC-32 as zlib's crc32() - reflected polynomial 0xEDB88320, init
 * and final XOR 0xFFFFFFFF - of n byte segments of one device buffer, the planes of a picture in one call.
 *   dcvc_crc32_segments: crc_out[k] (device uint32_t [n], 4-byte aligned) = crc32 of base[offsets[k] .. offsets[k] +
 *   lengths[k]), 0 for a length of 0; crc_out[n..] is not touched. offsets and lengths are host arrays, in bytes, read during
 *   the call; segments may start anywhere, overlap and come in any order. Integer arithmetic: the same value for every launch
 *   geometry and on every run. At most two launches on `stream`, no allocation, no host synchronisation. Refused before
 *   anything is enqueued: NULL base, offsets, lengths or crc_out; n outside 1..16; a negative offset or length; a segment
 *   that ends above 2^44 bytes; crc_out not 4-byte aligned.
 *   dcvc_crc32_combine: host only; crc32(A || B) from crc_a = crc32(A), crc_b = crc32(B) and len_b = the bytes of B. len_b = 0
 *   returns crc_a; a negative len_b returns 0 and sets dcvc_last_error. */
int dcvc_crc32_segments(const void* base, const long long* offsets, const long long* lengths, int n,
                        void* crc_out /* device uint32_t[n] */, void* stream);
uint32_t dcvc_crc32_combine(uint32_t crc_a, uint32_t crc_b, long long len_b);

/* Planes of integer samples at another size (no reference counterpart): a separable Lanczos-3 filter with
 * 12-bit integer coefficients, every output sample defined exactly. One 1-D pass n_in -> n_out, the tables in IEEE double:
 *   scale = n_in / n_out, fs = max(1, scale), support = 3 fs, T = 2 ceil(support) taps for every output of the pass;
 *   output j: centre = (j + 0.5) scale - 0.5, first = floor(centre - support) + 1, w[k] = L((first + k - centre) / fs) with
 *   L(t) = sinc(t) sinc(t / 3) for |t| < 3, else 0; c[k] = rint(w[k] * 4096 / sum w); 4096 - sum c is added to the largest
 *   c[k] (the first one on a tie), so every row sums to 4096 (4097 occurs);
 *   out[j] = clamp((sum_k c[k] in[clamp(first + k, 0, n_in - 1)] + 2048) >> 12, 0, max_val), an arithmetic shift.
 * A plane is filtered horizontally into an intermediate plane of clamped samples, then vertically. n_in == n_out copies.
 * Lengths are 1..16384 and each ratio lies in [1/8, 8] (T <= 48); anything else is refused.
 *   dcvc_resample_ntaps: host only; T, or -1 for what is refused.
 *   dcvc_resample_taps:  host only, no GPU; coef [n_out][T] int16, first [n_out] int32.
 *   dcvc_resample_plan_create: the tables of in_h x in_w -> out_h x out_w onto the current device, once (synchronous);
 *   dcvc_resample_plan_free releases them (NULL is fine).
 *   dcvc_resample_workspace_bytes: the intermediate planes of a call with n_planes planes (either sample type); 0 for bad
 *   arguments.
 *   dcvc_resample_planes: n_planes planes src [in_h][in_w] -> dst [out_h][out_w], every plane on its own. Sample types are
 *   DCVC_SAMPLE_U8 or DCVC_SAMPLE_U16, equal on both sides; strides in samples (plane strides are not read for one plane);
 *   max_val = 255, or 2^bit_depth - 1 for u16. Two launches on `stream`: nothing is allocated and nothing waits for the
 *   host, and the workspace is the caller's until they have run. Refused before anything is enqueued: NULL operands; another
 *   sample type or two different ones; max_val outside 1..255 (u8) / 1..65535 (u16); a row stride below the width or a plane
 *   stride below the plane; n_planes outside 1..65535; a workspace below dcvc_resample_workspace_bytes; dst or the workspace
 *   overlapping src, or the workspace overlapping dst. */
int dcvc_resample_ntaps(int n_in, int n_out);
int dcvc_resample_taps(int n_in, int n_out, int16_t* coef, int32_t* first);
int dcvc_resample_plan_create(int in_h, int in_w, int out_h, int out_w, void** plan);
int dcvc_resample_plan_free(void* plan);
long long dcvc_resample_workspace_bytes(const void* plan, int n_planes);
int dcvc_resample_planes(const void* plan, const void* src, int src_dtype, int src_row_stride, long long src_plane_stride, void* dst,
                         int dst_dtype, int dst_row_stride, long long dst_plane_stride, int n_planes, int max_val, void* workspace,
                         long long workspace_bytes, void* stream);

/* Denoising prefilter on the GPU (no reference counterpart): planes of integer samples through an
 * edge-preserving 3x3 spatial stage and a motion-adaptive recursive temporal stage, every output sample defined exactly in
 * signed 32-bit integers. Per plane, sh = bit_depth - 8, Ts = spatial << sh, Tt = temporal << sh, indexes clamped to the plane:
 *   spatial:  c the centre, n_i the 9 samples of its 3x3 neighbourhood, w_i = max(0, Ts - |n_i - c|), num = sum w_i (n_i - c),
 *             ws = sum w_i, sp = c + floor((2 num + ws) / (2 ws)), a true floor; spatial == 0: sp = c.
 *   temporal: prev is the same plane of the previous output picture. prev == NULL or temporal == 0: out = sp. Otherwise
 *             m = sum over the 3x3 neighbourhood q of |sp[q] - prev[q]| (sp at a clamped index is the sp of the clamped
 *             position), L = 9 Tt, k = (192 max(0, L - m)) / L, out = sp + ((k (prev - sp) + 128) >> 8), an arithmetic shift.
 * Every output lies between the smallest and the largest sample it read; spatial == temporal == 0 copies.
 *   dcvc_denoise_planes: n_planes planes src [H][W] (and prev) -> dst, every plane on its own; samples are DCVC_SAMPLE_U8
 *   (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned, bit_depth 9..16); strides in samples (plane strides are not read for one
 *   plane, prev's strides not without prev). One launch on `stream`: nothing is allocated and nothing waits for the host.
 *   Refused before anything is enqueued: NULL src or dst; another sample type; a bit_depth that is not the type's; H or W
 *   outside 1..16384; n_planes outside 1..65535; a strength outside 0..64; a row stride below W or a plane stride below the
 *   plane; a 16-bit plane at an odd address; dst overlapping src or prev. */
int dcvc_denoise_planes(const void* src, int src_row_stride, long long src_plane_stride, const void* prev, int prev_row_stride,
                        long long prev_plane_stride, void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int bit_depth,
                        int H, int W, int n_planes, int spatial, int temporal, void* stream);

/* Block motion search and motion compensation on the GPU (no reference counterpart), every value defined exactly
 * in signed 32-bit integers. cur and ref are luma planes [H][W]; sh = bit_depth - 8, L = lambda << sh; blocks are 16 x 16 luma
 * samples, Bh = ceil(H / 16), Bw = ceil(W / 16):
 *   half resolution: H1 = ceil(H / 2), W1 = ceil(W / 2),
 *                    a1[y][x] = (a[2y][2x] + a[2y][2x+1] + a[2y+1][2x] + a[2y+1][2x+1] + 2) >> 2, indexes clamped to the plane.
 *   block SAD:       over the block's samples inside cur (a partial block at the right or bottom edge sums fewer samples); the
 *                    reference index (y + dy, x + dx) is clamped to the plane.
 *   order:           the smallest tuple (cost, |dx| + |dy|, dy, dx) wins.
 *   level 1:         block (by, bx) is the 8 x 8 block of the half-resolution planes; every dx, dy in -range..range is a
 *                    candidate, cost = SAD + L (|dx| + |dy|); the winner is (dx1, dy1).
 *   level 0:         full resolution, the 16 x 16 block; the candidates are (2 dx1 + ex, 2 dy1 + ey), ex, ey in -1..1, and
 *                    (0, 0); cost = SAD + 4 L (|dx| + |dy|). The winner is the block's vector, |dx|, |dy| <= 2 range + 1.
 *   dcvc_motion_search_workspace_bytes: the two half-resolution planes of a search on [H][W]; 0 for bad arguments.
 *   dcvc_motion_search: mv (device, int16 [mv_bh][mv_bw][2]) takes (dx, dy) of blocks [0, Bh) x [0, Bw), the rest of the grid
 *   is left alone; sad (device, uint32 [mv_bh][mv_bw], or NULL) the winner's SAD without the penalty; moved (device, one
 *   uint32, or NULL) is increased by the number of blocks whose vector is not (0, 0), the caller zeroes it. Samples are
 *   DCVC_SAMPLE_U8 (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned, bit_depth 9..16); strides in samples; cur == ref is
 *   allowed. Two launches on `stream`: nothing is allocated and nothing waits for the host, and the workspace is the caller's
 *   until they have run. Refused before anything is enqueued: NULL cur, ref, mv or workspace; another sample type; a bit_depth
 *   that is not the type's; H or W outside 1..16384; range outside 0..15; lambda outside 0..255; an mv grid below Bh x Bw; a
 *   row stride below W; a 16-bit plane, mv or the workspace at an odd address; a sad or moved that is not 4-byte aligned; a workspace
 *   below dcvc_motion_search_workspace_bytes.
 *   dcvc_motion_compensate_planes: n_planes planes prev [H][W] -> dst, every plane on its own, the planes subsampled by
 *   (sx, sy) in {0, 1} against the luma plane the vectors were searched on: the block of sample (y, x) is
 *   (y / (16 >> sy), x / (16 >> sx)), dxc = dx >> sx, dyc = dy >> sy (arithmetic shifts: a floor),
 *   dst[y][x] = prev[clamp(y + dyc)][clamp(x + dxc)]. The vectors are device data and are not validated: the clamp makes any
 *   int16 vector safe; all-zero vectors copy. One launch on `stream`; plane strides are not read for one plane. Refused before
 *   anything is enqueued: NULL prev, dst or mv; another sample type; H or W outside 1..16384; sx or sy outside {0, 1}; n_planes
 *   outside 1..65535; an mv grid below ceil(H / (16 >> sy)) x ceil(W / (16 >> sx)); a row stride below W or a plane stride
 *   below the plane; a 16-bit plane or mv at an odd address; dst overlapping prev or mv. */
long long dcvc_motion_search_workspace_bytes(int H, int W);
int dcvc_motion_search(const void* cur, int cur_row_stride, const void* ref, int ref_row_stride, int dtype, int bit_depth, int H, int W,
                       int range, int lambda, void* mv, int mv_bh, int mv_bw, void* sad, void* moved, void* workspace,
                       long long workspace_bytes, void* stream);
int dcvc_motion_compensate_planes(const void* prev, int prev_row_stride, long long prev_plane_stride, void* dst, int dst_row_stride,
                                  long long dst_plane_stride, int dtype, int H, int W, int n_planes, int sx, int sy, const void* mv,
                                  int mv_bh, int mv_bw, void* stream);

/* Frame-rate conversion on the GPU (no reference counterpart): the picture at k / n of the way from picture a to
 * picture b, every value defined exactly in signed 32-bit integers. n in 2..8, k in 1..n-1, sh = bit_depth - 8; blocks are
 * 16 x 16 luma samples, Bh = ceil(H / 16), Bw = ceil(W / 16); all indexes into a plane are clamped to it; all divisions are floor
 * divisions of signed integers.
 *   vectors:       mv (device, int16 [mv_bh][mv_bw][2]) is the grid of dcvc_motion_search(cur = b, ref = a), b[p] ~ a[p + v]. It
 *                  is device data and is not validated: each component is clamped to -31..31 when read.
 *   split:         per component va = (2 k v + n) / (2 n) (k v / n rounded, halves up), vb = va - v: the in-between sample at p
 *                  is seen at a[p + va] and at b[p + vb].
 *   selection:     the candidates of block (y, x) are the clamped vectors of the 3 x 3 neighbourhood of mv[y][x], grid indexes
 *                  clamped to [0, Bh) x [0, Bw), and (0, 0). SAD(v) = sum of |a[p + va] - b[p + vb]| over the block's samples
 *                  inside the plane, no penalty; the smallest tuple (SAD, |vx| + |vy|, vy, vx) wins. The block falls back when
 *                  SAD > (limit << sh) * s, s the number of samples summed.
 *   dcvc_interp_select: a, b luma planes [H][W]. plan (device, int16 [plan_bh][plan_bw][4]) takes (vax, vay, vbx, vby) and wb
 *   (device, uint8 [plan_bh][plan_bw]) b's weight k of blocks [0, Bh) x [0, Bw); a block that fell back takes offsets 0 and
 *   wb = 0 when 2 k <= n, else wb = n: it repeats the nearer picture. The rest of the grids is left alone. sad (device, uint32
 *   [plan_bh][plan_bw], or NULL) takes the winner's SAD; fallen (device, one uint32, or NULL) is increased by the number of
 *   blocks that fell back, the caller zeroes it. Samples are DCVC_SAMPLE_U8 (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned,
 *   bit_depth 9..16); strides in samples. One launch on `stream`: nothing is allocated and nothing waits for the host. Refused
 *   before anything is enqueued: NULL a, b, mv, plan or wb; another sample type; a bit_depth that is not the type's; H or W
 *   outside 1..16384; n outside 2..8; k outside 1..n-1; limit outside 0..255; an mv or plan grid below Bh x Bw; a row stride
 *   below W; a 16-bit plane, mv or plan at an odd address; a sad or fallen that is not 4-byte aligned.
 *   dcvc_interp_planes: n_planes planes a, b [H][W] -> dst, every plane on its own, the planes subsampled by (sx, sy) in {0, 1}
 *   against the luma plane of the selection: the block of sample (y, x) is (y / (16 >> sy), x / (16 >> sx)), the offsets are
 *   vax >> sx, vay >> sy, vbx >> sx, vby >> sy (arithmetic shifts), w = min(wb, n),
 *   dst[y][x] = ((n - w) a[y + vay][x + vax] + w b[y + vby][x + vbx] + (n >> 1)) / n. plan and wb are device data and are not
 *   validated: the clamps make any value safe. With fallen (device, one uint32) and 2 * fallen > n_blocks every block is
 *   treated as fallen: the whole picture repeats a (2 k <= n) or b; the counter is read on the device. With fallen == NULL only
 *   the plan decides. One launch on `stream`; plane strides are not read for one plane. Refused before anything is enqueued:
 *   NULL a, b, dst, plan or wb; another sample type; H or W outside 1..16384; n outside 2..8; k outside 1..n-1; sx or sy outside
 *   {0, 1}; n_planes outside 1..65535; a plan grid below ceil(H / (16 >> sy)) x ceil(W / (16 >> sx)); n_blocks below 1 with
 *   fallen; a row stride below W or a plane stride below the plane; a 16-bit plane or plan at an odd address; a fallen that is
 *   not 4-byte aligned; dst overlapping a, b, plan or wb. */
int dcvc_interp_select(const void* a, int a_row_stride, const void* b, int b_row_stride, int dtype, int bit_depth, int H, int W,
                       const void* mv, int mv_bh, int mv_bw, int k, int n, int limit, void* plan, void* wb, int plan_bh, int plan_bw,
                       void* sad, void* fallen, void* stream);
int dcvc_interp_planes(const void* a, int a_row_stride, long long a_plane_stride, const void* b, int b_row_stride, long long b_plane_stride,
                       void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int H, int W, int n_planes, int sx, int sy,
                       const void* plan, const void* wb, int plan_bh, int plan_bw, int k, int n, const void* fallen, int n_blocks,
                       void* stream);

/* Deinterlacer on the GPU (no reference counterpart): planes of a woven frame -> progressive planes, every
 * output sample defined exactly in signed 32-bit integers. Per plane, T = threshold << (bit_depth - 8):
 *   rows y with y % 2 == keep are copied from cur. For a missing row y: ya = y - 1 (y + 1 at the top), yb = y + 1 (y - 1 at
 *   the bottom), A = cur[ya], B = cur[yb], column indexes clamped to the plane.
 *   spatial:  for d in the order 0, -1, +1: score_d = sum over j in -1..1 of |A[x + j + d] - B[x + j - d]|,
 *             pred_d = (A[x + d] + B[x - d] + 1) >> 1; the smallest score wins, a later direction only when strictly smaller.
 *   prev == NULL or threshold == 0: out = sp. Otherwise prev is the previous INPUT frame,
 *             m = max over rows {ya, y, yb} and columns x - 1 .. x + 1 of |cur - prev|, k = (256 max(0, T - m)) / T,
 *             wv = weave_from_prev ? prev[y][x] : cur[y][x], out = sp + ((k (wv - sp) + 128) >> 8), an arithmetic shift.
 * Where nothing moved out = wv exactly; every output lies between samples it read.
 *   dcvc_deinterlace_planes: n_planes planes cur [H][W] (and prev) -> dst, every plane on its own; samples are DCVC_SAMPLE_U8
 *   (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned, bit_depth 9..16); strides in samples (plane strides are not read for one
 *   plane, prev's strides not without prev). One launch on `stream`: nothing is allocated and nothing waits for the host.
 *   Refused before anything is enqueued: NULL cur or dst; another sample type; a bit_depth that is not the type's; H outside
 *   2..16384 or W outside 1..16384; n_planes outside 1..65535; keep or weave_from_prev outside {0, 1}; a threshold outside
 *   0..64; a row stride below W or a plane stride below the plane; a 16-bit plane at an odd address; dst overlapping cur or
 *   prev. */
int dcvc_deinterlace_planes(const void* cur, int cur_row_stride, long long cur_plane_stride, const void* prev, int prev_row_stride,
                            long long prev_plane_stride, void* dst, int dst_row_stride, long long dst_plane_stride, int dtype,
                            int bit_depth, int H, int W, int n_planes, int keep, int weave_from_prev, int threshold, void* stream);

/* Inverse telecine on the GPU (no reference counterpart): the measurement and the weave; the decisions are
 * dcvc_ivtc_* (dcvc_amd_rc.h). first = the parity (0, 1) of the rows of the field shown first (0 for tff, 1 for bff),
 * q = 1 - first, t = cthresh << (bit_depth - 8). cur and prev are the luma planes of source frames f and f - 1. For a candidate
 * second field S in {cur (match c), prev (match p)}, over the rows y with y % 2 == q and 1 <= y <= H - 2 and every x, with
 * a = cur[y-1][x], b = cur[y+1][x], s = S[y][x]:
 *   match_S  = sum |2 s - a - b|
 *   comb_S   = the number of samples with (s - a > t and s - b > t) or (s - a < -t and s - b < -t)
 *   blkmax_S = the largest count of such samples in a block (y / 16, x / 32); blocks are aligned to the plane's origin, edge
 *              blocks count what they hold
 *   dup      = sum |cur[y][x] - prev[y][x]| over ALL rows with y % 2 == first
 *   dcvc_field_match: out8 (device, eight uint64) = [match_c, match_p, comb_c, comb_p, blkmax_c, blkmax_p, dup, 0]; with
 *   prev == NULL words 1, 3, 5 and 6 are 0 (prev's stride is not read). H == 2 has no interior row: the match words are 0.
 *   Exact integers, the same for every launch geometry and every run. Two launches on `stream`: nothing is allocated and
 *   nothing waits for the host. Samples are DCVC_SAMPLE_U8 (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned, bit_depth 9..16);
 *   strides in samples. Refused before anything is enqueued: NULL cur or out8; another sample type; a bit_depth that is not
 *   the type's; H outside 2..16384 or W outside 1..16384; first outside {0, 1}; cthresh outside 0..255; a row stride below W;
 *   a 16-bit plane at an odd address; an out8 that is not 8-byte aligned.
 *   dcvc_weave_fields: n_planes planes [H][W]: dst rows of parity `first` are a's, the others b's, every plane on its own (a
 *   and b may be the same planes: a copy). One launch; plane strides are not read for one plane. Refused before anything is
 *   enqueued: NULL a, b or dst; another sample type; H outside 2..16384 or W outside 1..16384; n_planes outside 1..65535; first
 *   outside {0, 1}; a row stride below W or a plane stride below the plane; a 16-bit plane at an odd address; dst overlapping
 *   a or b. */
int dcvc_field_match(const void* cur, int cur_row_stride, const void* prev, int prev_row_stride, int dtype, int bit_depth, int H, int W,
                     int first, int cthresh, void* out8, void* stream);
int dcvc_weave_fields(const void* a, int a_row_stride, long long a_plane_stride, const void* b, int b_row_stride, long long b_plane_stride,
                      void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int H, int W, int n_planes, int first, void* stream);

/* Film grain on the GPU (no reference counterpart): synthesis onto decoded planes and the measurement of what
 * dcvc_denoise_planes removed; the template and the fit are host code, dcvc_grain_template / dcvc_grain_fit (dcvc_amd_rc.h).
 * Every value is an exact integer. sh = bit_depth - 8, max_val = 2^bit_depth - 1, u32 arithmetic wraps, shifts of signed values
 * are arithmetic. The planes of a call have one size [H][W] and share one luma plane Yl [Hl][Wl] against which they are
 * subsampled by (sx, sy) in {0, 1}; Hl >= ((H-1) << sy) + 1 and Wl >= ((W-1) << sx) + 1, indexes clamped into the luma plane:
 *   sx == 1: L = (Yl[y << sy][2x] + Yl[y << sy][2x + 1] + 1) >> 1;   sx == 0: L = Yl[y << sy][x];   i = min(L >> sh, 255)
 *   dcvc_grain_apply: plane p = first_plane + 0 .. n_planes - 1 (0, 1, 2 = Y, U, V) of output picture `pic`, block (by, bx) =
 *   (y / 32, x / 32) in the plane's own coordinates:
 *     h = seed*0x9E3779B1 + pic*0x85EBCA77 + p*0xC2B2AE3D + by*0x27D4EB2F + bx*0x165667B1; h ^= h >> 15; h *= 0x2C1B3C6D;
 *     h ^= h >> 12; h *= 0x297A2D39; h ^= h >> 15; ox = h & 63; oy = (h >> 8) & 63
 *     t = template_p[(oy + (y & 31)) & 63][(ox + (x & 31)) & 63]   (device, int16 [64][64], |t| <= 1023: dcvc_grain_template)
 *     k = i >> 5, fr = i & 31, v = (lut[p][k] (32 - fr) + lut[p][k+1] fr + 16) >> 5   (lut: host, uint8 [3][9], sixteenths of an
 *     8-bit code value at luma 0, 32, .., 256), n = (t v + (1 << (9 - sh))) >> (10 - sh), dst = clamp(rec + n, 0, max_val)
 *   A table of zeros copies. The luma is the UNGRAINED reconstruction. dst may be rec (the same pointer and strides); dst may
 *   overlap the luma plane only in a call of one plane that is rec and the luma at once (sx = sy = 0). Templates of planes
 *   outside the call are not read and may be NULL. One launch on `stream`.
 *   dcvc_grain_stats: src, and den = the denoiser's output for it, n_planes (1..2) planes; luma is DEN's luma plane.
 *   d = src - den; a sample counts when den's four 4-neighbours in its own plane (indexes clamped) each differ from den[y][x] by
 *   at most flat << sh; its bin is i >> 5. words (device, 8-byte aligned, 16 uint64 a plane): n[0..7] the counts, S[0..7] the
 *   sums of d^2. accumulate == 0: a first launch zeroes the words; 1: the call adds to them (less than 2^60 a call). Exact
 *   integers, the same for every launch geometry and every run.
 *   Both: samples are DCVC_SAMPLE_U8 (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned, bit_depth 9..16); strides in samples (plane
 *   strides are not read for one plane); nothing is allocated and nothing waits for the host. Refused before anything is
 *   enqueued: a NULL operand; another sample type; a bit_depth that is not the type's; H or W outside 1..16384; n_planes
 *   outside 1..3 (apply, and first_plane + n_planes above 3) or 1..2 (stats); sx or sy outside {0, 1}; a luma plane that is too
 *   small (or above 32768 a side); flat outside 0..255; accumulate outside {0, 1}; a row stride below the width or a plane stride
 *   below the plane; a 16-bit plane or a template at an odd address; words that are not 8-byte aligned; dst overlapping rec
 *   (unless it is rec), the luma (but for the case above) or a template. */
int dcvc_grain_apply(const void* rec, int rec_row_stride, long long rec_plane_stride, const void* luma, int luma_row_stride, int Hl, int Wl,
                     void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int bit_depth, int H, int W, int n_planes,
                     int first_plane, int sx, int sy, const int16_t* template_y, const int16_t* template_u, const int16_t* template_v,
                     const uint8_t* lut, uint32_t seed, uint32_t pic, void* stream);
int dcvc_grain_stats(const void* src, int src_row_stride, long long src_plane_stride, const void* den, int den_row_stride,
                     long long den_plane_stride, const void* luma, int luma_row_stride, int Hl, int Wl, int dtype, int bit_depth, int H,
                     int W, int n_planes, int sx, int sy, int flat, int accumulate, void* words, void* stream);

/* Black-bar cropping on the GPU (no reference counterpart): the measurement and the window copy; the decision
 * is dcvc_cropdet_* (dcvc_amd_rc.h). Every value is an exact integer.
 *   dcvc_crop_stats: t = limit << (bit_depth - 8); for the luma plane Y [H][W], rowcnt[r] = the number of x with Y[r][x] > t and
 *   colcnt[c] = the number of y with Y[y][c] > t. counts (device, uint32 [H + W], 4-byte aligned) = rowcnt, then colcnt; what it
 *   held is overwritten. The same words for every launch geometry and every run. Two launches on `stream`: nothing is allocated
 *   and nothing waits for the host. Samples are DCVC_SAMPLE_U8 (bit_depth 8) or DCVC_SAMPLE_U16 (LSB-aligned, bit_depth 9..16);
 *   strides in samples. Refused before anything is enqueued: NULL luma or counts; another sample type; a bit_depth that is not
 *   the type's; H or W outside 1..16384; limit outside 0..255; a row stride below W; a 16-bit plane at an odd address; counts
 *   that are not 4-byte aligned.
 *   dcvc_window_planes: n_planes planes, src [Hs][Ws] and dst [Hd][Wd]: dst[p][y][x] = src[p][y + oy][x + ox] where
 *   0 <= y + oy < Hs and 0 <= x + ox < Ws, else fill[p] (host, [n_planes], read during the call). ox, oy are signed: a crop is
 *   ox, oy >= 0 with the window inside the source, a pad ox, oy <= 0 with the source inside the window, any mixture is defined
 *   by the same line. Nothing is written past Wd in a row. One launch for every 16 planes; plane strides are not read for one
 *   plane. Refused before anything is enqueued: NULL src, dst or fill; another sample type; Hs, Ws, Hd or Wd outside 1..16384;
 *   n_planes outside 1..65535; |ox| or |oy| above 16384; a fill value outside the type (0..255, 0..65535); a row stride below
 *   the width or a plane stride below the plane; a 16-bit plane at an odd address; dst overlapping src. */
int dcvc_crop_stats(const void* luma, int row_stride, int dtype, int bit_depth, int H, int W, int limit, void* counts, void* stream);
int dcvc_window_planes(const void* src, int src_row_stride, long long src_plane_stride, int Hs, int Ws, void* dst, int dst_row_stride,
                       long long dst_plane_stride, int Hd, int Wd, int dtype, int n_planes, int ox, int oy, const int* fill, void* stream);

/* Tuning aid (no reference counterpart): device buffer of [blocks][16] int64 shader-clock stamps
 * written by wave 0 of every workgroup of the following contraction launches; NULL = off. */
int dcvc_gemm_timeline_buffer(void* device_buffer);
int dcvc_dcb_nsplit_timeline_buffer(void* device_buffer);   /* [workgroups][32] stamps of the N-split block kernel */
/* tuning aid (tools/probes/core_bench.hip -w): while set, dcvc_dcb_nsplit* launches of a shape that has the variant run with their
 * depthwise conv inside on these operands (t1 [pixels][ci] instead of the call's t2, taps [9][ci], picture width); t1 = NULL: off */
int dcvc_dcb_nsplit_dw_hook(const void* t1, const void* wdw, int width);

/* def_elementwise.h: round_z_cuda / int8_to_dtype_cuda */
int dcvc_round_z(const void* z, void* z_hat, void* z_i8, int count, void* stream);
int dcvc_int8_to_half(const void* in, void* out, int count, void* stream);

/* One autoregressive step of the 4x masked y coding, encoder side. Fuses
 * process_with_mask_cuda + single_part_for_writing_4x_cuda (x2) + build_index_enc_cuda +
 * conditional_index_part1_cuda (def_elementwise.h). Outputs: y_hat_acc (active group written;
 * step 0 also zeroes the other groups), sym[P*C/4] int16, cond bits, per-block counts, then the
 * compacted symbols out[...] and totals[step]. n_blocks = dcvc_symbol_blocks(P*C/4). */
int dcvc_symbol_blocks(int count);
int dcvc_y_step_enc(const void* y, int ldy, const void* scales, int lds, const void* means, int ldm,
                    void* y_hat_acc, int ldacc, void* sym, void* cond, void* block_count,
                    void* compact_out, void* totals,
                    int H, int W, int C, int step, float skip_thres, void* stream);
/* decoder side, part 1: single_part_for_reading_4x_cuda + build_index_dec_cuda + compaction */
int dcvc_y_step_dec_index(const void* scales, int lds, void* index, void* cond, void* block_count,
                          void* compact_out, void* totals,
                          int H, int W, int C, int step, float skip_thres, void* stream);
/* decoder side, part 2: conditional_recover_with_type_conversion_cuda + restore_y_4x*_cuda.
 * decoded: int8 symbols of ALL steps so far, this step's start at sum(totals[0..step)). */
int dcvc_y_step_dec_restore(const void* decoded, const void* cond, const void* block_count,
                            const void* totals, const void* means, int ldm,
                            void* y_hat_acc, int ldacc, int H, int W, int C, int step, void* stream);
/* Batched forms of the three (not part of the reference surface): n (1..16) pictures of H x W back to back in
 * every operand - y / scales / means / y_hat_acc [n][P][ld], sym and index [n][P*C/4], cond [n][P*C/32], block_count
 * [n][dcvc_symbol_blocks(P*C/4)] - the masks following each picture's own (row, column). Picture b compacts into
 * compact_out + b * out_stride (elements) with its counts in totals + b * totals_stride (int32s): this step's count goes to
 * totals[slot] and its output starts sum(totals[0..slot)) elements into the picture's region. The restore reads picture b's
 * symbols from decoded + b * decoded_stride in the same way. The single forms above are n = 1, slot = step. C must be a
 * multiple of 32; the argument checks are those of the layout group. */
int dcvc_y_step_enc_b(const void* y, int ldy, const void* scales, int lds, const void* means, int ldm, void* y_hat_acc, int ldacc,
                      void* sym, void* cond, void* block_count, void* compact_out, long long out_stride, void* totals,
                      int totals_stride, int slot, int H, int W, int C, int step, float skip_thres, int n, void* stream);
int dcvc_y_step_dec_index_b(const void* scales, int lds, void* index, void* cond, void* block_count, void* compact_out,
                            long long out_stride, void* totals, int totals_stride, int slot, int H, int W, int C, int step,
                            float skip_thres, int n, void* stream);
int dcvc_y_step_dec_restore_b(const void* decoded, long long decoded_stride, const void* cond, const void* block_count,
                              const void* totals, int totals_stride, int slot, const void* means, int ldm, void* y_hat_acc,
                              int ldacc, int H, int W, int C, int step, int n, void* stream);

/* The inter models' full-tensor masked steps (nsteps = 2: LD checkerboard x channel halves,
 * dmc_ld_proxy.cpp:672-683; nsteps = 4: HT-S channel-group x 2x2-position masks,
 * dmc_hts_proxy.cpp:869-890). One call = one step of
 *   divide_with_clamp_min_inplace_cuda (step 0) + process_with_mask_no_scale[_add[_and_multiply]]_inplace_cuda
 *   (+ build_index_enc_cuda + conditional_index_part1_cuda on the last step, compacted symbols -> compact_out,
 *   count -> totals[0]).
 * y is rescaled in place at step 0; y_hat accumulates over the steps and is final after the last. */
int dcvc_mask_step_enc(void* y, int ldy, const void* q_dec, int ldq, const void* scales, int lds,
                       const void* means, int ldm, void* y_hat, int ldh, void* sym, void* cond,
                       void* block_count, void* compact_out, void* totals, int H, int W, int C,
                       int nsteps, int step, float skip_thres, void* stream);
/* build_index_dec_cuda + conditional_index_part1_cuda over all channels */
int dcvc_mask_dec_index(const void* scales, int lds, void* index, void* cond, void* block_count,
                        void* compact_out, void* totals, int H, int W, int C, float skip_thres, void* stream);
/* conditional_recover_with_type_conversion_cuda (step 0) + restore_y[_and_add[_multiply]]_inplace_cuda;
 * yq: int8 scratch [H*W*C] carried from step 0 to the later steps */
int dcvc_mask_step_dec(const void* decoded, const void* cond, const void* block_count, const void* totals,
                       void* yq, const void* means, int ldm, const void* q_dec, int ldq, void* y_hat, int ldh,
                       int H, int W, int C, int nsteps, int step, void* stream);

/* Measurement hook (bench.py roofline leg, not a reference entry point): bracket every
 * contraction launch with HIP events on its stream; collect = summed kernel milliseconds,
 * algorithmic FLOPs (2*M*N*K) and launch count since the last reset. Graph replay must be off. */
int dcvc_gemm_profile_enable(int on);
int dcvc_gemm_profile_reset(void);
int dcvc_gemm_profile_collect(double* ms, double* flops, long long* launches);
/* per-launch records {int M, N, K, variant; float ms}; returns the number of launches recorded */
long long dcvc_gemm_profile_launches(void* records, long long cap);

/* Code length (no reference counterpart): what the host rANS coder will spend on symbols, from tables, in units of
 * 2^-16 bit. A value coded with frequency f out of 2^16 costs rint(65536 * (16 - log2(f))) (double arithmetic); an
 * escaped one (value >= cdf_len - 2) costs the escape value's frequency plus 2 bits for each of its bypass groups
 * (raw groups + 1 count group + raw groups / 3 continuation groups), exactly as the coder emits them.
 *   dcvc_code_length_cost: one entry from a frequency (1 .. 65536) and a bypass group count; 0xFFFFFFFF = not codable.
 *   dcvc_code_length_table (host memory, no GPU): the table of a CDF family as given to dcvc_rans_*_set_cdf
 *     (cdfs [num_cdf][stride], cdf_sizes [num_cdf]) -> out [num_cdf][cols]; cols = 256: column uint8(symbol), symbol an
 *     int8 (the y family); cols = 128: column symbol + 64, symbol in [-64, 63] (the z family).
 *   dcvc_predicted_stream_bytes: ideal length -> bytes of the stream of ec_parallel (1 .. 8) sub-streams: 32 bits of
 *     final coder state per sub-stream and the 32-bit offsets in front of 3 or more sub-streams are added, then
 *     rounded up to bytes. */
uint32_t dcvc_code_length_cost(int freq, int bypass_groups);
int dcvc_code_length_table(const int32_t* cdfs, int num_cdf, int stride, const int32_t* cdf_sizes, int cols, uint32_t* out);
long long dcvc_predicted_stream_bytes(long long y_units, long long z_units, int ec_parallel);
/* The sums on the device, n pictures per call (picture = blockIdx.y). Integer sums: exact, the same on every run.
 *   y: sym int16 (q << 8) + cdf index as dcvc_y_step_enc writes them, 16-byte aligned, picture b at sym + b * sym_stride
 *     (elements, a multiple of 8). cond: keep bits of the uncompacted layout (bit e % 8 of byte e / 8; picture b at
 *     cond + b * cond_stride bytes) or NULL = every symbol counts (compacted layout). totals: device int32 counts, picture
 *     b's symbol count = sum of totals[b * totals_stride + 0 .. n_totals) capped at `count`, or NULL = `count` symbols.
 *     table: device uint32 [num_cdf][256]. out: device uint64 [n][2] = {units, symbols counted}, zeroed by the call.
 *   z: int8 [n][count] in [-64, 63], symbol i coded with row i % ch of table (device uint32 [ch][128], the rows of the
 *     selected q_index). out: device uint64 [n] units, zeroed by the call. */
int dcvc_code_length_y(const void* sym, long long sym_stride, const void* cond, long long cond_stride, const void* totals,
                       int totals_stride, int n_totals, int count, const void* table, int num_cdf, void* out, int n,
                       void* stream);
int dcvc_code_length_z(const void* z, int count, int ch, const void* table, void* out, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCVC_AMD_OPS_H */
