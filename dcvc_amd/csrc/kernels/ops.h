// Host-side launch interface of the HIP kernels (raw device pointers + explicit leading
// dimensions, everything on the caller's stream; nothing here allocates or synchronises, so all
// of it can be captured into a hipGraph).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace dcvc {

typedef _Float16 half_t;

inline void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    }
}

// One-time device-side tables (WSiLU coefficients, scale->index LUT). Call once per process
// before the first launch and outside any graph capture.
void kernels_init();

// ---------------------------------------------------------------- per-kernel timing (conv_gemm.hip)
// When enabled, every contraction launch is bracketed by a pair of HIP events on its own stream
// (launches must then be eager, not captured). collect() synchronises the events and returns
// the summed kernel time, the algorithmic FLOPs (2*M*N*K) and the launch count since reset().
void gemm_profile_enable(bool on);
void gemm_profile_reset();
void gemm_profile_collect(double* ms, double* flops, long long* launches);
struct GemmLaunchInfo {
    int M, N, K, variant;   // variant bits: 1 spatial, 2 wsilu, 4 chunk-add, 8/16 residuals, 32 quant, 64 upsample
    float ms;
};
size_t gemm_profile_launches(GemmLaunchInfo* out, size_t cap);
// Other contraction kernels (dcb_nsplit.hip, dcb_tail.hip, ffn_fused.hip) register their launches in the same list: when profiling
// is on, reserves a record and hands out the two events hipExtLaunchKernelGGL stamps; false = off.
// info.K is chosen such that 2 * M * N * K is the launch's FLOP count; variant bits 28..31 name the kernel
// family: 0 conv_gemm, 2 dcb_tail, 3 ffn_fused, 4 dcb_nsplit, 5 dcb_nsplit8 (its variant also carries the inner width in bits
// 0..11 and the NEXT slot - 0, 1 = next dc.0, NN = closing conv - in bits 12..23), 6 dcb_pair8 (8 was round 2's dcb_core).
// Bits 0..27 name the instantiation that ran; every field keeps the place it has in any family that carries it:
//   bits 0..11   inner width (dcb_nsplit8, dcb_pair8) or block width C (dcb_tail, ffn_fused)
//   bits 12..23  dcb_nsplit8: the NEXT slot as above; dcb_pair8: the adaptor's input width CIN
//   bit 24       the depthwise conv runs inside (dcb_nsplit8, dcb_tail)
//   bit 25       64-pixel workgroups (dcb_nsplit8, dcb_pair8; 0 = 32 pixels)
//   bit 26       fused quant scale q (dcb_tail, ffn_fused)
//   bit 27       dcb_tail: dc.0 inside the launch; ffn_fused: second residual r2
bool gemm_profile_slot(const GemmLaunchInfo& info, hipEvent_t* start, hipEvent_t* stop);
// Tuning aid: when non-null, wave 0 of every workgroup of the following contraction launches
// writes up to 16 shader-clock stamps (kernel entry, prologue issued, start of k-steps 0..7, main
// loop done, epilogue math done, stores issued) to buffer[block * 16 + i]. Null switches it off.
void gemm_timeline_buffer(long long* device_buffer);

// ---------------------------------------------------------------- dense convolutions (conv_gemm.hip)
struct Conv1x1Desc {
    const half_t* x = nullptr; int ldx = 0;     // [pixels][ldx], first `cin` channels of each pixel
    const half_t* w = nullptr;                  // [cout][cin]
    const half_t* bias = nullptr;               // [cout] or null
    const half_t* r1 = nullptr; int ldr1 = 0;   // residuals (added in fp32 before the rounding)
    const half_t* r2 = nullptr; int ldr2 = 0;
    const half_t* q = nullptr;                  // fused per-channel scale (…_with_quant)
    const half_t* q2 = nullptr;                 // per-channel scale applied to the rounded fp16 output
    half_t* y = nullptr; int ldy = 0;           // [pixels][ldy]; cout (or cout/4 with chunk_add) channels
    int pixels = 0, cin = 0, cout = 0;
    bool wsilu = false, chunk_add = false;
};
void conv1x1(const Conv1x1Desc& d, hipStream_t stream);

// DepthConvBlock behind its depthwise conv in one launch, "N-split" form (dcb_nsplit.hip, round 3; round 2's register-resident
// dcb_core kernel is in the history only):
//   y1 = W3 t2 + b3 + x ; t = chunk_add(WSiLU(W0 y1 + b0)) ; y = (W2 t + b2 + y1 [+ x]) [* q] -> fp16 [* q2]
//   and optionally the next block's dc.0: t1n = WSiLU(W1n y + b1n).
// Bit-identical to conv1x1(dc.3) + conv1x1(ffn.0, wsilu, chunk_add) + conv1x1(ffn.2) [+ conv1x1(dc.0, wsilu)].
// Activations in LDS, every wave owns a quarter of
// the output channels and streams ITS weight fragments straight from L2 out of a pre-packed per-wave stream
// (dcb_nsplit_pack_main / _dc0, packed once at set_param time). (c, ci) = (block width, inner width cdc = cffn): the rows of
// BLOCK_SHAPES (kernels/dcb_shapes.h), full-width and the half-width `dcb2` blocks. Bit-identical to
// the launch sequence. y may alias x (a workgroup reads and writes only its own pixels).
struct DcbNsplitDesc {
    const half_t* t2 = nullptr; int ldt = 0;
    const half_t* x = nullptr; int ldx = 0;
    const half_t* wmain = nullptr;              // packed dc.3 | ffn.0 | ffn.2 (dcb_nsplit_main_halves(c, ci) halves)
    const half_t* wnext = nullptr;              // packed dc.0 of the NEXT block (dcb_nsplit_dc0_halves(c, ci)) or null
    const half_t* b3 = nullptr; const half_t* b0 = nullptr; const half_t* b2 = nullptr; const half_t* b1n = nullptr;
    const half_t* q = nullptr; const half_t* q2 = nullptr;
    half_t* t1n = nullptr; int ldt1 = 0;
    half_t* y = nullptr; int ldy = 0;
    int pixels = 0, c = 0, ci = 0;
    bool shortcut = false;
    // round 6: instead of the next block's dc.0 the launch can run the 1x1 conv that CLOSES a chain (y_prior_fusion.conv.3,
    // y_spatial_prior.conv.3, decoder.conv2, recon_head.head ...): yfin = (Wfin y + bfin) [* qfin] -> fp16, width nfin.
    // wfin = dcb_nsplit_pack_fin's stream. Bit-identical to conv1x1(bias [, q]) on y. With a closing conv y may be null: the
    // block's own output then never leaves LDS (nothing else reads it in the codecs).
    const half_t* wfin = nullptr; const half_t* bfin = nullptr; const half_t* qfin = nullptr;
    half_t* yfin = nullptr; int ldyfin = 0; int nfin = 0;
    // round 6: the block's depthwise conv inside the launch (dcb_nsplit_dw_supported shapes): t1 = dc.0's output [pixels][ldt]
    // INSTEAD of t2, wdw = the taps [9][ci] (tap major, as dwconv3x3 takes them), width = the picture's width (pixels = rows x width).
    // Bit-identical to dwconv3x3 + the launch on its output. t1 must not be the buffer t1n is written to (a workgroup reads its
    // neighbours' rows of t1).
    const half_t* t1 = nullptr; const half_t* wdw = nullptr; int width = 0;
};
bool dcb_nsplit_dw_supported(int c, int ci, int pixels);      // (256, 128); (384, 192) on 32-pixel workgroups. DCVC_NSPLIT_DW=0: never (A/B)
bool dcb_nsplit_shape(int c, int ci);                         // a shape the kernel is instantiated for
void dcb_nsplit_check_shape(int c, int ci);                   // throws std::invalid_argument naming the shapes there are
bool dcb_nsplit_supported(int c, int cdc, int cffn);          // DCVC_NSPLIT: 0 = off, 1 = full-width blocks only (A/B)
size_t dcb_nsplit_main_halves(int c, int ci);
size_t dcb_nsplit_dc0_halves(int c, int ci);
void dcb_nsplit_pack_main(const half_t* w3, const half_t* w0, const half_t* w2, int c, int ci, half_t* out, hipStream_t stream);
void dcb_nsplit_pack_dc0(const half_t* w1, int c, int ci, half_t* out, hipStream_t stream);
bool dcb_nsplit_fin_supported(int c, int ci, int nn);        // a closing conv of width nn behind a (c, ci) block in one launch
size_t dcb_nsplit_fin_halves(int c, int nn);
bool dcb_nsplit_fin_packable(int c, int nn);                 // a closing conv [nn][c] dcb_nsplit_pack_fin takes (FinW::load packs exactly these)
void dcb_nsplit_pack_fin(const half_t* w /* [nn][c] */, int c, int nn, half_t* out, hipStream_t stream);
void dcb_nsplit(const DcbNsplitDesc& d, hipStream_t stream);
void dcb_nsplit_timeline_buffer(long long* device_buffer);    // tuning aid: [workgroups][32] shader-clock stamps
void dcb_nsplit_dw_hook(const half_t* t1, const half_t* wdw, int width);      // tuning aid: dcb_nsplit launches take their depthwise conv inside, on these operands (null: off)

// The two 1x1 convs in front of a block's depthwise conv in one launch (dcb_pair8_kernel.h, round 6):
//   y = Wa x + ba (the block's adaptor, layers_proxy.cpp:73-77);  t1 = WSiLU(W1 y + b1) (dc.0, :79).
// wa = dcb_pair_pack_adaptor's stream, w1 = the block's dcb_nsplit_pack_dc0 stream. Bit-identical to conv1x1 + conv1x1(wsilu).
struct DcbPairDesc {
    const half_t* x = nullptr; int ldx = 0;
    const half_t* wa = nullptr; const half_t* ba = nullptr;
    const half_t* w1 = nullptr; const half_t* b1 = nullptr;
    half_t* y = nullptr; int ldy = 0;
    half_t* t1 = nullptr; int ldt1 = 0;
    int pixels = 0, cin = 0, c = 0, ci = 0;
};
bool dcb_pair_supported(int cin, int c, int ci);
size_t dcb_pair_adaptor_halves(int cin, int c);
void dcb_pair_pack_adaptor(const half_t* wa /* [c][cin] */, int cin, int c, half_t* out, hipStream_t stream);
void dcb_pair(const DcbPairDesc& d, hipStream_t stream);

struct ConvKxKDesc {
    const half_t* x = nullptr; int ldx = 0;     // [in_h][in_w][ldx]
    const half_t* w = nullptr;                  // [cout][ky][kx][cin]  (tap major, cin contiguous)
    const half_t* bias = nullptr;
    const half_t* zeros = nullptr;              // >= 128 B of zeros
    half_t* y = nullptr; int ldy = 0;           // [out_h][out_w][ldy]
    int in_h = 0, in_w = 0, cin = 0, cout = 0, ksize = 0, stride = 1, pad = 0;
    // batch: n pictures back to back in x ([n][in_h][in_w][ldx]) and y ([n][out_h][out_w][ldy]); in_h / out_h are per picture,
    // the padding taps follow each picture's own rows. n = 1: one picture, the launch of before
    int n = 1;
};
void conv_kxk(const ConvKxKDesc& d, hipStream_t stream);

struct TConv2x2Desc {
    const half_t* x = nullptr; int ldx = 0;     // [in_h][in_w][ldx]
    const half_t* w = nullptr;                  // [4 = dy*2+dx][cout][cin]
    half_t* y = nullptr; int ldy = 0;           // [2 in_h][2 in_w][ldy]
    int in_h = 0, in_w = 0, cin = 0, cout = 0;
    int n = 1;                                  // n pictures back to back (no overlap: stacking them is the same layout)
};
void tconv2x2(const TConv2x2Desc& d, hipStream_t stream);

// ---------------------------------------------------------------- fused FFN (ffn_fused.hip)
// out = W2 * chunk_add(WSiLU(W0 * x + b0)) + b2 + x [+ r2] [* q]  (then [* q2] on the rounded
// output): ffn.0 and ffn.2 of a DepthConvBlock (layers_proxy.cpp:84-98) in one launch, bit-identical
// to conv1x1(wsilu, chunk_add) followed by conv1x1(r1 = x, ...). y may alias x.
struct FfnFusedDesc {
    const half_t* x = nullptr; int ldx = 0;     // [pixels][ldx], first c channels
    const half_t* w0 = nullptr;                 // [4*cffn][c]
    const half_t* b0 = nullptr;                 // [4*cffn]
    const half_t* w2 = nullptr;                 // [c][cffn]
    const half_t* b2 = nullptr;                 // [c]
    const half_t* r2 = nullptr; int ldr2 = 0;   // optional second residual
    const half_t* q = nullptr;                  // optional fused scale
    const half_t* q2 = nullptr;                 // optional scale on the rounded output
    half_t* y = nullptr; int ldy = 0;
    int pixels = 0, c = 0, cffn = 0;
};
// shapes the fused kernel takes (c in {128, 256, 384}, cffn % 64 == 0) AND that are large enough to
// fill the chip with 128-row strips; DCVC_FFN_FUSED=0 switches the fusion off (A/B measurements)
bool ffn_fused_supported(int pixels, int c, int cffn);
void ffn_fused(const FfnFusedDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- DepthConvBlock tail (dcb_tail.hip)
// Everything of a half-width DepthConvBlock behind dc.0 in one launch (layers_proxy.cpp:79-98):
//   t2 = depthwise3x3(t) (when dw != null; else t IS t2), y1 = W3 t2 + b3 + x, then the FFN
//   out = W2 chunk_add(WSiLU(W0 y1 + b0)) + b2 + y1 [+ x when shortcut] [* q], rounded, [* q2].
// c in {128, 256}, cdc <= 128 (half-width blocks, and the full-width 128-wide ones) and cffn multiples of 64. Bit-identical to the
// four-launch sequence.
// y may alias x; t must not alias y.
struct DcbTailDesc {
    const half_t* w1 = nullptr;                 // dc.0 weights [cdc][c] + bias [cdc]: when given (with dw), dc.0 (1x1 +
    const half_t* b1 = nullptr;                 //   WSiLU on x) runs inside the launch as well and `t` is not read
    const half_t* t = nullptr; int ldt = 0;     // dc.0 output [H*W][ldt] (first cdc channels)
    const half_t* dw = nullptr;                 // [9][cdc] tap-major depthwise weights, or null
    const half_t* x = nullptr; int ldx = 0;     // block-internal input (residual of dc.3)
    const half_t* w3 = nullptr;                 // [c][cdc]
    const half_t* b3 = nullptr;                 // [c] (depthwise bias folded in)
    const half_t* w0 = nullptr;                 // [4*cffn][c]
    const half_t* b0 = nullptr;
    const half_t* w2 = nullptr;                 // [c][cffn]
    const half_t* b2 = nullptr;
    const half_t* q = nullptr;
    const half_t* q2 = nullptr;
    half_t* y = nullptr; int ldy = 0;
    int H = 0, W = 0, c = 0, cdc = 0, cffn = 0;
    bool shortcut = false;                      // ffn.2 also adds x (block-level shortcut)
    int n = 1;                                  // n pictures of H x W back to back in t, x and y (the halo stays in each picture)
};
// shape supported AND enough 8x16 patches to fill the chip; DCVC_DCB_TAIL=0 / 2 = never / whenever possible
bool dcb_tail_supported(int H, int W, int c, int cdc, int cffn);
bool dcb_tail_takes_dc0();       // false only for A/B measurements (DCVC_DCB_TAIL=3)
void dcb_tail(const DcbTailDesc& d, hipStream_t stream);
// debugging aid: when non-null, launches with dc.0 inside also write dc.0's output of every pixel
// ([H*W][cdc]) to this device buffer
void dcb_tail_debug_buffer(half_t* device_buffer);

// ---------------------------------------------------------------- depthwise 3x3 (dwconv.hip)
// y[h][w][c] = sum_{ky,kx} x[h+ky-1][w+kx-1][c] * wt[ky][kx][c]   (zero padding, no bias: the
// reference folds the bias into the next 1x1, layers_proxy.cpp:175-178)
void dwconv3x3(const half_t* x, int ldx, const half_t* wt /* [9][C] */, half_t* y, int ldy,
               int H, int W, int C, hipStream_t stream);
// n pictures of H x W back to back in x and y ([n][H][W][ld]); the zero padding follows each picture's own rows
void dwconv3x3_b(const half_t* x, int ldx, const half_t* wt, half_t* y, int ldy, int H, int W, int C, int n,
                 hipStream_t stream);

// ---------------------------------------------------------------- layout kernels (layout.hip)
// x: [H][W][C3] (channels_last view of [1, C3, H, W]); out: [H8][W8][C3*64] with pixel stride
// ldout (0 = dense), replicate padding.
void pad_unshuffle8(const half_t* x, int H, int W, int C3, half_t* out, int H8, int W8,
                    hipStream_t stream, int ldout = 0);
// in: [H8][W8][C3*64] -> out: [H8*8][W8*8][C3] with optional clamp to [-0.5, 0.5]
void shuffle8(const half_t* in, int ldin, int H8, int W8, int C3, bool clamp, half_t* out,
              hipStream_t stream);
// in: [H][W][4*C] -> out [2H][2W][C]   (pixel_shuffle(2), HT-L biased SubpelConv2x)
void shuffle2(const half_t* in, int ldin, int H, int W, int C, half_t* out, int ldout,
              hipStream_t stream);
// replicate pad bottom/right: in [H][W][C] -> out [H+pb][W+pr][C]; with pb = pr = 0 a strided copy
void replicate_pad(const half_t* in, int ldin, int H, int W, int C, int pad_b, int pad_r,
                   half_t* out, int ldout, hipStream_t stream);
// crop: in [Hin][Win][C] -> out [H][W][C]
void crop(const half_t* in, int ldin, int Win, half_t* out, int ldout, int H, int W, int C,
          hipStream_t stream);
// Batched forms (intra batches): n pictures back to back on both sides, each with the per-picture geometry
// of the single form; n = 1 is the single launch. crop_b also needs the input picture's height.
void pad_unshuffle8_b(const half_t* x, int H, int W, int C3, half_t* out, int H8, int W8, int n, hipStream_t stream,
                      int ldout = 0);
void shuffle8_b(const half_t* in, int ldin, int H8, int W8, int C3, bool clamp, half_t* out, int n, hipStream_t stream);
void replicate_pad_b(const half_t* in, int ldin, int H, int W, int C, int pad_b, int pad_r, half_t* out, int ldout, int n,
                     hipStream_t stream);
void crop_b(const half_t* in, int ldin, int Hin, int Win, half_t* out, int ldout, int H, int W, int C, int n,
            hipStream_t stream);
// y = x * q[c] (fp16 multiply, may be in place)
void mul_channel(const half_t* x, int ldx, const half_t* q, half_t* y, int ldy, int pixels, int C,
                 hipStream_t stream);

// y = x * max(q, 0.5) (add_and_multiply_with_clamp_min, stream.cu:40-76, after the add) or, with
// `reciprocal`, y = x * fp16(1 / max(q, 0.5)) (divide_with_clamp, stream.cu:422-443); q is a tensor
void scale_clamped(const half_t* x, int ldx, const half_t* q, int ldq, half_t* y, int ldy, int pixels,
                   int C, bool reciprocal, hipStream_t stream);

// ---------------------------------------------------------------- YUV pictures (picture_yuv.hip)
// One picture in file layout - Y [H][W], then Cb / Cr as planes [2][Hc][Wc] or, for NV12, interleaved [Hc][Wc][2] - of 8-bit
// (u8) or 9..16-bit (u16: LSB-aligned in the planar formats, in the high bits for NV12 = P010 / P012 / P016) samples.
constexpr int kPixYuv420p = 0, kPixYuv422p = 1, kPixYuv444p = 2, kPixNv12 = 3;      // DCVC_PIX_*
// samples of one picture; throws for an unknown format or sides that are not positive and even
long long pix_picture_samples(int fmt, int H, int W);
// -> x fp16, 3 channels per pixel at pixel stride ldx (3 for one picture, 24 + a channel offset for a chunk of 8):
// nearest-neighbour chroma, x = fp16(fp16(fp32(v) / fp32(max_val)) - 0.5) with max_val = 2^b - 1 (test_video.py:69-123,
// transforms.py:69-80; DCVC-FM's YUVReader) and / or `planar`: the picture as LSB-aligned planar samples (Y, Cb, Cr at the
// format's subsampling). One of the two may be null.
void pix_to_x(const void* src, int fmt, int bit_depth, int H, int W, half_t* x, int ldx, void* planar, hipStream_t stream);
// x_hat fp16 [rows][row_pixels][3] -> the top-left H x W picture as planar fp32 distortion planes [H][W] + [2][Hc][Wc] (what
// get_distortion measures, test_video.py:32-45: scaled to 0..max_val and clamped) and / or the samples in file layout (rint,
// half to even: DCVC-FM's YUVWriter; the 4:2:0 layouts at 8 bits truncate Cb / Cr as the reference's writer does,
// test_video.py:356-363). Chroma: the mean of the 1, 2 or 2 x 2 luma positions of fp16(x_hat + 0.5), summed in fp32 and
// rounded to fp16 once. Null outputs are skipped.
void x_to_pix(const half_t* x, int row_pixels, int H, int W, int fmt, int bit_depth, float* dist, void* out, hipStream_t stream);
// The 4:2:0 planar forms of the two with the planes handed over one by one (y [H][W], uv [2][H/2][W/2]); the same kernels
// and bits. 8 bits: the distortion planes are fp16 (the same values), and each of the four outputs may be null.
void yuv420_to_x(const uint8_t* y, const uint8_t* uv, int H, int W, half_t* x, int ldx, hipStream_t stream);
void x_to_yuv420(const half_t* x, int row_pixels, int H, int W, half_t* y16, half_t* uv16, uint8_t* y8,
                 uint8_t* uv8, hipStream_t stream);
// 9..16 bits: dist and yuv are whole pictures, [H][W] + [2][H/2][W/2]
void yuv420p16_to_x(const uint16_t* y, const uint16_t* uv, int H, int W, int bit_depth, half_t* x, int ldx, hipStream_t stream);
void x_to_yuv420p16(const half_t* x, int row_pixels, int H, int W, int bit_depth, float* dist, uint16_t* yuv, hipStream_t stream);

// ---------------------------------------------------------------- wire formats (wire_formats.hip)
// Capture and file layouts in front of pix_to_x and behind x_to_pix: NV21 (8 bits), NV16 / P210 and YUY2 / Y210 (8..16 bits,
// u16 samples in the high bits), UYVY (8 bits) and v210 (10 bits in 32-bit words, rows of 128 ceil(W / 48) bytes).
constexpr int kWireNv21 = 0, kWireNv16 = 1, kWireUyvy = 2, kWireYuy2 = 3, kWireV210 = 4;      // DCVC_WIRE_*
// the kPix* layout that holds a wire format's samples at its subsampling (NV12 for NV21, else YUV422P); throws for an unknown one
int wire_carrier(int wire);
// file bytes of one picture; throws for an unknown format, a depth the format does not have, sides that are not positive and even
long long wire_picture_bytes(int wire, int bit_depth, int H, int W);
// src (one wire picture) -> carrier (one picture in the carrier's file layout, as pix_to_x takes it) and back; one launch each.
// Throw before the launch: null operands, what wire_picture_bytes refuses, ranges that overlap.
void wire_unpack(const void* src, int wire, int bit_depth, int H, int W, void* carrier, hipStream_t stream);
void wire_pack(const void* carrier, int wire, int bit_depth, int H, int W, void* dst, hipStream_t stream);

// ---------------------------------------------------------------- MS-SSIM (msssim.hip)
// metrics.py:27-91 calc_msssim of n_planes pairs of H x W planes (u8 or fp16 samples in 0..255; src and rec share row_stride
// and plane_stride, in samples), fp64 after the load; out[plane] (device, fp64). The workspace (msssim_workspace_bytes) holds the
// downsampled planes and the per-workgroup partial sums; 1 + 4 or 5 launches on `stream`.
// u16 / fp32 samples (high bit depth) in 0..data_range; C1 and C2 follow data_range (fp64), 255 by default.
constexpr int kSampleU8 = 0, kSampleF16 = 1;        // DCVC_SAMPLE_U8 / DCVC_SAMPLE_F16
constexpr int kSampleU16 = 3, kSampleF32 = 4;       // DCVC_SAMPLE_U16 / DCVC_SAMPLE_F32 (2 stays unassigned)
inline bool known_sample(int t) { return t == kSampleU8 || t == kSampleF16 || t == kSampleU16 || t == kSampleF32; }
struct MsssimDesc {
    const void* src = nullptr; int src_dtype = kSampleU8;
    const void* rec = nullptr; int rec_dtype = kSampleU8;
    int n_planes = 0, H = 0, W = 0;
    int row_stride = 0; long long plane_stride = 0;
    double* out = nullptr;
    double data_range = 255.0;
};
void msssim_validate(const MsssimDesc& d);       // throws std::invalid_argument for a geometry or operand msssim() refuses
size_t msssim_workspace_bytes(int n_planes, int H, int W);
void msssim(const MsssimDesc& d, void* workspace, hipStream_t stream);

// ---------------------------------------------------------------- RGB pictures (rgb_cs.hip)
// test_video.py:87-122 + transforms.py:17-27 (BT.709 rgb2ycbcr): u8 RGB read through (row, pixel, channel) strides in bytes
// (packed HWC: 3W, 3, 1; planar CHW: W, 1, H*W) -> x fp16 at pixel stride ldx (3 channels written; 3 for one picture, 24
// for the slots of an 8-picture chunk) and / or a planar u8 copy [3][H][W] of the source. Either output may be null.
struct RgbToXDesc {
    const uint8_t* src = nullptr;
    long long row_stride = 0, pixel_stride = 0, channel_stride = 0;
    int H = 0, W = 0;
    half_t* x = nullptr; int ldx = 3;
    uint8_t* planar = nullptr;
};
void rgb_to_x(const RgbToXDesc& d, hipStream_t stream);
// test_video.py:55-64 + transforms.py:53-66 (ycbcr2rgb) and :366-370: x_hat fp16 [rows][row_pixels][3] -> the top-left
// H x W picture as planar fp16 [3][H][W] in 0..255 (the distortion planes) and / or packed u8 HWC (rint of those, the
// writer's pixels). Null outputs are skipped.
void x_to_rgb(const half_t* x, int row_pixels, int H, int W, half_t* rgb16, uint8_t* rgb8, hipStream_t stream);
// rgb_to_x / x_to_rgb with the colour matrix (DCVC_MATRIX_*) and range (DCVC_RANGE_*) chosen; yuv_bit_depth (8..16) is the
// depth b of the YUV samples x stands for (x = v / (2^b - 1) - 0.5), which places the limited-range levels. Layouts, null
// rules and refusals are those of the two functions above, which are these at BT.709 / full range.
constexpr int kMatrixBt601 = 0, kMatrixBt709 = 1, kMatrixBt2020 = 2;
constexpr int kRangeFull = 0, kRangeLimited = 1;
struct ColourSpace {
    int matrix = kMatrixBt709, range = kRangeFull, yuv_bit_depth = 8;
};
void rgb_to_x_cs(const RgbToXDesc& d, const ColourSpace& cs, hipStream_t stream);
void x_to_rgb_cs(const half_t* x, int row_pixels, int H, int W, half_t* rgb16, uint8_t* rgb8, const ColourSpace& cs, hipStream_t stream);
// 9..16-bit RGB: u16 samples, LSB-aligned in 0..max_val = 2^bit_depth - 1, strides in samples; the unit value
// is fp32(v) / fp32(max_val), a correctly rounded division, and from there on the 8-bit conversion. planar: u16 [3][H][W].
struct Rgb16ToXDesc {
    const uint16_t* src = nullptr;
    long long row_stride = 0, pixel_stride = 0, channel_stride = 0;
    int bit_depth = 16;
    int H = 0, W = 0;
    half_t* x = nullptr; int ldx = 3;
    uint16_t* planar = nullptr;
};
void rgb16_to_x_cs(const Rgb16ToXDesc& d, const ColourSpace& cs, hipStream_t stream);
// x_hat -> dist32: planar fp32 [3][H][W] = clamp(fp32(fp16(clamp(rgb, 0, 1))) * max_val, 0, max_val), the distortion planes,
// and / or rgb16u: packed u16 [H][W][3] = rint of those (half to even, NaN -> 0). One of the two may be null, not both.
void x_to_rgb16_cs(const half_t* x, int row_pixels, int H, int W, int bit_depth, float* dist32, uint16_t* rgb16u, const ColourSpace& cs,
                   hipStream_t stream);

// ---------------------------------------------------------------- SSE (sse.hip)
// metrics.py:10-24's fp64 sum of squared differences of n_planes pairs of H x W planes (u8, fp16, u16 or fp32 samples; src and rec share
// row_stride and plane_stride, in samples) -> out[plane] (device). Per-workgroup partials in the workspace
// (sse_workspace_bytes), reduced by a second launch in a fixed order.
struct SseDesc {
    const void* src = nullptr; int src_dtype = kSampleU8;
    const void* rec = nullptr; int rec_dtype = kSampleU8;
    int n_planes = 0, H = 0, W = 0;
    int row_stride = 0; long long plane_stride = 0;
    double* out = nullptr;
};
void sse_validate(const SseDesc& d);             // throws std::invalid_argument for a geometry or operand sse() refuses
size_t sse_workspace_bytes(int n_planes, int H, int W);
void sse(const SseDesc& d, void* workspace, hipStream_t stream);

// ---------------------------------------------------------------- scene-cut measurement (scene.hip)
// x fp16, pixel (r, c) at x + (r W + c) ldx (all ldx halfs of a pixel readable), luma in channel 0 -> luma u8 [H][W] =
// clamp(rintf((float(x0) + 0.5f) * 255.f), 0, 255) and *sad (one device uint64) = sum |luma - prev| over the plane, an
// exact integer; prev null: *sad = 0. At most two launches, no host synchronisation.
constexpr int kLumaSadMaxSide = 16384;
struct LumaSadDesc {
    const half_t* x = nullptr; int ldx = 3;
    int H = 0, W = 0;
    const uint8_t* prev = nullptr;
    uint8_t* luma = nullptr;
    void* sad = nullptr;
};
void luma_sad_validate(const LumaSadDesc& d);    // throws std::invalid_argument for what luma_sad() refuses
void luma_sad(const LumaSadDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- picture hashes (crc32.hip)
// out[k] (device uint32 [n]) = zlib's crc32 of the bytes base[offsets[k] .. offsets[k] + lengths[k]), 0 for an empty segment;
// out[n..] is not touched. offsets and lengths are host arrays, read during the call. An exact integer result, the same for
// every launch geometry and arrival order. At most two launches, no allocation, no host synchronisation.
constexpr int kCrc32MaxSegments = 16;
struct Crc32Desc {
    const void* base = nullptr;
    const long long* offsets = nullptr;
    const long long* lengths = nullptr;
    int n = 0;
    void* out = nullptr;
};
void crc32_validate(const Crc32Desc& d);         // throws std::invalid_argument for what crc32_segments() refuses
void crc32_segments(const Crc32Desc& d, hipStream_t stream);
uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, long long len_b);      // host: crc32(A || B); throws for len_b < 0

// ---------------------------------------------------------------- resampling (resample.hip)
// Planes of u8 / u16 samples at another size: separable integer Lanczos-3, horizontal pass then vertical pass through an
// intermediate plane of clamped samples (the filter is stated at the head of resample.hip).
constexpr int kResampleMaxSide = 16384;
constexpr int kResampleMaxRatio = 8;             // each side's ratio lies in [1/8, 8]
constexpr int kResampleMaxTaps = 48;
int resample_ntaps(int n_in, int n_out);         // host; -1 for a length outside 1..kResampleMaxSide or a ratio outside [1/8, 8]
// host: coef [n_out][T] (every row sums to 4096), first [n_out]; throws std::invalid_argument for what resample_ntaps refuses
void resample_taps(int n_in, int n_out, int16_t* coef, int32_t* first);
struct ResamplePlan {
    int in_h = 0, in_w = 0, out_h = 0, out_w = 0;
    int taps_w = 0, taps_h = 0;
    int span_w = 0;                              // samples of a horizontal tile's row segment in LDS (a multiple of 16)
    void* tables = nullptr;                      // the device allocation behind the four tables
    const int16_t* coef_w = nullptr; const int32_t* first_w = nullptr;
    const int16_t* coef_h = nullptr; const int32_t* first_h = nullptr;
};
ResamplePlan* resample_plan_create(int in_h, int in_w, int out_h, int out_w);     // tables onto the current device (synchronous)
void resample_plan_free(ResamplePlan* p);
unsigned long long resample_workspace_bytes(const ResamplePlan& p, int n_planes);
struct ResampleDesc {
    const void* src = nullptr; int src_dtype = kSampleU8; int src_row_stride = 0; long long src_plane_stride = 0;
    void* dst = nullptr; int dst_dtype = kSampleU8; int dst_row_stride = 0; long long dst_plane_stride = 0;
    int n_planes = 1, max_val = 255;
    void* workspace = nullptr; long long workspace_bytes = 0;
};
void resample_validate(const ResamplePlan& p, const ResampleDesc& d);     // throws std::invalid_argument for what is refused
// two launches on `stream`: validates first, allocates nothing, never waits for the host
void resample_planes(const ResamplePlan& p, const ResampleDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- denoising prefilter (denoise.hip)
// Planes of u8 / u16 samples through an edge-preserving 3x3 spatial stage and a motion-adaptive recursive temporal stage
// against the previous output picture (the filter is stated at the head of denoise.hip). Strides in samples.
constexpr int kDenoiseMaxSide = 16384;
struct DenoiseDesc {
    const void* src = nullptr; int src_row_stride = 0; long long src_plane_stride = 0;
    const void* prev = nullptr; int prev_row_stride = 0; long long prev_plane_stride = 0;      // nullptr: no history
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0;
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0, n_planes = 1;
    int spatial = 0, temporal = 0;                   // 0..64, in 8-bit code values
};
void denoise_validate(const DenoiseDesc& d);         // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void denoise_planes(const DenoiseDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- deinterlacer (deinterlace.hip)
// Planes of u8 / u16 samples of a woven frame: the rows of parity `keep` are copied, the others made from an edge-directed
// spatial interpolation blended, by a motion measure against the previous input frame, with the woven sample (DESIGN.md 27;
// the filter is stated at the head of deinterlace.hip). Strides in samples.
constexpr int kDeinterlaceMaxSide = 16384;
struct DeinterlaceDesc {
    const void* cur = nullptr; int cur_row_stride = 0; long long cur_plane_stride = 0;
    const void* prev = nullptr; int prev_row_stride = 0; long long prev_plane_stride = 0;      // nullptr: spatial only
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0;
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0, n_planes = 1;
    int keep = 0, weave_from_prev = 0;               // 0 or 1
    int threshold = 0;                               // 0..64, in 8-bit code values
};
void deinterlace_validate(const DeinterlaceDesc& d);      // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void deinterlace_planes(const DeinterlaceDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- inverse telecine (ivtc.hip)
// field_match: how well the second field of a woven luma plane (rows of parity 1 - first) fits the first field of the same
// frame (c) or the second field of the previous frame fits it (p), and how much the first field differs from the previous
// frame's (dup): eight exact uint64 words on the device (stated at the head of ivtc.hip). Strides in samples.
constexpr int kIvtcMaxSide = 16384;
struct FieldMatchDesc {
    const void* cur = nullptr; int cur_row_stride = 0;
    const void* prev = nullptr; int prev_row_stride = 0;      // nullptr: words 1, 3, 5 and 6 are 0
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0;
    int first = 0;                                   // 0 or 1: the parity of the rows of the field shown first
    int cthresh = 0;                                 // 0..255, in 8-bit code values
    void* out8 = nullptr;                            // device, 8-byte aligned: [match_c, match_p, comb_c, comb_p, blkmax_c, blkmax_p, dup, 0]
};
void field_match_validate(const FieldMatchDesc& d);       // throws std::invalid_argument for what is refused
// two launches on `stream`: validates first, allocates nothing, never waits for the host
void field_match(const FieldMatchDesc& d, hipStream_t stream);
// weave_fields: dst rows of parity `first` from plane set a, the others from b, every plane on its own
struct WeaveFieldsDesc {
    const void* a = nullptr; int a_row_stride = 0; long long a_plane_stride = 0;
    const void* b = nullptr; int b_row_stride = 0; long long b_plane_stride = 0;
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0;
    int dtype = kSampleU8, H = 0, W = 0, n_planes = 1, first = 0;
};
void weave_fields_validate(const WeaveFieldsDesc& d);     // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void weave_fields(const WeaveFieldsDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- film grain (grain.hip)
// grain_apply: synthetic grain onto the planes of a decoded picture - a 64 x 64 template per plane at a hashed offset per 32 x 32
// block, scaled by a table over the collocated luma; grain_stats: what a denoiser took out of a source picture, per luma bin,
// in 16 exact uint64 words a plane (both stated at the head of grain.hip). Strides in samples.
constexpr int kGrainMaxSide = 16384;
struct GrainApplyDesc {
    const void* rec = nullptr; int rec_row_stride = 0; long long rec_plane_stride = 0;
    const void* luma = nullptr; int luma_row_stride = 0; int Hl = 0, Wl = 0;      // the ungrained luma plane all planes share
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0;  // may be rec
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0, n_planes = 1;
    int first_plane = 0;                             // the planes are first_plane .. first_plane + n_planes - 1 of Y, U, V
    int sx = 0, sy = 0;                              // 0 or 1: the planes' subsampling against the luma plane
    const int16_t* templates[3] = {nullptr, nullptr, nullptr};      // device, int16 [64][64] each; read for the call's planes
    const uint8_t* lut = nullptr;                    // host, [3][9]
    uint32_t seed = 0, pic = 0;
};
void grain_apply_validate(const GrainApplyDesc& d);  // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void grain_apply(const GrainApplyDesc& d, hipStream_t stream);
struct GrainStatsDesc {
    const void* src = nullptr; int src_row_stride = 0; long long src_plane_stride = 0;
    const void* den = nullptr; int den_row_stride = 0; long long den_plane_stride = 0;
    const void* luma = nullptr; int luma_row_stride = 0; int Hl = 0, Wl = 0;      // den's luma plane
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0, n_planes = 1, sx = 0, sy = 0;
    int flat = 0;                                    // 0..255, in 8-bit code values
    int accumulate = 0;                              // 0: the words are zeroed first; 1: added to
    void* words = nullptr;                           // device, 8-byte aligned: per plane n[0..7], S[0..7]
};
void grain_stats_validate(const GrainStatsDesc& d);  // throws std::invalid_argument for what is refused
// one launch (two with accumulate == 0) on `stream`: validates first, allocates nothing, never waits for the host
void grain_stats(const GrainStatsDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- black-bar crop (crop.hip)
// crop_stats: per row and per column of a luma plane the number of samples above limit << (bit_depth - 8): H + W exact uint32
// words on the device, rows first (stated at the head of crop.hip). Strides in samples.
constexpr int kCropMaxSide = 16384;
struct CropStatsDesc {
    const void* luma = nullptr; int row_stride = 0;
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0;
    int limit = 0;                                   // 0..255, in 8-bit code values
    void* counts = nullptr;                          // device, 4-byte aligned: uint32 [H + W]
};
void crop_stats_validate(const CropStatsDesc& d);    // throws std::invalid_argument for what is refused
// two launches on `stream`: validates first, allocates nothing, never waits for the host
void crop_stats(const CropStatsDesc& d, hipStream_t stream);
// window_planes: dst[p][y][x] = src[p][y + oy][x + ox] inside the source, fill[p] outside: a crop, a pad or any mixture
struct WindowPlanesDesc {
    const void* src = nullptr; int src_row_stride = 0; long long src_plane_stride = 0; int Hs = 0, Ws = 0;
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0; int Hd = 0, Wd = 0;
    int dtype = kSampleU8, n_planes = 1;
    int ox = 0, oy = 0;                              // signed, |.| <= kCropMaxSide
    const int* fill = nullptr;                       // host, [n_planes]
};
void window_planes_validate(const WindowPlanesDesc& d);   // throws std::invalid_argument for what is refused
// one launch for every 16 planes on `stream`: validates first, allocates nothing, never waits for the host
void window_planes(const WindowPlanesDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- block motion search and compensation (motion.hip)
// motion_search: one integer vector per 16 x 16 block of a luma plane against a reference plane, a two-level search in exact
// integers; motion_compensate_planes: planes fetched through those vectors (both stated at the head of
// motion.hip). Strides in samples.
constexpr int kMotionMaxSide = 16384;
constexpr int kMotionBlock = 16;
constexpr int kMotionMaxRange = 15;
constexpr int kMotionMaxLambda = 255;
struct MotionSearchDesc {
    const void* cur = nullptr; int cur_row_stride = 0;
    const void* ref = nullptr; int ref_row_stride = 0;           // may be cur
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0;
    int range = 0;                                   // 0..15, in half-resolution samples
    int lambda = 0;                                  // 0..255, in 8-bit code values a sample of vector length
    void* mv = nullptr; int mv_bh = 0, mv_bw = 0;    // device int16 [mv_bh][mv_bw][2] holding (dx, dy); the grid's own pitch
    void* sad = nullptr;                             // device uint32 [mv_bh][mv_bw], or nullptr
    void* moved = nullptr;                           // device uint32, or nullptr: + the number of blocks with a vector != (0, 0)
    void* workspace = nullptr; long long workspace_bytes = 0;
};
size_t motion_search_workspace_bytes(int H, int W);  // the two half-resolution planes
void motion_search_validate(const MotionSearchDesc& d);      // throws std::invalid_argument for what is refused
// two launches on `stream`: validates first, allocates nothing, never waits for the host
void motion_search(const MotionSearchDesc& d, hipStream_t stream);
struct MotionCompensateDesc {
    const void* prev = nullptr; int prev_row_stride = 0; long long prev_plane_stride = 0;
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0;
    int dtype = kSampleU8, H = 0, W = 0, n_planes = 1;
    int sx = 0, sy = 0;                              // the planes' subsampling against the luma plane of the search
    const void* mv = nullptr; int mv_bh = 0, mv_bw = 0;
};
void motion_compensate_validate(const MotionCompensateDesc& d);   // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void motion_compensate_planes(const MotionCompensateDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- frame-rate conversion (interp.hip)
// The picture at k / n of the way from picture a to picture b, through the vectors of motion_search(cur = b, ref = a):
// interp_select picks, per 16 x 16 block of the in-between picture, the vector under which a and b agree best and marks the
// blocks where they do not agree; interp_planes fetches both pictures through that plan and blends (both stated at
// the head of interp.hip). Strides in samples.
constexpr int kInterpMinN = 2, kInterpMaxN = 8;
constexpr int kInterpMaxLimit = 255;
constexpr int kInterpMaxVec = 31;                    // a component of mv is clamped to -31..31 when read
struct InterpSelectDesc {
    const void* a = nullptr; int a_row_stride = 0;   // luma of the earlier picture
    const void* b = nullptr; int b_row_stride = 0;   // ... of the later one
    int dtype = kSampleU8, bit_depth = 8, H = 0, W = 0;
    const void* mv = nullptr; int mv_bh = 0, mv_bw = 0;  // device int16 [mv_bh][mv_bw][2]: (dx, dy), b[p] ~ a[p + v]
    int k = 1, n = 2;                                // the phase k / n, k in 1..n-1
    int limit = 8;                                   // 0..255, 8-bit code values a sample: a block above it falls back
    void* plan = nullptr;                            // device int16 [plan_bh][plan_bw][4]: (ax, ay, bx, by)
    void* wb = nullptr;                              // device uint8 [plan_bh][plan_bw]: b's weight of n
    int plan_bh = 0, plan_bw = 0;
    void* sad = nullptr;                             // device uint32 [plan_bh][plan_bw], or nullptr: the winner's SAD
    void* fallen = nullptr;                          // device uint32, or nullptr: + the number of blocks that fell back
};
void interp_select_validate(const InterpSelectDesc& d);      // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void interp_select(const InterpSelectDesc& d, hipStream_t stream);
struct InterpPlanesDesc {
    const void* a = nullptr; int a_row_stride = 0; long long a_plane_stride = 0;
    const void* b = nullptr; int b_row_stride = 0; long long b_plane_stride = 0;
    void* dst = nullptr; int dst_row_stride = 0; long long dst_plane_stride = 0;
    int dtype = kSampleU8, H = 0, W = 0, n_planes = 1;
    int sx = 0, sy = 0;                              // the planes' subsampling against the luma plane of the selection
    const void* plan = nullptr; const void* wb = nullptr; int plan_bh = 0, plan_bw = 0;
    int k = 1, n = 2;
    const void* fallen = nullptr; int n_blocks = 0;  // device uint32, or nullptr: 2 * fallen > n_blocks repeats the whole picture
};
void interp_planes_validate(const InterpPlanesDesc& d);      // throws std::invalid_argument for what is refused
// one launch on `stream`: validates first, allocates nothing, never waits for the host
void interp_planes(const InterpPlanesDesc& d, hipStream_t stream);

// ---------------------------------------------------------------- symbol kernels (symbols.hip)
// Uploads the scale -> Gaussian-table-index lookup table (call once per process before the
// first symbol kernel and outside any graph capture).
void symbols_init();
// number of 2048-element blocks the symbol kernels use for `count` elements (= size of block_count)
int symbol_blocks(int count);

// z -> round half away, clamp [-64, 63] -> fp16 z_hat and int8 symbols
void round_z(const half_t* z, half_t* z_hat, int8_t* z_i8, int count, hipStream_t stream);
void int8_to_half(const int8_t* in, half_t* out, int count, hipStream_t stream);

// One step (0..3) of the 4-step masked quantisation of y (encoder side): fuses the reference's
// process_with_mask + single_part_for_writing_4x (x2) + build_index_enc + compaction counting.
struct YStepEnc {
    const half_t* y = nullptr; int ldy = 0;            // scaled latent [P][C]
    const half_t* scales = nullptr; int lds = 0;       // [P][C]
    const half_t* means = nullptr; int ldm = 0;        // [P][C]
    half_t* y_hat_acc = nullptr; int ldacc = 0;        // y_hat_so_far [P][C] (written for the active group)
    int16_t* sym = nullptr;                            // [P * C/4] (symbol << 8) + index, NHWC order
    uint8_t* cond = nullptr;                           // [P * C/4 / 8] 8 skip flags per byte
    int32_t* block_count = nullptr;                    // [blocks] kept symbols per 2048-element block
    int H = 0, W = 0, C = 0, step = 0;
    float skip_thres = 0.f;
    bool first = false;                                // step 0 initialises y_hat_acc (copy, not add)
    // n pictures of H x W back to back in every operand: y / scales / means / y_hat_acc [n][P][ld], sym [n][P*C/4],
    // cond [n][P*C/32], block_count [n][symbol_blocks(P*C/4)]. The masks follow each picture's own (y, x).
    int n = 1;
};
void y_step_enc(const YStepEnc& d, hipStream_t stream);

// Decoder side: scales of the active group -> table index + skip flag (+ counting)
struct YStepDecIndex {
    const half_t* scales = nullptr; int lds = 0;
    uint8_t* index = nullptr;                          // [P * C/4]
    uint8_t* cond = nullptr;
    int32_t* block_count = nullptr;
    int H = 0, W = 0, C = 0, step = 0;
    float skip_thres = 0.f;
    int n = 1;                                         // n pictures, laid out as YStepEnc's
};
void y_step_dec_index(const YStepDecIndex& d, hipStream_t stream);

// Stream compaction out[base + rank] = in[i] for kept i (ELEM = 2: int16 symbols, 1: uint8 index).
// base = total[0..slot) summed; total[slot] receives this step's kept count.
void compact(const void* in, int elem_bytes, const uint8_t* cond, const int32_t* block_count,
             int count, void* out, int32_t* totals, int slot, hipStream_t stream);
// n pictures of `count` elements each (in [n][count], cond [n][count/8], block_count [n][symbol_blocks(count)]), each
// compacted into its own region: picture b writes out + b * out_stride (elements) and totals + b * totals_stride (int32s),
// with the base of its own totals[0..slot). count must be a multiple of 8.
void compact_b(const void* in, int elem_bytes, const uint8_t* cond, const int32_t* block_count, int count, void* out,
               long long out_stride, int32_t* totals, int totals_stride, int slot, int n, hipStream_t stream);

// Decoder: scatter decoded int8 symbols back (zeros where skipped), add the mean of the active
// group and accumulate into y_hat_so_far (restore_y_4x*, stream.cu:757-844).
struct YStepDecRestore {
    const int8_t* decoded = nullptr;                   // compacted, this step's symbols start at totals-base
    const uint8_t* cond = nullptr;
    const int32_t* block_count = nullptr;
    const int32_t* totals = nullptr; int slot = 0;
    const half_t* means = nullptr; int ldm = 0;
    half_t* y_hat_acc = nullptr; int ldacc = 0;
    int H = 0, W = 0, C = 0, step = 0;
    bool first = false;
    // n pictures, laid out as YStepEnc's; picture b's symbols start at decoded + b * decoded_stride and its totals at
    // totals + b * totals_stride
    int n = 1;
    long long decoded_stride = 0;
    int totals_stride = 0;
};
void y_step_dec_restore(const YStepDecRestore& d, hipStream_t stream);

// ---------------------------------------------------------------- full-tensor masked steps (inter models)
// The inter models quantise ALL channels of y against one scale tensor in `nsteps` masked steps and
// entropy-code them in one go:
//   nsteps = 2 (LD):   mask_0 = first channel half on even (h + w), second half on odd; mask_1 the
//                      complement (dmc_ld_proxy.cpp:672-683)
//   nsteps = 4 (HT-S): the channel-group x 2x2-position masks of the intra model
//                      (dmc_hts_proxy.cpp:869-890 == common_model.py:174-195)
// A run of 8 channels never straddles a channel group, so every 8-channel vector of a pixel belongs
// to exactly one step.
//
// Encoder step k:
//   k == 0:          y *= 1/max(q_dec, 0.5) in place (divide_with_clamp, stream.cu:422-443) and
//                    y_hat = 0 at the positions of later steps;
//   active positions: quantise against `means` -> symbol (<< 8 | scale index), y_hat = y_q + mean
//                    (process_with_mask_kernel, stream.cu:549-630);
//   k == nsteps - 1: everywhere y_hat *= max(q_dec, 0.5), plus the skip flags / per-block counts of
//                    ALL symbols (build_index_enc, stream.cu:130-161).
struct MaskStepEnc {
    half_t* y = nullptr; int ldy = 0;
    const half_t* q_dec = nullptr; int ldq = 0;
    const half_t* scales = nullptr; int lds = 0;
    const half_t* means = nullptr; int ldm = 0;
    half_t* y_hat = nullptr; int ldh = 0;
    int16_t* sym = nullptr;                 // [P * C] NHWC order
    uint8_t* cond = nullptr;                // [P * C / 8]   (last step)
    int32_t* block_count = nullptr;         // [blocks]      (last step)
    int H = 0, W = 0, C = 0, nsteps = 2, step = 0;
    float skip_thres = 0.f;
};
void mask_step_enc(const MaskStepEnc& d, hipStream_t stream);

// Decoder: table index + skip flag of every symbol (build_index_dec, stream.cu:100-128)
struct MaskDecIndex {
    const half_t* scales = nullptr; int lds = 0;
    uint8_t* index = nullptr;
    uint8_t* cond = nullptr;
    int32_t* block_count = nullptr;
    int H = 0, W = 0, C = 0;
    float skip_thres = 0.f;
};
void mask_dec_index(const MaskDecIndex& d, hipStream_t stream);

// Decoder step k:
//   k == 0:          scatter the decoded symbols back (conditional_recover, stream.cu:360-383); the
//                    symbols of later steps are parked in `yq`, their y_hat is zeroed;
//   active positions: y_hat = y_q + means   (restore_y_kernel, stream.cu:686-729);
//   k == nsteps - 1: everywhere y_hat *= max(q_dec, 0.5).
struct MaskStepDec {
    const int8_t* decoded = nullptr;        // compacted symbols (step 0)
    const uint8_t* cond = nullptr;
    const int32_t* block_count = nullptr;
    const int32_t* totals = nullptr;
    int8_t* yq = nullptr;                   // [P * C] scratch
    const half_t* means = nullptr; int ldm = 0;
    const half_t* q_dec = nullptr; int ldq = 0;
    half_t* y_hat = nullptr; int ldh = 0;
    int H = 0, W = 0, C = 0, nsteps = 2, step = 0;
};
void mask_step_dec(const MaskStepDec& d, hipStream_t stream);

// ---------------------------------------------------------------- code length (code_length.hip)
// Sum of the cost-table entries (rans/code_length.h, units of 2^-16 bit) of the symbols of n pictures: the ideal length
// of the stream the host coder would build from them. Integer sums, so exact and the same on every run. The sums are
// ADDED to out (unsigned 64-bit, device memory): the caller zeroes it.
struct CodeLengthY {
    const int16_t* sym = nullptr;           // (q << 8) + cdf index, as y_step_enc writes them; 16-byte aligned
    long long sym_stride = 0;               // picture b's symbols start at sym + b * sym_stride (a multiple of 8)
    const uint8_t* cond = nullptr;          // keep bits of the uncompacted layout (bit i of byte e / 8), picture b at
    long long cond_stride = 0;              //   cond + b * cond_stride; nullptr: every symbol counts (compacted layout)
    const int32_t* totals = nullptr;        // device-side counts: picture b holds totals[b * totals_stride + 0 .. n_totals)
    int totals_stride = 0, n_totals = 0;    //   summed symbols (compacted layout); nullptr: `count` symbols
    int count = 0;                          // symbols per picture, or with totals the most a picture can hold
    const uint32_t* table = nullptr;        // [num_cdf][256], column uint8(q)
    int num_cdf = 0;                        // a symbol whose index is not below it counts nothing
    unsigned long long* out = nullptr;      // picture b: out[b * out_stride] += cost, out[b * out_stride + kept_slot] += symbols
    int out_stride = 1, kept_slot = -1;     //   counted (kept_slot < 0: not written)
    int n = 1;
};
void code_length_y(const CodeLengthY& d, hipStream_t stream);

struct CodeLengthZ {
    const int8_t* z = nullptr;              // [n][count], values in [-64, 63]; symbol i is coded with row i % ch
    int count = 0, ch = 1;
    const uint32_t* table = nullptr;        // [ch][128] rows of the selected q_index, column z + 64
    unsigned long long* out = nullptr;      // picture b: out[b * out_stride] += cost
    int out_stride = 1;
    int n = 1;
};
void code_length_z(const CodeLengthZ& d, hipStream_t stream);

}  // namespace dcvc
