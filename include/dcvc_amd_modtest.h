/* TEST SURFACE - not part of the product ABI.
 *
 * The module layer (dcvc_amd/csrc/codec/modules.{h,hip}: DcbW, run_dcb_chain / DcbChain, Stride2W, SubpelW, UpsampleW, FinW /
 * FinCall, Scratch) reached without a codec around it, so that tests/test_modules_gpu.py can run its launch choices and its
 * buffer bookkeeping against plain launch sequences at grids of their own choosing. Nothing in the product calls these.
 *
 * Conventions of the other headers: int status (0, or -1 with dcvc_last_error() set - the modules' std::invalid_argument
 * refusals arrive that way with their message), an explicit stream, and no allocation or synchronisation inside a run call
 * (the *_forward entries; create / set_param / load_* / read allocate and synchronise).
 *
 * A handle owns a parameter store, a device arena for the prepared weights, the three scratch planes of `scratch_elems`
 * halves each with Scratch::batch = batch, and a page of zeros for the padding taps. Modules are loaded from a checkpoint
 * prefix and named by the index load_* returns; a block is named by (module, index): index i of a block array, index 0 =
 * the block of a stride-2 or up-sampling module. module < 0 = no block (next / after / fin absent).
 * Activations are (pointer, ld, c) views into buffers the caller owns, [batch][H][W][ld] halves.
 */
#ifndef DCVC_AMD_MODTEST_H
#define DCVC_AMD_MODTEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcvc_modtest dcvc_modtest;

dcvc_modtest* dcvc_modtest_create(long long scratch_elems, int batch);       /* NULL on error */
void dcvc_modtest_destroy(dcvc_modtest* h);
/* as dcvc_dmci_set_param: checkpoint layout, host memory, dtype 0 = fp16, 1 = fp32, 2 = int32 */
int dcvc_modtest_set_param(dcvc_modtest* h, const char* name, const void* data, int dtype, const int64_t* dims, int ndim);

/* n > 0: DcbW[n] from prefix + "0.", "1.", ...; n = 0: a DcbChain (as many blocks as the store has); n < 0: ONE block at prefix */
int dcvc_modtest_load_blocks(dcvc_modtest* h, const char* prefix, int n);
int dcvc_modtest_load_stride2(dcvc_modtest* h, const char* prefix, int shortcut);
int dcvc_modtest_load_upsample(dcvc_modtest* h, const char* prefix, int shortcut);
int dcvc_modtest_load_subpel(dcvc_modtest* h, const char* prefix);
int dcvc_modtest_load_fin(dcvc_modtest* h, const char* prefix);
int dcvc_modtest_blocks(dcvc_modtest* h, int module);                          /* number of blocks of a module */

/* what load() decided: out[0] = nsplit(), out[1] = packed_adaptor != null, out[2] = one_launch(H, W),
 * out[3] = feeds(next block) (0 without one), out[4..7] = c, cdc, cffn, adaptor cin (0 without an adaptor) */
int dcvc_modtest_block_info(dcvc_modtest* h, int module, int index, int H, int W, int next_module, int next_index, int* out);
/* out[0] = the closing conv has a packed stream, out[1] = cin, out[2] = cout */
int dcvc_modtest_fin_info(dcvc_modtest* h, int module, int* out);

/* prepared device tensors back to the host; returns the number of halves (at most cap are written) or -1 */
#define DCVC_MODTEST_TAPS     0   /* block: depthwise taps [9][cdc] */
#define DCVC_MODTEST_FOLDED   1   /* block: dc.3 bias with the depthwise bias folded in [c] */
#define DCVC_MODTEST_STRIDE2  2   /* stride-2 module: [cout][2][2][cin] */
#define DCVC_MODTEST_SUBPEL   3   /* sub-pixel / up-sampling module: [4][cout][cin] or [4 cout][k][k][cin] */
long long dcvc_modtest_read(dcvc_modtest* h, int module, int index, int what, void* dst, long long cap);

/* the scratch planes and Scratch::hand (state tests) */
int dcvc_modtest_scratch(dcvc_modtest* h, void** t1, void** t2, void** t3, int* hand);

/* DcbW::forward, the flat arguments gathered into its DcbCall. fin_module < 0: no closing conv */
int dcvc_modtest_block_forward(dcvc_modtest* h, int module, int index, void* x, int ldx, int cx, void* y, int ldy, int cy,
                               int H, int W, int shortcut, const void* q_fused, const void* q_after,
                               void* alt, int ldalt, int calt, int next_module, int next_index, int dc0_done,
                               int fin_module, const void* fin_q, void* fin_y, int fin_ldy, int keep_block_output, void* stream);
/* run_dcb_chain over blocks [first, first + n) of a module, the flat arguments gathered into its ChainCall (n = 0: all of
 * them; a DcbChain that is run whole runs through DcbChain::forward) */
int dcvc_modtest_chain_forward(dcvc_modtest* h, int module, int first, int n, void* x, int ldx, int cx,
                               void* tmp, int ldtmp, int ctmp, void* y, int ldy, int cy, int H, int W,
                               const void* q_fused_last, void* tmp2, int ldtmp2, int ctmp2,
                               int fin_module, const void* fin_q, void* fin_y, int fin_ldy, int keep_block_output,
                               int after_module, int after_index, int first_dc0_done, void* stream);
/* the same with ChainCall::q_after_last (chain_forward passes null); an entry of its own so that callers bound to
 * chain_forward's argument list keep working */
int dcvc_modtest_chain_forward_qa(dcvc_modtest* h, int module, int first, int n, void* x, int ldx, int cx,
                                  void* tmp, int ldtmp, int ctmp, void* y, int ldy, int cy, int H, int W,
                                  const void* q_fused_last, const void* q_after_last, void* tmp2, int ldtmp2, int ctmp2,
                                  int fin_module, const void* fin_q, void* fin_y, int fin_ldy, int keep_block_output,
                                  int after_module, int after_index, int first_dc0_done, void* stream);
int dcvc_modtest_stride2_forward(dcvc_modtest* h, int module, void* x, int ldx, int cx, void* tmp, int ldtmp, int ctmp,
                                 void* y, int ldy, int cy, int H, int W, void* stream);
int dcvc_modtest_upsample_forward(dcvc_modtest* h, int module, void* x, int ldx, int cx, void* tmp, int ldtmp, int ctmp,
                                  void* y, int ldy, int cy, int H, int W, void* up_tmp, int with_zeros,
                                  int next_module, int next_index, void* stream);
int dcvc_modtest_subpel_forward(dcvc_modtest* h, int module, void* x, int ldx, int cx, void* y, int ldy, int cy, int H, int W,
                                void* up_tmp, int with_zeros, int n, void* stream);

/* The block kernels' packed weight streams (tests/test_block_pack_gpu.py): packs device weights into the device buffer `out`
 * (cap halves) on `stream` and returns the stream's size in halves, or -1. No handle, no allocation, no synchronisation.
 * (a, b) = (c, ci) for MAIN (w0 = dc.3 [c][ci], w1 = ffn.0 [4 ci][c], w2 = ffn.2 [c][ci]) and DC0 (w0 [ci][c]), (c, nn) for
 * FIN (w0 [nn][c]), (cin, c) for ADAPTOR (w0 [c][cin]); w1, w2 null but for MAIN */
#define DCVC_MODTEST_PACK_MAIN    0
#define DCVC_MODTEST_PACK_DC0     1
#define DCVC_MODTEST_PACK_FIN     2
#define DCVC_MODTEST_PACK_ADAPTOR 3
long long dcvc_modtest_pack_stream(int kind, const void* w0, const void* w1, const void* w2, int a, int b, void* out, long long cap,
                                   void* stream);

#ifdef __cplusplus
}
#endif

#endif
