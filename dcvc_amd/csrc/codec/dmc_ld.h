// DMC low-delay inter codec (DCVC-UF "LD") on MI355X. Replaces the reference class DMCLDProxy
// (src/layers/extensions/inference/dmc_ld_proxy.{h,cpp}): set_param / add_ref_feature_from_frame /
// compress / decompress. One picture per call; the temporal state (feature memory, last decoded
// feature, context, temporal prior) stays resident in HBM between calls.
#pragma once

#include "codec/inter_codec.h"

namespace dcvc {

class DmcLdCodec : public InterCodec {
public:
    // video_model_ld.py:16-21
    static constexpr int kChSrc = 192, kChY = 128, kChD = 256, kChM = 256;

    DmcLdCodec();

    // dmc_ld_proxy.cpp:595-639
    void set_param(const ParamStore& ps, float skip_thres);

    // dmc_ld_proxy.cpp:407-418. frame: device fp16 [H][W][3], the intra codec's reconstruction
    // (any size; extended by edge replication to multiples of 16 like the pictures themselves).
    void add_ref_feature_from_frame(const half_t* frame, int height, int width, bool apply_adaptor,
                                    hipStream_t stream);

    // dmc_ld_proxy.cpp:420-473. Returns ec_parallel; the bit stream is in stream_bytes().
    int compress(const half_t* x, int height, int width, int qp, bool reset_feature_memory,
                 hipStream_t stream);

    // dmc_ld_proxy.cpp:475-593. x_hat: device fp16 [H16*16][W16*16][3], caller-owned.
    void decompress(const uint8_t* bits, size_t nbytes, int qp, int height, int width, int ec_parallel,
                    bool reset_feature_memory, half_t* x_hat, hipStream_t stream);

    // Not in the reference: the size probe. What compress(x, qp, ...) would spend, without coding: the first
    // stage of compress (the same launches, the same graph), then the code lengths summed on the device. units = {y, z}
    // in 2^-16 bit, kept (may be null) = the y symbols that would be coded. Neither the temporal state nor the stream of
    // the last compress changes. Refused, with nothing touched: qp outside 0..63, no encoder-side reference, a picture size
    // other than the temporal state's.
    void estimate_bits(const half_t* x, int height, int width, int qp, int64_t units[2], int64_t* kept, hipStream_t stream);

    // Not in the reference: the encoder-side reconstruction. The picture of the unit whose feature_p the
    // object holds - after compress, after decompress, after import_state of such a state - bit-identical to what
    // decompress of that unit's stream writes. x_hat: device fp16 [H16*16][W16*16][3]. A stage of its own (the recon head
    // into a scratch plane, shuffle8) that reads feature_p and writes no state: export_state gives the bytes it gave
    // before, and every later call gives what it gives without this one. Refused, with nothing touched: no parameters,
    // no feature_p yet.
    void reconstruct(half_t* x_hat, hipStream_t stream);

    size_t debug_read(const std::string& name, void* dst, size_t cap, hipStream_t stream);

    // Temporal state as one flat DEVICE buffer (reference feature, memory | feature_p, ctx, temporal
    // prior + the validity flags in a 64-byte header): what another GPU needs to continue the same
    // GOP (torch.distributed.send / recv over RCCL, dcvc_amd/sharding.py). export with dst == nullptr
    // returns the size. import requires the same picture size and parameters.
    size_t export_state(void* dst, size_t cap, hipStream_t stream);
    void import_state(const void* src, size_t bytes, int height, int width, hipStream_t stream);

private:
    void prepare(int height, int width);
    std::vector<StatePart> state_parts() const;
    // sub-networks (operands are fixed views of the resident buffers, see prepare())
    // feed_fe: the feature extractor runs RIGHT behind this chain (nothing in between touches the scratch planes): the
    // chain's last launch also computes dc.0 of its first block (ChainCall::after), and run_fe is told so (dc0_done ->
    // ChainCall::first_dc0_done)
    void run_fa_i(hipStream_t st, bool feed_fe = false);     // FI -> memory
    void run_fa_m(hipStream_t st, bool feed_fe = false);     // [memory | feature_p] -> memory
    void run_fe(hipStream_t st, bool dc0_done = false);      // memory -> ctx
    void run_tpe(hipStream_t st);                     // memory -> temporal params
    void run_encoder(hipStream_t st);                 // [x unshuffled | ctx] -> Y
    void run_hyper_encoder(hipStream_t st);           // Y -> z, z_hat
    void run_priors(hipStream_t st);                  // z_hat, temporal -> common params (the temporal prior is only read)
    void run_spatial_prior(hipStream_t st);           // [y_hat | common] -> means of step 1
    void run_decoder(hipStream_t st);                 // y_hat, ctx -> feature_p
    void run_recon_head(half_t* head, half_t* x_hat, hipStream_t st);   // feature_p -> head: FI or RHS (+ x_hat)
    void enc_stage0(hipStream_t st);                  // x, ctx, temporal -> symbols, totals, z: all compress() codes

    // ---- parameters
    DcbW m_fa_i[4], m_fa_m[4], m_fe[5];
    DcbW m_encb[3];               // encoder.conv1.0, .1 and encoder.conv2: one chain of three blocks, the last with the quant scale
    ConvKW m_enc_down;
    DcbW m_henc0;
    Stride2W m_henc1, m_henc2;
    UpsampleW m_hdec0, m_hdec1;
    DcbW m_hdec2;
    Stride2W m_tpe;
    DcbW m_fus[3];
    FinW m_fus3;
    DcbW m_sp[2];
    FinW m_sp2;
    SubpelW m_dec_up;
    DcbW m_dec1[3];
    FinW m_dec2;
    DcbW m_rh[3];
    FinW m_rh_head;

    // ---- resident buffers (per resolution, views into m_bmem)
    half_t* m_FI = nullptr;      // [P8][192]  reference feature: unshuffled I picture / recon-head output
    half_t* m_CATM = nullptr;    // [P8][512]  memory | feature_p          (feature_adaptor_m input)
    half_t* m_CATD = nullptr;    // [P8][512]  decoder.up out (x unshuffled at 64:256) | ctx
    half_t* m_T = nullptr;       // [P8][256]  chain temporaries (the blocks ping-pong between the two)
    half_t* m_T2 = nullptr;
    half_t *m_Y = nullptr, *m_Ypad = nullptr;
    half_t *m_Z1 = nullptr, *m_Z2 = nullptr, *m_Z3 = nullptr, *m_ZH = nullptr;
    half_t *m_H1 = nullptr, *m_H2 = nullptr, *m_HP = nullptr;
    half_t* m_TP = nullptr;      // [P16][256] temporal params: state, written by run_tpe alone
    half_t* m_PF = nullptr;      // [P16][384] hyper params | temporal params * q_feature: the fusion chain, in place
    half_t* m_CATSP = nullptr;   // [P16][512] y_hat | q_dec | scales | means
    half_t* m_SPT = nullptr;     // [P16][256]
    half_t* m_MEANS1 = nullptr;  // [P16][128]
    half_t* m_RHS = nullptr;     // [P8][192]  reconstruct(): its head output (FI is state)
};

}  // namespace dcvc
