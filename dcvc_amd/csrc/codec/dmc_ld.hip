// DMC-LD codec orchestration on MI355X (see dmc_ld.h). Dataflow follows dmc_ld_proxy.cpp:407-593;
// as in the intra codec the launch structure is ours: one hipGraph per stage for all qps, the
// concatenations of the reference (torch.cat inputs of the adaptor blocks) are fixed channel
// ranges of resident buffers, and the two checkerboard steps are fused symbol kernels.
#include "codec/dmc_ld.h"

#include <algorithm>

namespace dcvc {

namespace {

enum StageKey : int { kRef = 0, kEnc0 = 1, kEnc1 = 2 /* +reset */, kDec0 = 10 /* +memory_has_value */,
                      kDec1 = 12, kDec2 = 13, kDec3 = 14, kRecon = 30 };
constexpr uint32_t kLdMagic = 0x44434c44;     // "DCLD"

}  // namespace

DmcLdCodec::DmcLdCodec() : InterCodec("DMC-LD")
{
    // LD's kernels are short (4.2 ms of kernel time in ~350 launches per 1080p picture): measured on
    // MI355X, eager launches on the codec's stream beat hipGraph replay (139 vs 123 pictures/s), the
    // other codecs are neutral. set_use_graphs(true) switches back.
    m_use_graphs = false;
}

// ------------------------------------------------------------------------------------ set_param
void DmcLdCodec::set_param(const ParamStore& ps, float skip_thres)
{
    begin_set_param(ps, skip_thres, kChD, 2 * kChY);
    auto chain = [&](DcbW* blocks, int n, const std::string& prefix) {
        for (int i = 0; i < n; ++i) blocks[i].load(ps, m_wmem, prefix + std::to_string(i) + ".");
    };
    chain(m_fa_i, 4, "feature_adaptor_i.conv.");
    chain(m_fa_m, 4, "feature_adaptor_m.conv.");
    chain(m_fe, 5, "feature_extractor.conv.");
    chain(m_encb, 2, "encoder.conv1.");
    m_encb[2].load(ps, m_wmem, "encoder.conv2.");
    m_enc_down.load(ps, m_wmem, "encoder.down.");
    m_henc0.load(ps, m_wmem, "hyper_encoder.conv.0.");
    m_henc1.load(ps, m_wmem, "hyper_encoder.conv.1.", false);      // dmc_ld_proxy.cpp:250-251
    m_henc2.load(ps, m_wmem, "hyper_encoder.conv.2.", false);
    m_hdec0.load(ps, m_wmem, "hyper_decoder.conv.0.", false);      // dmc_ld_proxy.cpp:221-222
    m_hdec1.load(ps, m_wmem, "hyper_decoder.conv.1.", false);
    m_hdec2.load(ps, m_wmem, "hyper_decoder.conv.2.");
    m_tpe.load(ps, m_wmem, "temporal_prior_encoder.conv.", false); // dmc_ld_proxy.cpp:366
    chain(m_fus, 3, "y_prior_fusion.conv.");
    m_fus3.load(ps, m_wmem, "y_prior_fusion.conv.3.");
    chain(m_sp, 2, "y_spatial_prior.conv.");
    m_sp2.load(ps, m_wmem, "y_spatial_prior.conv.2.");
    m_dec_up.load(ps, m_wmem, "decoder.up.");
    chain(m_dec1, 3, "decoder.conv1.");
    m_dec2.load(ps, m_wmem, "decoder.conv2.");
    chain(m_rh, 3, "recon_head.conv.");
    m_rh_head.load(ps, m_wmem, "recon_head.head.");
    finish_set_param(ps);
}

// ------------------------------------------------------------------------------------ buffers
void DmcLdCodec::prepare(int height, int width)
{
    if (!begin_prepare(height, width)) return;
    const Geometry& g = m_g;
    auto H = [&](size_t n) { return m_bmem.alloc_half(n); };
    const size_t P8 = g.P8(), P16 = g.P16(), P16p = g.P16p(), P32 = g.P32(), P64 = g.P64();
    m_s.elems = std::max<size_t>(P8 * (kChM / 2), P16p * (3 * kChY / 2));
    m_s.t1 = H(m_s.elems); m_s.t2 = H(m_s.elems); m_s.t3 = H(m_s.elems);
    m_FI = H(P8 * kChSrc);
    m_CATM = H(P8 * (kChM + kChD));
    m_CATD = H(P8 * (kChD + kChM));
    m_T = H(P8 * kChM); m_T2 = H(P8 * kChM);
    m_Y = H(P16 * kChY); m_Ypad = g.padded() ? H(P16p * kChY) : m_Y;
    m_Z1 = H(P16p * kChZ); m_Z2 = H(P32 * kChZ); m_Z3 = H(P64 * kChZ); m_ZH = H(P64 * kChZ);
    m_ZI8 = static_cast<int8_t*>(m_bmem.alloc(P64 * kChZ));
    m_H1 = H(P32 * kChZ); m_H2 = H(P16p * kChZ); m_HP = H(P16p * kChY);
    m_TP = H(P16 * 2 * kChY);
    m_PF = H(P16 * 3 * kChY);
    m_CATSP = H(P16 * 4 * kChY);
    m_SPT = H(P16 * 2 * kChY);
    m_MEANS1 = H(P16 * kChY);
    const size_t n = P16 * kChY;
    alloc_symbol_buffers(n, 1, n);      // the compacted indexes of the one round trip, no count in front
    m_RHS = H(P8 * kChSrc);             // last: every other buffer keeps the address it had without it
}

// ------------------------------------------------------------------------------------ networks
void DmcLdCodec::run_fa_i(hipStream_t st, bool feed_fe)
{
    const View t(m_T, kChM, kChM);
    ChainCall c; c.tmp2 = View(m_T2, kChM, kChM); c.after = feed_fe && m_fa_i[3].feeds(m_fe[0]) ? &m_fe[0] : nullptr;
    run_dcb_chain(m_fa_i, 4, View(m_FI, kChSrc, kChSrc), t, View(m_CATM, kChM + kChD, kChM), m_g.H8, m_g.W8, m_s, st, c);
}

void DmcLdCodec::run_fa_m(hipStream_t st, bool feed_fe)
{
    const View t(m_T, kChM, kChM);
    ChainCall c; c.tmp2 = View(m_T2, kChM, kChM); c.after = feed_fe && m_fa_m[3].feeds(m_fe[0]) ? &m_fe[0] : nullptr;
    run_dcb_chain(m_fa_m, 4, View(m_CATM, kChM + kChD, kChM + kChD), t, View(m_CATM, kChM + kChD, kChM),
                  m_g.H8, m_g.W8, m_s, st, c);
}

void DmcLdCodec::run_fe(hipStream_t st, bool dc0_done)
{
    const View t(m_T, kChM, kChM);
    ChainCall c; c.tmp2 = View(m_T2, kChM, kChM); c.first_dc0_done = dc0_done;
    run_dcb_chain(m_fe, 5, View(m_CATM, kChM + kChD, kChM), t, View(m_CATD + kChD, kChD + kChM, kChM),
                  m_g.H8, m_g.W8, m_s, st, c);
}

void DmcLdCodec::run_tpe(hipStream_t st)
{
    const View out(m_TP, 2 * kChY, 2 * kChY);
    m_tpe.forward(View(m_CATM, kChM + kChD, kChM), out, out, m_g.H8, m_g.W8, m_zeros, m_s, st);
}

void DmcLdCodec::run_encoder(hipStream_t st)
{
    const Geometry& g = m_g;
    const View t(m_T, kChD, kChD);
    // [x unshuffled | ctx] = channels 64..511 of CATD (dmc_ld_proxy.cpp:755-757)
    // encoder.conv1 (two blocks) and encoder.conv2 (its output scaled by q_encoder inside its last conv) as ONE chain: every
    // launch also computes dc.0 of the block behind it
    ChainCall c; c.q_fused_last = m_cur_q_encoder; c.tmp2 = View(m_T2, kChD, kChD);
    run_dcb_chain(m_encb, 3, View(m_CATD + 64, kChD + kChM, kChSrc + kChM), t, t, g.H8, g.W8, m_s, st, c);
    ConvKxKDesc d;
    d.x = m_T; d.ldx = kChD; d.w = m_enc_down.w; d.bias = m_enc_down.b; d.zeros = m_zeros;
    d.y = m_Y; d.ldy = kChY; d.in_h = g.H8; d.in_w = g.W8; d.cin = kChD; d.cout = kChY;
    d.ksize = 3; d.stride = 2; d.pad = 1;
    conv_kxk(d, st);
}

void DmcLdCodec::run_hyper_encoder(hipStream_t st)
{
    const Geometry& g = m_g;
    if (g.padded()) {
        replicate_pad(m_Y, kChY, g.H16, g.W16, kChY, g.H16p - g.H16, g.W16p - g.W16, m_Ypad, kChY, st);
    }
    const View z1(m_Z1, kChZ, kChZ), z2(m_Z2, kChZ, kChZ), z3(m_Z3, kChZ, kChZ);
    m_henc0.forward(View(m_Ypad, kChY, kChY), z1, g.H16p, g.W16p, m_s, st);
    m_henc1.forward(z1, z2, z2, g.H16p, g.W16p, m_zeros, m_s, st);
    m_henc2.forward(z2, z3, z3, g.H32, g.W32, m_zeros, m_s, st);
    round_z(m_Z3, m_ZH, m_ZI8, g.P64() * kChZ, st);
}

void DmcLdCodec::run_priors(hipStream_t st)
{
    const Geometry& g = m_g;
    const View h1(m_H1, kChZ, kChZ), h2(m_H2, kChZ, kChZ);
    m_hdec0.forward(View(m_ZH, kChZ, kChZ), h1, h1, g.H64, g.W64, m_s, st);
    m_hdec1.forward(h1, h2, h2, g.H32, g.W32, m_s, st);
    m_hdec2.forward(h2, View(m_HP, kChY, kChY), g.H16p, g.W16p, m_s, st);
    // crop_hyper_params -> first third of the fusion input (dmc_ld_proxy.cpp:437-438)
    crop(m_HP, kChY, g.W16p, m_PF, 3 * kChY, g.H16, g.W16, kChY, st);
    // the temporal prior is state (the previous picture's last stage left it, export_state carries it): it is scaled INTO
    // the fusion input, which the chain then overwrites, and stays as it is - a size probe reads it any number of times
    mul_channel(m_TP, 2 * kChY, m_cur_q_feature, m_PF + kChY, 3 * kChY, g.P16(), 2 * kChY, st);
    const View pf(m_PF, 3 * kChY, 3 * kChY);
    // y_prior_fusion: three (384, 192) blocks in place, each launch with dc.0 of the next inside, the last one with
    // y_prior_fusion.conv.3 -> (q_dec | scales | means) behind y_hat in the spatial-prior input
    const FinCall fin(m_fus3, m_CATSP + kChY, 4 * kChY);
    ChainCall c; c.fin = &fin;
    run_dcb_chain(m_fus, 3, pf, pf, pf, g.H16, g.W16, m_s, st, c);
}

void DmcLdCodec::run_spatial_prior(hipStream_t st)
{
    const Geometry& g = m_g;
    const View t(m_SPT, 2 * kChY, 2 * kChY);
    const FinCall fin(m_sp2, m_MEANS1, kChY);              // y_spatial_prior.conv.2 closes the chain
    ChainCall c; c.fin = &fin;
    run_dcb_chain(m_sp, 2, View(m_CATSP, 4 * kChY, 4 * kChY), t, t, g.H16, g.W16, m_s, st, c);
}

void DmcLdCodec::run_decoder(hipStream_t st)
{
    const Geometry& g = m_g;
    m_dec_up.forward(View(m_CATSP, 4 * kChY, kChY), View(m_CATD, kChD + kChM, kChD), g.H16, g.W16, st);
    const View t(m_T, kChD, kChD);
    // decoder.conv2 (conv1x1_bias_with_quant) closes the chain -> feature_p, second half of the adaptor_m input
    const FinCall fin(m_dec2, m_CATM + kChM, kChM + kChD, m_cur_q_decoder);
    ChainCall c; c.tmp2 = View(m_T2, kChD, kChD); c.fin = &fin;
    run_dcb_chain(m_dec1, 3, View(m_CATD, kChD + kChM, kChD + kChM), t, t, g.H8, g.W8, m_s, st, c);
}

void DmcLdCodec::run_recon_head(half_t* head, half_t* x_hat, hipStream_t st)
{
    const Geometry& g = m_g;
    const View t(m_T, kChD, kChD);
    const FinCall fin(m_rh_head, head, kChSrc);            // into FI the head output doubles as the reference feature after a reset
    ChainCall c; c.tmp2 = View(m_T2, kChD, kChD); c.fin = &fin;
    run_dcb_chain(m_rh, 3, View(m_CATM + kChM, kChM + kChD, kChD), t, t, g.H8, g.W8, m_s, st, c);
    if (x_hat != nullptr) shuffle8(head, kChSrc, g.H8, g.W8, 3, true, x_hat, st);
}

// ------------------------------------------------------------------------------------ reference frame
void DmcLdCodec::add_ref_feature_from_frame(const half_t* frame, int height, int width,
                                            bool apply_adaptor, hipStream_t user)
{
    prepare(height, width);
    hipStream_t st = enter(user);
    pad_unshuffle8(frame, height, width, 3, m_FI, m_g.H8, m_g.W8, st);
    if (apply_adaptor) {
        run_stage(kRef, st, [&] {
            run_fa_i(st, true);
            run_fe(st, m_fa_i[3].feeds(m_fe[0]));
            run_tpe(st);
        });
    }
    leave(user);
    m_flags.after_add_ref(apply_adaptor);
}

// ------------------------------------------------------------------------------------ compress
int DmcLdCodec::compress(const half_t* x, int height, int width, int qp, bool reset, hipStream_t user)
{
    prepare(height, width);
    require_encoder_ready("compress");
    const Geometry& g = m_g;
    hipStream_t st = enter(user);
    select_qp(qp, st);
    pad_unshuffle8(x, height, width, 3, m_CATD + 64, g.H8, g.W8, st, kChD + kChM);   // x varies: outside the graph
    run_stage(kEnc0, st, [&] { enc_stage0(st); });
    submit(st, [this, qp] { entropy_encode(qp, 1); });
    // decoder + temporal state update run on the GPU while the worker entropy-codes on the host
    run_stage(kEnc1 + (reset ? 1 : 0), st, [&] {
        run_decoder(st);
        if (reset) {
            run_recon_head(m_FI, nullptr, st);     // forward_reset, dmc_ld_proxy.cpp:297-305
            run_fa_i(st, true);
        } else {
            run_fa_m(st, true);
        }
        run_fe(st, (reset ? m_fa_i[3] : m_fa_m[3]).feeds(m_fe[0]));      // its first dc.0 came with the adaptor chain's last launch
        run_tpe(st);
    });
    leave(user);
    m_flags.after_compress();
    wait_job();
    return m_ec_parallel;
}

// ------------------------------------------------------------------------------------ size probe
void DmcLdCodec::enc_stage0(hipStream_t st)
{
    const Geometry& g = m_g;
    run_encoder(st);
    run_hyper_encoder(st);
    run_priors(st);
    MaskStepEnc d;
    d.y = m_Y; d.ldy = kChY;
    d.q_dec = m_CATSP + kChY; d.ldq = 4 * kChY;
    d.scales = m_CATSP + 2 * kChY; d.lds = 4 * kChY;
    d.means = m_CATSP + 3 * kChY; d.ldm = 4 * kChY;
    d.y_hat = m_CATSP; d.ldh = 4 * kChY;
    d.sym = m_SYM; d.cond = m_COND; d.block_count = m_CNT;
    d.H = g.H16; d.W = g.W16; d.C = kChY; d.step = 0; d.skip_thres = m_skip_thres;
    mask_step_enc(d, st);
    run_spatial_prior(st);
    d.means = m_MEANS1; d.ldm = kChY; d.step = 1;
    mask_step_enc(d, st);
    compact(m_SYM, 2, m_COND, m_CNT, g.P16() * kChY, m_COMP, m_TOTALS, 0, st);
}

void DmcLdCodec::estimate_bits(const half_t* x, int height, int width, int qp, int64_t units[2], int64_t* kept,
                               hipStream_t user)
{
    check_probe(qp, height, width);
    const Geometry& g = m_g;
    hipStream_t st = enter(user);
    select_qp(qp, st);
    pad_unshuffle8(x, height, width, 3, m_CATD + 64, g.H8, g.W8, st, kChD + kChM);
    // the stage compress() runs (and, with graphs, the graph it replays). It reads the temporal state - ctx, the temporal
    // prior - and writes none of it; what it leaves in the scratch buffers the next call's first stage overwrites.
    run_stage(kEnc0, st, [&] { enc_stage0(st); });
    probe_code_length(1, m_COMP, g.P16() * kChY, g.P16() * kChY, m_TOTALS, 1, m_ZI8, g.P64() * kChZ, qp, units, kept, st);
    leave(user);
}

// ------------------------------------------------------------------------------------ decompress
void DmcLdCodec::decompress(const uint8_t* bits, size_t nbytes, int qp, int height, int width,
                            int ec_parallel, bool reset, half_t* x_hat, hipStream_t user)
{
    prepare(height, width);
    require_decoder_ready();
    const Geometry& g = m_g;
    hipStream_t st = enter(user);
    select_qp(qp, st);
    const bool extend = m_flags.memory_has_value;
    run_stage(kDec0 + (extend ? 1 : 0), st, [&] {
        if (extend) run_fa_m(st);
        else run_fa_i(st);
        run_tpe(st);
    });
    // z is decoded on the host while the GPU updates the feature memory
    m_dec.set_parallel(ec_parallel);
    m_dec.set_stream(bits, nbytes);
    const int nz = g.P64() * kChZ;
    const int ny = g.P16() * kChY;
    m_dec.decode_z(nz, qp * kChZ, kChZ, m_h_z.get());
    hip_check(hipMemcpyAsync(m_ZI8, m_h_z.get(), nz, hipMemcpyHostToDevice, st), "H2D z");
    run_stage(kDec1, st, [&] {
        int8_to_half(m_ZI8, m_ZH, nz, st);
        run_priors(st);
        MaskDecIndex d;
        d.scales = m_CATSP + 2 * kChY; d.lds = 4 * kChY;
        d.index = m_IDX; d.cond = m_COND; d.block_count = m_CNT;
        d.H = g.H16; d.W = g.W16; d.C = kChY; d.skip_thres = m_skip_thres;
        mask_dec_index(d, st);
        compact(m_IDX, 1, m_COND, m_CNT, ny, m_CIDX, m_TOTALS, 0, st);
    });
    const int n = fetch_total_and_indexes(st);
    // the context network runs while the host decodes y (dmc_ld_proxy.cpp:556-560)
    run_stage(kDec2, st, [&] { run_fe(st); });
    decode_y_and_upload(n, st);
    bind_stage_arg(kDec3, x_hat);
    run_stage(kDec3, st, [&] {
        MaskStepDec d;
        d.decoded = m_DECODED; d.cond = m_COND; d.block_count = m_CNT; d.totals = m_TOTALS; d.yq = m_YQ;
        d.means = m_CATSP + 3 * kChY; d.ldm = 4 * kChY;
        d.q_dec = m_CATSP + kChY; d.ldq = 4 * kChY;
        d.y_hat = m_CATSP; d.ldh = 4 * kChY;
        d.H = g.H16; d.W = g.W16; d.C = kChY; d.step = 0;
        mask_step_dec(d, st);
        run_spatial_prior(st);
        d.means = m_MEANS1; d.ldm = kChY; d.step = 1;
        mask_step_dec(d, st);
        run_decoder(st);
        run_recon_head(m_FI, x_hat, st);
    });
    leave(user);
    m_flags.after_decompress(reset);       // the temporal params were consumed by this picture
}

// ------------------------------------------------------------------------------------ encoder-side reconstruction
void DmcLdCodec::reconstruct(half_t* x_hat, hipStream_t user)
{
    require_feature_p("reconstruct");
    hipStream_t st = enter(user);
    bind_stage_arg(kRecon, x_hat);
    // reads feature_p (the second half of CATM: run_fa_m rewrote the memory half alone); writes the chain temporaries, the
    // scratch planes, RHS and x_hat - nothing export_state carries, nothing a later stage reads before writing it
    run_stage(kRecon, st, [&] { run_recon_head(m_RHS, x_hat, st); });
    leave(user);
}

// ------------------------------------------------------------------------------------ state hand-off, debug
std::vector<InterCodec::StatePart> DmcLdCodec::state_parts() const
{
    const size_t P8 = m_g.P8(), P16 = m_g.P16();
    // reference feature, memory | feature_p, ctx (a channel slice), temporal prior
    return {{m_FI, kChSrc, kChSrc, P8}, {m_CATM, kChM + kChD, kChM + kChD, P8}, {m_CATD + kChD, kChM, kChD + kChM, P8},
            {m_TP, 2 * kChY, 2 * kChY, P16}};
}

size_t DmcLdCodec::export_state(void* dst, size_t cap, hipStream_t user)
{
    return InterCodec::export_state(kLdMagic, state_parts(), dst, cap, user);
}

void DmcLdCodec::import_state(const void* src, size_t bytes, int height, int width, hipStream_t user)
{
    prepare(height, width);
    InterCodec::import_state(kLdMagic, "import_state: not a DMC-LD state of this picture size", state_parts(), src, bytes, user);
}

size_t DmcLdCodec::debug_read(const std::string& name, void* dst, size_t cap, hipStream_t st)
{
    const Geometry& g = m_g;
    const size_t P8 = g.P8(), P16 = g.P16(), P64 = g.P64();
    return InterCodec::debug_read({{"y", m_Y, P16, kChY, kChY, 2},
                                   {"y_hat", m_CATSP, P16, kChY, 4 * kChY, 2},
                                   {"common", m_CATSP + kChY, P16, 3 * kChY, 4 * kChY, 2},
                                   {"means1", m_MEANS1, P16, kChY, kChY, 2},
                                   {"z_i8", m_ZI8, P64, kChZ, kChZ, 1},
                                   {"memory", m_CATM, P8, kChM, kChM + kChD, 2},
                                   {"feature_p", m_CATM + kChM, P8, kChD, kChM + kChD, 2},
                                   {"ctx", m_CATD + kChD, P8, kChM, kChD + kChM, 2},
                                   {"temporal", m_TP, P16, 2 * kChY, 2 * kChY, 2},
                                   {"feature_i", m_FI, P8, kChSrc, kChSrc, 2},
                                   {"symbols", m_COMP, 1, g.P16() * kChY, g.P16() * kChY, 2},
                                   {"totals", m_TOTALS, 1, 4, 4, 4}},
                                  name, dst, cap, st);
}

}  // namespace dcvc
