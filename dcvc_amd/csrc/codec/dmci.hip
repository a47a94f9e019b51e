// DMCI codec orchestration on MI355X (see dmci.h). Dataflow follows dmci_proxy.cpp:296-602; the
// launch structure does not: one hipGraph per stage for ALL qps (the per-qp scale vectors are
// copied into fixed device slots before the graph), fused per-step symbol kernels, a single
// device->host transfer of the compacted symbols of all four steps.
#include "codec/dmci.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <cstring>

namespace dcvc {

namespace {

enum StageKey : int { kEnc0 = 0, kEnc1 = 1, kDec0 = 10, kDec1 = 11 };

}  // namespace

DmciCodec::DmciCodec() = default;

DmciCodec::~DmciCodec()
{
    quiesce();
}

// ------------------------------------------------------------------------------------ set_param
void DmciCodec::set_param(const ParamStore& ps, float skip_thres)
{
    quiesce();            // compress() returns before its reconstruction graph has finished
    clear_graphs();
    m_wmem.release();
    kernels_init();
    m_skip_thres = skip_thres;
    m_q_enc = upload_qp_table(ps, m_wmem, "q_scale_enc", kChEncDec);
    m_q_dec = upload_qp_table(ps, m_wmem, "q_scale_dec", kChEncDec);
    m_q_y_enc = upload_qp_table(ps, m_wmem, "q_scale_y_enc", kChY);
    m_q_y_dec = upload_qp_table(ps, m_wmem, "q_scale_y_dec", kChY);
    m_zeros = m_wmem.alloc_half(2048);
    m_cur_q_enc = m_wmem.alloc_half(kChEncDec);
    m_cur_q_dec = m_wmem.alloc_half(kChEncDec);
    m_cur_q_y_enc = m_wmem.alloc_half(kChY);
    m_cur_q_y_dec = m_wmem.alloc_half(kChY);

    m_enc1.load(ps, m_wmem, "enc.enc_1.");
    for (int i = 0; i < 6; ++i) m_enc2[i].load(ps, m_wmem, "enc.enc_2." + std::to_string(i) + ".");
    m_enc_down.load(ps, m_wmem, "enc.enc_2.6.");
    m_henc0.load(ps, m_wmem, "hyper_enc.conv.0.");
    m_henc1.load(ps, m_wmem, "hyper_enc.conv.1.");
    m_henc2.load(ps, m_wmem, "hyper_enc.conv.2.");
    m_hdec0.load(ps, m_wmem, "hyper_dec.conv.0.");
    m_hdec1.load(ps, m_wmem, "hyper_dec.conv.1.");
    m_hdec2.load(ps, m_wmem, "hyper_dec.conv.2.");
    for (int i = 0; i < 3; ++i) m_fus[i].load(ps, m_wmem, "y_prior_fusion.conv." + std::to_string(i) + ".");
    m_fus3.load(ps, m_wmem, "y_prior_fusion.conv.3.");
    m_reduction.load(ps, m_wmem, "y_spatial_prior_reduction.");
    for (int i = 0; i < 3; ++i) {
        m_sp_adaptor[i].load(ps, m_wmem, "y_spatial_prior_adaptor_" + std::to_string(i + 1) + ".");
        m_sp[i].load(ps, m_wmem, "y_spatial_prior.conv." + std::to_string(i) + ".");
    }
    m_sp3.load(ps, m_wmem, "y_spatial_prior.conv.3.");
    m_dec_up.load(ps, m_wmem, "dec.dec_1.0.");
    for (int i = 0; i < 12; ++i) m_dec1[i].load(ps, m_wmem, "dec.dec_1." + std::to_string(i + 1) + ".");
    m_dec2.load(ps, m_wmem, "dec.dec_2.");

    load_cdf_tables(ps);
    upload_code_length_tables(ps, m_wmem, kChZ, kMaxBatch);      // for estimate_bits
    m_has_params = true;
}

// ------------------------------------------------------------------------------------ buffers
// n pictures back to back in every buffer: [n][rows][cols][ld] with one picture's geometry. The stage graphs are captured
// per (H, W, n): a change of any of them drops them with the buffers.
void DmciCodec::prepare(int height, int width, int n)
{
    if (!m_has_params) throw std::runtime_error("DMCI: set_param() has not been called");
    if (n < 1 || n > kMaxBatch) throw std::invalid_argument("DMCI: batch size must be in [1, 16]");
    if (m_g.H == height && m_g.W == width && m_g.N == n) return;
    quiesce();
    clear_graphs();
    m_bmem.release();
    m_g = BatchGeometry();
    BatchGeometry g;
    static_cast<Geometry&>(g) = Geometry::of(height, width);
    g.N = n;
    g.H = height; g.W = width;
    auto H = [&](size_t count) { return m_bmem.alloc_half(count); };
    // every pixel count is that of the whole batch
    const size_t N = n;
    const size_t P8 = N * g.P8(), P16 = N * g.P16(), P16p = N * g.P16p(), P32 = N * g.P32(), P64 = N * g.P64();
    m_s.elems = std::max<size_t>(P8 * kChEncDec, P16p * 2 * kChY);
    m_s.batch = n;
    m_s.t1 = H(m_s.elems); m_s.t2 = H(m_s.elems); m_s.t3 = H(m_s.elems);
    m_U = H(P8 * kChSrc); m_F = H(P8 * kChEncDec);
    m_Y = H(P16 * kChY); m_Ypad = g.padded() ? H(P16p * kChY) : m_Y;
    m_Z1 = H(P16p * kChZ); m_Z2a = H(P32 * kChZ); m_Z2 = H(P32 * kChZ);
    m_Z3a = H(P64 * kChZ); m_Z3 = H(P64 * kChZ); m_ZH = H(P64 * kChZ);
    m_ZI8 = static_cast<int8_t*>(m_bmem.alloc(P64 * kChZ));
    m_H1a = H(P32 * kChZ); m_H1 = H(P32 * kChZ); m_H2a = H(P16p * kChZ); m_H2 = H(P16p * kChZ);
    m_HP = H(P16p * kChY);
    m_PF = H(P16p * 2 * kChY); m_PARAMSp = H(P16p * 2 * kChY);
    m_PARAMS = g.padded() ? H(P16 * 2 * kChY) : m_PARAMSp;
    m_CAT = H(P16 * 2 * kChY); m_AD = H(P16 * 2 * kChY); m_SP = H(P16 * 2 * kChY);
    m_YHAT = H(P16 * kChY);
    m_D0 = H(P8 * kChEncDec); m_D1 = H(P8 * kChEncDec); m_R = H(P8 * kChSrc);
    const size_t nq = static_cast<size_t>(g.P16()) * (kChY / 4);     // symbols per autoregressive step of ONE picture
    // per picture: nq symbols / indexes / skip flags, the counts of its own blocks, 4 compacted steps and 4 totals
    m_SYM = static_cast<int16_t*>(m_bmem.alloc(N * nq * 2));
    m_COMP = static_cast<int16_t*>(m_bmem.alloc(N * 4 * nq * 2));
    m_COND = static_cast<uint8_t*>(m_bmem.alloc(N * nq / 8 + 8));
    m_IDX = static_cast<uint8_t*>(m_bmem.alloc(N * nq));
    // decode side: step k's compacted indexes of picture b live in their own region (b * 4 + k) [count, int32 | 12 B pad |
    // indexes], so that ONE device->host copy brings the count and (nearly always) all the indexes of a step
    m_idx_region = (16 + nq + 15) / 16 * 16;
    m_CIDX = static_cast<uint8_t*>(m_bmem.alloc(N * 4 * m_idx_region));
    m_DECODED = static_cast<int8_t*>(m_bmem.alloc(N * 4 * nq));
    m_CNT = static_cast<int32_t*>(m_bmem.alloc(sizeof(int32_t) * N * symbol_blocks(static_cast<int>(nq))));
    m_TOTALS = static_cast<int32_t*>(m_bmem.alloc(sizeof(int32_t) * 4 * N));
    m_h_totals.reserve(16 * N);
    m_h_sym.reserve(N * 4 * nq);
    m_h_z.reserve(P64 * kChZ + 64);
    m_h_idx.reserve(N * 4 * m_idx_region);
    m_h_dec.reserve(N * 4 * nq);
    m_g = g;
}

void DmciCodec::select_qp(int qp, hipStream_t st)
{
    copy_qp_rows({{m_cur_q_enc, m_q_enc, kChEncDec}, {m_cur_q_dec, m_q_dec, kChEncDec},
                  {m_cur_q_y_enc, m_q_y_enc, kChY}, {m_cur_q_y_dec, m_q_y_dec, kChY}}, qp, st);
}

// ------------------------------------------------------------------------------------ networks
void DmciCodec::run_encoder(hipStream_t st)
{
    const BatchGeometry& g = m_g;
    // dmci_proxy.cpp:92-105 (the per-channel q_scale_enc multiply is applied to the rounded
    // output of enc_1 inside its last conv's epilogue)
    // consecutive full-width blocks hand dc.0 over: block i's launch also computes dc.0 of block i+1, across the seam too
    const View f(m_F, kChEncDec, kChEncDec);
    ChainCall enc1, enc2;
    enc1.q_after_last = m_cur_q_enc;
    enc1.after = m_enc1.feeds(m_enc2[0]) ? &m_enc2[0] : nullptr;
    enc2.first_dc0_done = enc1.after != nullptr;
    run_dcb_chain(&m_enc1, 1, View(m_U, kChSrc, kChSrc), f, f, g.H8, g.W8, m_s, st, enc1);
    run_dcb_chain(m_enc2, 6, f, f, f, g.H8, g.W8, m_s, st, enc2);
    ConvKxKDesc d;
    d.x = m_F; d.ldx = kChEncDec; d.w = m_enc_down.w; d.bias = m_enc_down.b; d.zeros = m_zeros;
    d.y = m_Y; d.ldy = kChY; d.in_h = g.H8; d.in_w = g.W8; d.cin = kChEncDec; d.cout = kChY;
    d.ksize = 3; d.stride = 2; d.pad = 1; d.n = g.N;
    conv_kxk(d, st);
}

void DmciCodec::run_hyper_and_priors_enc(hipStream_t st)
{
    const BatchGeometry& g = m_g;
    if (g.padded()) {
        replicate_pad_b(m_Y, kChY, g.H16, g.W16, kChY, g.H16p - g.H16, g.W16p - g.W16, m_Ypad, kChY, g.N, st);
    }
    m_henc0.forward(View(m_Ypad, kChY, kChY), View(m_Z1, kChZ, kChZ), g.H16p, g.W16p, m_s, st);
    m_henc1.forward(View(m_Z1, kChZ, kChZ), View(m_Z2a, kChZ, kChZ), View(m_Z2, kChZ, kChZ), g.H16p, g.W16p,
                    m_zeros, m_s, st);
    m_henc2.forward(View(m_Z2, kChZ, kChZ), View(m_Z3a, kChZ, kChZ), View(m_Z3, kChZ, kChZ), g.H32, g.W32,
                    m_zeros, m_s, st);
    round_z(m_Z3, m_ZH, m_ZI8, g.N * g.P64() * kChZ, st);
    run_priors_from_zhat(st);
}

void DmciCodec::run_priors_from_zhat(hipStream_t st)
{
    const BatchGeometry& g = m_g;
    m_hdec0.forward(View(m_ZH, kChZ, kChZ), View(m_H1a, kChZ, kChZ), View(m_H1, kChZ, kChZ), g.H64, g.W64, m_s, st);
    m_hdec1.forward(View(m_H1, kChZ, kChZ), View(m_H2a, kChZ, kChZ), View(m_H2, kChZ, kChZ), g.H32, g.W32, m_s, st);
    m_hdec2.forward(View(m_H2, kChZ, kChZ), View(m_HP, kChY, kChY), g.H16p, g.W16p, m_s, st);
    const View pf(m_PF, 2 * kChY, 2 * kChY);
    {   // a chain of full-width blocks: each launch also computes dc.0 of the block behind it (DcbW::feeds), and the last
        // one the conv that closes the chain (y_prior_fusion.conv.3 -> params)
        const FinCall fin(m_fus3, m_PARAMSp, 2 * kChY);
        ChainCall fus;
        fus.fin = &fin;
        run_dcb_chain(m_fus, 3, View(m_HP, kChY, kChY), pf, pf, g.H16p, g.W16p, m_s, st, fus);
    }
    if (g.padded()) {
        crop_b(m_PARAMSp, 2 * kChY, g.H16p, g.W16p, m_PARAMS, 2 * kChY, g.H16, g.W16, 2 * kChY, g.N, st);
    }
    {   // y_spatial_prior_reduction -> second half of the adaptor input (free torch.cat)
        Conv1x1Desc d;
        d.x = m_PARAMS; d.ldx = 2 * kChY; d.w = m_reduction.w; d.bias = m_reduction.b;
        d.y = m_CAT + kChY; d.ldy = 2 * kChY; d.pixels = g.N * g.P16(); d.cin = 2 * kChY; d.cout = kChY;
        conv1x1(d, st);
    }
}

void DmciCodec::run_spatial_prior(int k, hipStream_t st)
{
    const BatchGeometry& g = m_g;
    const View ad(m_AD, 2 * kChY, 2 * kChY);
    const FinCall fin(m_sp3, m_SP, 2 * kChY);              // y_spatial_prior.conv.3 closes the chain
    ChainCall adaptor, sp;
    adaptor.after = m_sp_adaptor[k].feeds(m_sp[0]) ? &m_sp[0] : nullptr;
    sp.first_dc0_done = adaptor.after != nullptr;
    sp.fin = &fin;
    run_dcb_chain(&m_sp_adaptor[k], 1, View(m_CAT, 2 * kChY, 2 * kChY), ad, ad, g.H16, g.W16, m_s, st, adaptor);
    run_dcb_chain(m_sp, 3, ad, ad, ad, g.H16, g.W16, m_s, st, sp);
}

void DmciCodec::run_decoder(half_t* x_hat, hipStream_t st)
{
    const BatchGeometry& g = m_g;
    // dmci_proxy.cpp:14-33
    const View d1(m_D1, kChEncDec, kChEncDec);
    const DcbW* after_up = m_dec_up.block.feeds(m_dec1[0]) ? &m_dec1[0] : nullptr;
    m_dec_up.forward(View(m_YHAT, kChY, kChY), View(m_D0, kChEncDec, kChEncDec), d1, g.H16, g.W16, m_s, st, nullptr, nullptr,
                     after_up);
    ChainCall dec1;
    dec1.q_after_last = m_cur_q_dec;
    dec1.first_dc0_done = after_up != nullptr;
    run_dcb_chain(m_dec1, 12, d1, d1, d1, g.H8, g.W8, m_s, st, dec1);
    m_dec2.forward(d1, View(m_R, kChSrc, kChSrc), g.H8, g.W8, m_s, st);
    shuffle8_b(m_R, kChSrc, g.H8, g.W8, 3, true, x_hat, g.N, st);
}

void DmciCodec::enc_stage0(hipStream_t st)
{
    const BatchGeometry& g = m_g;
    run_encoder(st);
    run_hyper_and_priors_enc(st);
    mul_channel(m_Y, kChY, m_cur_q_y_enc, m_Y, kChY, g.N * g.P16(), kChY, st);
    const int nq = g.P16() * (kChY / 4);
    for (int k = 0; k < 4; ++k) {
        const half_t* prm = k == 0 ? m_PARAMS : m_SP;
        YStepEnc d;
        d.y = m_Y; d.ldy = kChY;
        d.scales = prm; d.lds = 2 * kChY;
        d.means = prm + kChY; d.ldm = 2 * kChY;
        d.y_hat_acc = m_CAT; d.ldacc = 2 * kChY;
        d.sym = m_SYM; d.cond = m_COND; d.block_count = m_CNT;
        d.H = g.H16; d.W = g.W16; d.C = kChY; d.step = k; d.skip_thres = m_skip_thres; d.first = (k == 0); d.n = g.N;
        y_step_enc(d, st);
        // picture b: its four steps in m_COMP + b * 4 nq, its totals in m_TOTALS[b * 4 ..]
        compact_b(m_SYM, 2, m_COND, m_CNT, nq, m_COMP, 4LL * nq, m_TOTALS, 4, k, g.N, st);
        if (k < 3) run_spatial_prior(k, st);
    }
    // (y_hat_so_far + y_hat_3) * q_scale_y_dec  (add_and_multiply_broadcast, stream.cu:8-38)
    mul_channel(m_CAT, 2 * kChY, m_cur_q_y_dec, m_YHAT, kChY, g.N * g.P16(), kChY, st);
}

// ------------------------------------------------------------------------------------ compress
int DmciCodec::compress(const half_t* x, int height, int width, int qp, half_t* x_hat, hipStream_t user)
{
    compress_impl(1, x, height, width, qp, x_hat, user);
    return m_ec_parallel;
}

void DmciCodec::compress_batch(int n, const half_t* x, int height, int width, int qp, half_t* x_hat, int* ec_parallel_out,
                               hipStream_t user)
{
    compress_impl(n, x, height, width, qp, x_hat, user);
    for (int i = 0; i < n; ++i) ec_parallel_out[i] = i == 0 ? m_ec_parallel : m_ec_parallels[i];
}

const std::vector<uint8_t>& DmciCodec::stream_at(int i) const
{
    if (i < 0 || i >= m_last_n) throw std::invalid_argument("DMCI: no stream " + std::to_string(i) + " in the last call");
    return i == 0 ? stream_bytes() : m_streams[i];
}

void DmciCodec::compress_impl(int n, const half_t* x, int height, int width, int qp, half_t* x_hat, hipStream_t user)
{
    m_last_n = 0;
    prepare(height, width, n);
    hipStream_t st = enter(user);
    select_qp(qp, st);
    pad_unshuffle8_b(x, height, width, 3, m_U, m_g.H8, m_g.W8, n, st);   // outside the graph: x varies
    run_stage(kEnc0, st, [&] { enc_stage0(st); });
    submit(st, [this, qp] { entropy_encode(qp); });
    // the reconstruction runs on the GPU while the worker thread entropy-codes on the host
    bind_stage_arg(kEnc1, x_hat);
    run_stage(kEnc1, st, [&] { run_decoder(x_hat, st); });
    leave(user);
    wait_job();
    m_last_n = n;
}

// ------------------------------------------------------------------------------------ size probe
void DmciCodec::estimate_bits(int n, const half_t* x, int height, int width, int qp, int64_t* units, int64_t* kept,
                              hipStream_t user)
{
    if (qp < 0 || qp >= kQpNum) throw std::invalid_argument("DMCI estimate_bits: qp must be in [0, 63]");
    prepare(height, width, n);
    const BatchGeometry& g = m_g;
    hipStream_t st = enter(user);
    select_qp(qp, st);
    pad_unshuffle8_b(x, height, width, 3, m_U, g.H8, g.W8, n, st);
    run_stage(kEnc0, st, [&] { enc_stage0(st); });          // the graph compress() replays; nothing below is part of it
    const long long nq = static_cast<long long>(g.P16()) * (kChY / 4);
    // picture b: its four compacted steps at m_COMP + b * 4 nq, its four totals at m_TOTALS + 4 b
    probe_code_length(n, m_COMP, 4 * nq, static_cast<int>(4 * nq), m_TOTALS, 4, m_ZI8, g.P64() * kChZ, qp, units, kept, st);
    leave(user);
}

void DmciCodec::entropy_encode(int qp)
{
    // dmci_proxy.cpp:809-845: wait for the symbols, copy them out, code groups 3,2,1,0 then z
    // (a batch: every picture from its own totals, symbols and z into a stream of its own)
    const BatchGeometry& g = m_g;
    static const bool trace = getenv("DCVC_TIMING") != nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    hip_check(hipMemcpyAsync(m_h_totals.get(), m_TOTALS, 4 * g.N * sizeof(int32_t), hipMemcpyDeviceToHost, m_io_stream), "D2H totals");
    const int nz = g.P64() * kChZ;
    const size_t nq = static_cast<size_t>(g.P16()) * (kChY / 4);
    hip_check(hipMemcpyAsync(m_h_z.get(), m_ZI8, static_cast<size_t>(g.N) * nz, hipMemcpyDeviceToHost, m_io_stream), "D2H z");
    hip_check(hipStreamSynchronize(m_io_stream), "sync io");
    bool copied = false;
    for (int b = 0; b < g.N; ++b) {
        int total = 0;
        for (int k = 0; k < 4; ++k) total += m_h_totals[4 * b + k];
        if (total > 0) {
            hip_check(hipMemcpyAsync(m_h_sym.get() + 4 * nq * b, m_COMP + 4 * nq * b, static_cast<size_t>(total) * 2,
                                     hipMemcpyDeviceToHost, m_io_stream), "D2H symbols");
            copied = true;
        }
    }
    if (copied) hip_check(hipStreamSynchronize(m_io_stream), "sync io");
    const auto t_coded = std::chrono::steady_clock::now();
    m_streams.resize(g.N);
    m_ec_parallels.resize(g.N);
    // picture 0 last: its stream stays in m_enc, where a single call leaves it
    for (int b = g.N - 1; b >= 0; --b) {
        const int32_t* totals = m_h_totals.get() + 4 * b;
        const int16_t* sym = m_h_sym.get() + 4 * nq * b;
        int base[4], total = 0;
        for (int k = 0; k < 4; ++k) {
            base[k] = total;
            total += totals[k];
        }
        m_ec_parallel = ec_parallel_for(total);
        m_enc.reset();
        m_enc.set_parallel(m_ec_parallel);
        for (int k = 3; k >= 0; --k) m_enc.push_y(sym + base[k], totals[k]);
        m_enc.push_z(m_h_z.get() + static_cast<size_t>(nz) * b, nz, qp * kChZ, kChZ);
        m_enc.flush();
        m_ec_parallels[b] = m_ec_parallel;
        if (b > 0) m_streams[b] = m_enc.stream();
    }
    if (trace) {
        using us = std::chrono::duration<double, std::micro>;
        fprintf(stderr, "[dcvc] compress host entropy coding of %d pictures %.0f us (waiting for the GPU %.0f us)\n", g.N,
                us(std::chrono::steady_clock::now() - t_coded).count(), us(t_coded - t_call).count());
    }
}

// ------------------------------------------------------------------------------------ decompress
void DmciCodec::decompress(const uint8_t* bits, size_t nbytes, int qp, int height, int width,
                           int ec_parallel, half_t* x_hat, hipStream_t user)
{
    decompress_impl(1, &bits, &nbytes, &ec_parallel, qp, height, width, x_hat, user);
}

void DmciCodec::decompress_batch(int n, const uint8_t* const* bits, const size_t* nbytes, const int* ec_parallel, int qp,
                                 int height, int width, half_t* x_hat, hipStream_t user)
{
    decompress_impl(n, bits, nbytes, ec_parallel, qp, height, width, x_hat, user);
}

void DmciCodec::decompress_impl(int n, const uint8_t* const* bits, const size_t* nbytes, const int* ec_parallel, int qp,
                                int height, int width, half_t* x_hat, hipStream_t user)
{
    prepare(height, width, n);
    const BatchGeometry& g = m_g;
    hipStream_t st = enter(user);
    select_qp(qp, st);
    const int nz = g.P64() * kChZ;
    const int nq = g.P16() * (kChY / 4);
    // DCVC_TIMING: where a decompress() call spends its host time (f3: the entropy decoder's share)
    static const bool trace = getenv("DCVC_TIMING") != nullptr;
    using clk = std::chrono::steady_clock;
    auto us_since = [](clk::time_point t) { return std::chrono::duration<double, std::micro>(clk::now() - t).count(); };
    const auto t_call = clk::now();
    double us_rans = 0, us_wait = 0;
    long n_sym = 0;
    // a batch decodes its pictures' streams in turns on the one decoder: picture b's position waits in m_dec_states[b]
    const bool turns = n > 1;
    if (turns) m_dec_states.resize(n);
    auto t_z = clk::now();
    for (int b = 0; b < n; ++b) {
        m_dec.set_parallel(ec_parallel[b]);
        m_dec.set_stream(bits[b], nbytes[b]);
        m_dec.decode_z(nz, qp * kChZ, kChZ, m_h_z.get() + static_cast<size_t>(nz) * b);
        if (turns) m_dec.swap_state(m_dec_states[b]);
    }
    us_rans += us_since(t_z);
    hip_check(hipMemcpyAsync(m_ZI8, m_h_z.get(), static_cast<size_t>(nz) * n, hipMemcpyHostToDevice, st), "H2D z");

    // step k of picture b: compacted indexes in region b * 4 + k, decoded symbols at m_DECODED + (b * 4 + k) nq
    auto region_of = [&](int b, int k) { return static_cast<size_t>(b * 4 + k) * m_idx_region; };
    auto index_step = [&](int k) {
        YStepDecIndex d;
        d.scales = k == 0 ? m_PARAMS : m_SP; d.lds = 2 * kChY;
        d.index = m_IDX; d.cond = m_COND; d.block_count = m_CNT;
        d.H = g.H16; d.W = g.W16; d.C = kChY; d.step = k; d.skip_thres = m_skip_thres; d.n = n;
        y_step_dec_index(d, st);
        uint8_t* region = m_CIDX + region_of(0, k);
        compact_b(m_IDX, 1, m_COND, m_CNT, nq, region + 16, 4LL * static_cast<long long>(m_idx_region),
                  reinterpret_cast<int32_t*>(region), static_cast<int>(m_idx_region), 0, n, st);
    };
    run_stage(kDec0, st, [&] {
        int8_to_half(m_ZI8, m_ZH, n * nz, st);
        run_priors_from_zhat(st);
        index_step(0);
    });
    bind_stage_arg(kDec1 + 3, x_hat);
    // the first copy of a step takes the count and up to kFirst index bytes (a 1080p step has 50-130 k of its 522 k
    // possible symbols): one copy + one synchronisation per step instead of two of each (the second pair cost
    // ~25 us of GPU idle time per step in the kernel trace)
    static const size_t kFirst = [] { const char* e = getenv("DCVC_IDX_FIRST_KB"); return static_cast<size_t>(e ? atoi(e) : 192) * 1024; }();
    const size_t first = std::min(m_idx_region, 16 + kFirst);
    for (int k = 0; k < 4; ++k) {
        // one GPU -> CPU -> GPU round trip per autoregressive step (dmci_proxy.cpp:857-871), for all pictures at once
        auto t_w = clk::now();
        for (int b = 0; b < n; ++b) {
            hip_check(hipMemcpyAsync(m_h_idx.get() + region_of(b, k), m_CIDX + region_of(b, k), first, hipMemcpyDeviceToHost, st),
                      "D2H count + indexes");
        }
        hip_check(hipStreamSynchronize(st), "sync");
        bool more = false;
        for (int b = 0; b < n; ++b) {
            uint8_t* h_region = m_h_idx.get() + region_of(b, k);
            const int cnt = *reinterpret_cast<const int32_t*>(h_region);
            if (cnt < 0 || cnt > nq) throw std::runtime_error("DMCI decompress: bad symbol count");
            if (16 + static_cast<size_t>(cnt) > first) {
                hip_check(hipMemcpyAsync(h_region + first, m_CIDX + region_of(b, k) + first, 16 + cnt - first,
                                         hipMemcpyDeviceToHost, st), "D2H indexes");
                more = true;
            }
        }
        if (more) hip_check(hipStreamSynchronize(st), "sync");
        us_wait += us_since(t_w);
        for (int b = 0; b < n; ++b) {
            const uint8_t* h_region = m_h_idx.get() + region_of(b, k);
            const int cnt = *reinterpret_cast<const int32_t*>(h_region);
            if (cnt == 0) continue;
            const size_t at = static_cast<size_t>(b * 4 + k) * nq;
            auto t_r = clk::now();
            if (turns) m_dec.swap_state(m_dec_states[b]);
            m_dec.decode_y(h_region + 16, cnt, m_h_dec.get() + at);
            if (turns) m_dec.swap_state(m_dec_states[b]);
            us_rans += us_since(t_r);
            n_sym += cnt;
            hip_check(hipMemcpyAsync(m_DECODED + at, m_h_dec.get() + at, cnt, hipMemcpyHostToDevice, st), "H2D symbols");
        }
        run_stage(kDec1 + k, st, [&] {
            YStepDecRestore d;
            d.decoded = m_DECODED + static_cast<size_t>(k) * nq; d.cond = m_COND; d.block_count = m_CNT;
            d.totals = reinterpret_cast<const int32_t*>(m_CIDX + region_of(0, k));
            d.slot = 0;                                        // the step's own region: no base to add up
            // picture b: symbols 4 nq further, totals four regions (m_idx_region int32s) further
            d.n = n; d.decoded_stride = 4LL * nq; d.totals_stride = static_cast<int>(m_idx_region);
            d.means = (k == 0 ? m_PARAMS : m_SP) + kChY; d.ldm = 2 * kChY;
            d.y_hat_acc = m_CAT; d.ldacc = 2 * kChY;
            d.H = g.H16; d.W = g.W16; d.C = kChY; d.step = k; d.first = (k == 0);
            y_step_dec_restore(d, st);
            if (k < 3) {
                run_spatial_prior(k, st);
                index_step(k + 1);
            } else {
                mul_channel(m_CAT, 2 * kChY, m_cur_q_y_dec, m_YHAT, kChY, n * g.P16(), kChY, st);
                run_decoder(x_hat, st);
            }
        });
    }
    if (trace) {
        size_t bytes = 0;
        for (int b = 0; b < n; ++b) bytes += nbytes[b];
        fprintf(stderr, "[dcvc] decompress host %.0f us: entropy decoding %.0f us (%ld y symbols, %zu bytes, %d streams, "
                        "%d pictures), waiting for the GPU %.0f us\n", us_since(t_call), us_rans, n_sym, bytes, ec_parallel[0],
                n, us_wait);
    }
    leave(user);
}

// ------------------------------------------------------------------------------------ debug
size_t DmciCodec::debug_read(const std::string& name, void* dst, size_t cap, hipStream_t st)
{
    const BatchGeometry& g = m_g;
    const void* src = nullptr;
    size_t bytes = 0;
    if (name == "y") { src = m_Y; bytes = static_cast<size_t>(g.N) * g.P16() * kChY * 2; }
    else if (name == "y_hat") { src = m_YHAT; bytes = static_cast<size_t>(g.N) * g.P16() * kChY * 2; }
    else if (name == "z_i8") { src = m_ZI8; bytes = static_cast<size_t>(g.N) * g.P64() * kChZ; }
    else if (name == "params") { src = m_PARAMS; bytes = static_cast<size_t>(g.N) * g.P16() * 2 * kChY * 2; }
    else if (name == "unshuffled") { src = m_U; bytes = static_cast<size_t>(g.N) * g.P8() * kChSrc * 2; }
    else if (name == "features") { src = m_F; bytes = static_cast<size_t>(g.N) * g.P8() * kChEncDec * 2; }
    else if (name == "totals") { src = m_TOTALS; bytes = 16 * static_cast<size_t>(g.N); }
    else if (name == "symbols") { src = m_COMP; bytes = static_cast<size_t>(g.N) * g.P16() * kChY * 2; }
    else throw std::invalid_argument("unknown debug tensor '" + name + "'");
    if (dst != nullptr) {
        hip_check(hipStreamSynchronize(st), "sync");
        hip_check(hipStreamSynchronize(m_cs), "sync");
        hip_check(hipMemcpy(dst, src, std::min(bytes, cap), hipMemcpyDeviceToHost), "debug D2H");
    }
    return bytes;
}

}  // namespace dcvc
