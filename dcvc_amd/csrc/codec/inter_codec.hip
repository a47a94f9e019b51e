// Host scaffolding of the inter codecs (see inter_codec.h). No network code here.
#include "codec/inter_codec.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace dcvc {

InterCodec::InterCodec(const char* name) : m_name(name)
{
    hip_check(hipEventCreateWithFlags(&m_ev_idx, hipEventDisableTiming), "hipEventCreate");
}

InterCodec::~InterCodec()
{
    quiesce();
    if (m_ev_idx) (void)hipEventDestroy(m_ev_idx);
}

// ------------------------------------------------------------------------------------ temporal state
void InterCodec::require_encoder_ready(const char* what) const
{
    if (!m_has_params || !m_flags.enc_ready) {
        throw std::runtime_error(m_name + " " + what + ": no reference feature "
                                 "(call add_ref_feature_from_frame(frame, true) first)");
    }
}

void InterCodec::require_decoder_ready() const
{
    if (m_flags.memory_has_value ? !m_flags.has_feature_p : !m_flags.has_ref) {
        throw std::runtime_error(m_name + " decompress: no reference feature "
                                 "(call add_ref_feature_from_frame first)");
    }
}

void InterCodec::require_feature_p(const char* what) const
{
    if (!m_has_params) throw std::runtime_error(m_name + " " + what + ": set_param() has not been called");
    if (m_g.H8 == 0 || !m_flags.has_feature_p) {
        throw std::runtime_error(m_name + " " + what + ": no feature_p yet (compress, decompress or import_state first)");
    }
}

void InterCodec::check_probe(int qp, int height, int width) const
{
    if (qp < 0 || qp >= kQpNum) throw std::invalid_argument(m_name + " estimate_bits: qp must be in [0, 63]");
    require_encoder_ready("estimate_bits");
    if (height <= 0 || width <= 0 || ceil_div(height, 16) * 2 != m_g.H8 || ceil_div(width, 16) * 2 != m_g.W8) {
        throw std::invalid_argument(m_name + " estimate_bits: the picture size is not the one of the temporal state");
    }
}

// ------------------------------------------------------------------------------------ set_param
void InterCodec::begin_set_param(const ParamStore& ps, float skip_thres, int ch_d, int ch_feature)
{
    quiesce();
    clear_graphs();
    m_wmem.release();
    kernels_init();
    m_skip_thres = skip_thres;
    m_q_ch_d = ch_d;
    m_q_ch_feature = ch_feature;
    m_q_encoder = upload_qp_table(ps, m_wmem, "q_encoder", ch_d);
    m_q_decoder = upload_qp_table(ps, m_wmem, "q_decoder", ch_d);
    m_q_feature = upload_qp_table(ps, m_wmem, "q_feature", ch_feature);
    m_cur_q_encoder = m_wmem.alloc_half(ch_d);
    m_cur_q_decoder = m_wmem.alloc_half(ch_d);
    m_cur_q_feature = m_wmem.alloc_half(ch_feature);
    m_zeros = m_wmem.alloc_half(2048);
}

void InterCodec::finish_set_param(const ParamStore& ps)
{
    load_cdf_tables(ps);
    upload_code_length_tables(ps, m_wmem, kChZ, 1);      // for estimate_bits
    m_has_params = true;
    m_flags.clear();
}

void InterCodec::select_qp(int qp, hipStream_t st)
{
    copy_qp_rows({{m_cur_q_encoder, m_q_encoder, m_q_ch_d}, {m_cur_q_decoder, m_q_decoder, m_q_ch_d},
                  {m_cur_q_feature, m_q_feature, m_q_ch_feature}}, qp, st);
}

// ------------------------------------------------------------------------------------ buffers
bool InterCodec::begin_prepare(int height, int width)
{
    if (!m_has_params) throw std::runtime_error(m_name + ": set_param() has not been called");
    if (height <= 0 || width <= 0) throw std::invalid_argument(m_name + ": empty picture");
    const Geometry g = Geometry::of(height, width);
    if (m_g.H8 == g.H8 && m_g.W8 == g.W8) return false;
    quiesce();
    clear_graphs();
    m_bmem.release();
    m_flags.clear();                    // the state had another size
    m_g = g;
    return true;
}

void InterCodec::alloc_symbol_buffers(size_t n, int idx_regions, size_t idx_region_bytes)
{
    m_SYM = static_cast<int16_t*>(m_bmem.alloc(n * 2));
    m_COMP = static_cast<int16_t*>(m_bmem.alloc(n * 2));
    m_COND = static_cast<uint8_t*>(m_bmem.alloc(n / 8 + 8));
    m_IDX = static_cast<uint8_t*>(m_bmem.alloc(n));
    m_CIDX = static_cast<uint8_t*>(m_bmem.alloc(idx_regions * idx_region_bytes));
    m_DECODED = static_cast<int8_t*>(m_bmem.alloc(n));
    m_YQ = static_cast<int8_t*>(m_bmem.alloc(n));
    m_CNT = static_cast<int32_t*>(m_bmem.alloc(sizeof(int32_t) * symbol_blocks(static_cast<int>(n))));
    m_TOTALS = static_cast<int32_t*>(m_bmem.alloc(sizeof(int32_t) * 4));
    m_h_totals.reserve(16);
    m_h_sym.reserve(n);
    m_h_z.reserve(static_cast<size_t>(m_g.P64()) * kChZ + 64);
    m_h_idx.reserve(idx_regions * idx_region_bytes);
    m_h_dec.reserve(n);
}

// ------------------------------------------------------------------------------------ entropy stage, host side
void InterCodec::entropy_encode(int qp, int groups)
{
    static const bool trace = getenv("DCVC_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (trace) {
            fprintf(stderr, "[dcvc]   %s encode: %s at +%.0f us\n", m_name.c_str(), what,
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
    };
    // the reference's worker, Encode: the y groups last to first, then z
    hip_check(hipMemcpyAsync(m_h_totals.get(), m_TOTALS, groups * sizeof(int32_t), hipMemcpyDeviceToHost, m_io_stream), "D2H totals");
    const int nz = m_g.P64() * kChZ;
    hip_check(hipMemcpyAsync(m_h_z.get(), m_ZI8, nz, hipMemcpyDeviceToHost, m_io_stream), "D2H z");
    hip_check(hipStreamSynchronize(m_io_stream), "sync io");
    int base[4] = { 0, 0, 0, 0 }, total = 0;
    for (int k = 0; k < groups; ++k) {
        base[k] = total;
        total += m_h_totals[k];
    }
    lap("totals + z on the host (GPU stage 0 done)");
    if (total > 0) {
        hip_check(hipMemcpyAsync(m_h_sym.get(), m_COMP, static_cast<size_t>(total) * 2, hipMemcpyDeviceToHost, m_io_stream), "D2H symbols");
        hip_check(hipStreamSynchronize(m_io_stream), "sync io");
    }
    lap("symbols on the host");
    m_ec_parallel = ec_parallel_for(total);
    m_enc.reset();
    m_enc.set_parallel(m_ec_parallel);
    for (int k = groups - 1; k >= 0; --k) m_enc.push_y(m_h_sym.get() + base[k], m_h_totals[k]);
    m_enc.push_z(m_h_z.get(), nz, qp * kChZ, kChZ);
    m_enc.flush();
    lap("rANS done");
}

// (one copy for count + indexes in front of the stage between the two halves was measured SLOWER - LD 300 -> 271,
// HT-S 570 -> 541 pictures/s: the 192 KB copy sits in the stream in front of the context network's kernels; the two small
// copies with a synchronisation in between do not hold them up)
int InterCodec::fetch_total_and_indexes(hipStream_t st)
{
    hip_check(hipMemcpyAsync(m_h_totals.get(), m_TOTALS, sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H totals");
    hip_check(hipStreamSynchronize(st), "sync");
    const int n = m_h_totals[0];
    if (n > 0) {
        hip_check(hipMemcpyAsync(m_h_idx.get(), m_CIDX, n, hipMemcpyDeviceToHost, st), "D2H indexes");
        hip_check(hipEventRecord(m_ev_idx, st), "hipEventRecord");
    }
    return n;
}

void InterCodec::decode_y_and_upload(int n, hipStream_t st)
{
    if (n > 0) {
        hip_check(hipEventSynchronize(m_ev_idx), "hipEventSynchronize");
        m_dec.decode_y(m_h_idx.get(), n, m_h_dec.get());
        hip_check(hipMemcpyAsync(m_DECODED, m_h_dec.get(), n, hipMemcpyHostToDevice, st), "H2D symbols");
    }
}

// ------------------------------------------------------------------------------------ state hand-off
namespace {

struct StateHeader {
    uint32_t magic, h8, w8, flags;
    uint32_t reserved[12];
};

// rows of `width` bytes; a channel slice of a wider buffer (pitch > width) becomes dense and the other way round
void copy_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t st)
{
    if (dpitch == width && spitch == width) {
        hip_check(hipMemcpyAsync(dst, src, width * rows, hipMemcpyDeviceToDevice, st), "state D2D");
    } else {
        hip_check(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, hipMemcpyDeviceToDevice, st), "state D2D");
    }
}

}  // namespace

size_t InterCodec::export_state(uint32_t magic, const std::vector<StatePart>& parts, void* dst, size_t cap, hipStream_t user)
{
    if (!m_has_params || m_g.H8 == 0) throw std::runtime_error(m_name + " export_state: no state yet");
    size_t bytes = sizeof(StateHeader);
    for (const StatePart& s : parts) bytes += 2 * s.pixels * s.channels;
    if (dst == nullptr) return bytes;
    if (cap < bytes) throw std::invalid_argument("export_state: destination too small");
    hipStream_t st = enter(user);
    StateHeader h{};
    h.magic = magic; h.h8 = m_g.H8; h.w8 = m_g.W8;
    h.flags = m_flags.pack();
    char* out = static_cast<char*>(dst);
    hip_check(hipMemcpyAsync(out, &h, sizeof(h), hipMemcpyHostToDevice, st), "state header");
    hip_check(hipStreamSynchronize(st), "sync");          // the header lives on this stack frame
    out += sizeof(h);
    for (const StatePart& s : parts) {
        copy_rows(out, 2 * s.channels, s.p, 2 * s.ld, 2 * s.channels, s.pixels, st);
        out += 2 * s.pixels * s.channels;
    }
    leave(user);
    return bytes;
}

void InterCodec::import_state(uint32_t magic, const char* wrong_state, const std::vector<StatePart>& parts, const void* src,
                              size_t bytes, hipStream_t user)
{
    size_t want = sizeof(StateHeader);
    for (const StatePart& s : parts) want += 2 * s.pixels * s.channels;
    if (bytes != want) throw std::invalid_argument("import_state: size does not match this picture size");
    hipStream_t st = enter(user);
    StateHeader h{};
    const char* in = static_cast<const char*>(src);
    hip_check(hipMemcpyAsync(&h, in, sizeof(h), hipMemcpyDeviceToHost, st), "state header");
    hip_check(hipStreamSynchronize(st), "sync");
    if (h.magic != magic || h.h8 != static_cast<uint32_t>(m_g.H8) || h.w8 != static_cast<uint32_t>(m_g.W8)) {
        throw std::invalid_argument(wrong_state);
    }
    in += sizeof(h);
    for (const StatePart& s : parts) {
        copy_rows(s.p, 2 * s.ld, in, 2 * s.channels, 2 * s.channels, s.pixels, st);
        in += 2 * s.pixels * s.channels;
    }
    leave(user);
    m_flags.unpack(h.flags);
}

// ------------------------------------------------------------------------------------ debug
size_t InterCodec::debug_read(std::initializer_list<DebugView> views, const std::string& name, void* dst, size_t cap, hipStream_t st)
{
    const DebugView* v = nullptr;
    for (const DebugView& c : views) {
        if (name == c.name) v = &c;
    }
    if (v == nullptr) throw std::invalid_argument("unknown debug tensor '" + name + "'");
    const size_t ch_bytes = static_cast<size_t>(v->channels) * v->elem, pitch = static_cast<size_t>(v->ld) * v->elem;
    const size_t bytes = v->pixels * ch_bytes;
    if (dst != nullptr) {
        if (cap < bytes) throw std::invalid_argument("debug_read: destination too small");
        hip_check(hipStreamSynchronize(st), "sync");
        hip_check(hipStreamSynchronize(m_cs), "sync");
        hip_check(hipMemcpy2D(dst, ch_bytes, v->p, pitch, ch_bytes, v->pixels, hipMemcpyDeviceToHost), "debug D2H");
    }
    return bytes;
}

}  // namespace dcvc
