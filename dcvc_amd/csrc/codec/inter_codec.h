// What the inter codecs (LD, HT-S, HT-L) share around their networks: the parameter and per-resolution arenas, the per-qp
// scale tables, the symbol staging buffers, the validity flags of the temporal state with their transitions and refusals,
// the host entropy-coding job, the decoder's round trip to the host, the state hand-off format and debug_read.
// A plain base class with protected helpers: the derived classes keep their public methods, their networks and the call
// order of compress / decompress in their own files.
//
// Reference counterpart: the parts that dmc_ld_proxy.cpp, dmc_hts_proxy.cpp and dmc_htl_proxy.cpp each write out again.
#pragma once

#include "codec/codec_base.h"

#include <initializer_list>
#include <string>
#include <vector>

namespace dcvc {

class InterCodec : public CodecBase {
public:
    static constexpr int kChZ = 128;      // video_model_ld.py:18, video_model_ht.py:20

protected:
    explicit InterCodec(const char* name);      // "DMC-LD" / "DMC-HT": the name in messages
    // Waits for everything in flight before the arenas below go away. The derived classes own no device memory (their
    // weight structs are views into m_wmem, their buffer pointers views into m_bmem), so their members may be destroyed
    // before this runs: what is still in flight - kernels, the worker's entropy_encode - touches only members of this class
    // and of CodecBase.
    ~InterCodec();

    // ---- validity of the temporal state
    struct TemporalFlags {
        bool has_ref = false;            // the reference feature is valid
        bool enc_ready = false;          // memory, ctx (LD: and the temporal prior) are those of the next unit to encode
        bool memory_has_value = false;   // decoder: the next unit extends the memory (else restarts from the reference feature)
        bool has_feature_p = false;
        uint32_t pack() const { return (has_ref ? 1u : 0u) | (enc_ready ? 2u : 0u) | (memory_has_value ? 4u : 0u) | (has_feature_p ? 8u : 0u); }
        void unpack(uint32_t f) { has_ref = f & 1u; enc_ready = f & 2u; memory_has_value = f & 4u; has_feature_p = f & 8u; }
        void clear() { unpack(0); }
        void after_add_ref(bool apply_adaptor) { has_ref = true; enc_ready = memory_has_value = apply_adaptor; has_feature_p = false; }
        void after_compress() { has_feature_p = true; }
        // the last head output is the reference feature after a reset; the encoder side must be re-seeded
        void after_decompress(bool reset) { has_feature_p = has_ref = true; memory_has_value = !reset; enc_ready = false; }
    };
    void require_encoder_ready(const char* what) const;      // compress / estimate_bits
    void require_decoder_ready() const;
    // reconstruct: parameters and a feature_p (compress, decompress or import_state of such a state left it)
    void require_feature_p(const char* what) const;
    // estimate_bits: qp, encoder-side state, picture size. Every refusal comes before anything is touched: prepare() with
    // another size would drop the temporal state.
    void check_probe(int qp, int height, int width) const;

    // ---- set_param: head (quiesce, weight memory released, the q tables: q_encoder / q_decoder ch_d wide, q_feature
    // ch_feature wide, m_zeros) and tail (CDF and code-length tables, flags cleared)
    void begin_set_param(const ParamStore& ps, float skip_thres, int ch_d, int ch_feature);
    void finish_set_param(const ParamStore& ps);
    void select_qp(int qp, hipStream_t st);

    // ---- prepare: checks, m_g; false when the size is the one the buffers have (else: quiesced, graphs and buffers dropped)
    bool begin_prepare(int height, int width);
    // symbols, skip flags, indexes, decoded symbols, block counts, totals + their pinned mirrors for n_symbols symbols;
    // the decode side's compacted indexes as idx_regions regions of idx_region_bytes
    void alloc_symbol_buffers(size_t n_symbols, int idx_regions, size_t idx_region_bytes);

    // ---- host side of the entropy stage
    // worker thread: `groups` compacted symbol groups back to back in m_COMP with their totals, then z
    void entropy_encode(int qp, int groups);
    // decoder, one round trip around a stage that does not need y: the symbol count, then the compacted indexes on their way
    // to the host (m_ev_idx) -> caller's stage -> decode y, decoded symbols on their way to the device
    int fetch_total_and_indexes(hipStream_t st);
    void decode_y_and_upload(int n, hipStream_t st);

    // ---- state hand-off: 64-byte header (magic, H8, W8, flags), then every part dense
    struct StatePart {
        half_t* p;
        int channels, ld;
        size_t pixels;
    };
    size_t export_state(uint32_t magic, const std::vector<StatePart>& parts, void* dst, size_t cap, hipStream_t user);
    // behind the derived prepare(); wrong_state: the message for another magic or size in the header
    void import_state(uint32_t magic, const char* wrong_state, const std::vector<StatePart>& parts, const void* src,
                      size_t bytes, hipStream_t user);

    struct DebugView {
        const char* name;
        const void* p;
        size_t pixels;
        int channels, ld, elem;
    };
    size_t debug_read(std::initializer_list<DebugView> views, const std::string& name, void* dst, size_t cap, hipStream_t st);

    const std::string m_name;
    // ---- parameters
    DeviceArena m_wmem;
    const half_t *m_q_encoder = nullptr, *m_q_decoder = nullptr, *m_q_feature = nullptr;
    half_t *m_cur_q_encoder = nullptr, *m_cur_q_decoder = nullptr, *m_cur_q_feature = nullptr;
    int m_q_ch_d = 0, m_q_ch_feature = 0;
    half_t* m_zeros = nullptr;
    float m_skip_thres = 0.f;
    bool m_has_params = false;

    // ---- per resolution
    Geometry m_g;
    DeviceArena m_bmem;
    Scratch m_s;
    int8_t* m_ZI8 = nullptr;          // [P64][kChZ], allocated by the derived prepare() among its z buffers
    int16_t *m_SYM = nullptr, *m_COMP = nullptr;
    uint8_t *m_COND = nullptr, *m_IDX = nullptr, *m_CIDX = nullptr;
    int8_t *m_DECODED = nullptr, *m_YQ = nullptr;
    int32_t *m_CNT = nullptr, *m_TOTALS = nullptr;
    Pinned<int32_t> m_h_totals;
    Pinned<int16_t> m_h_sym;
    Pinned<int8_t> m_h_z;
    Pinned<uint8_t> m_h_idx;
    Pinned<int8_t> m_h_dec;
    hipEvent_t m_ev_idx = nullptr;
    int m_ec_parallel = 1;

    TemporalFlags m_flags;
};

}  // namespace dcvc
