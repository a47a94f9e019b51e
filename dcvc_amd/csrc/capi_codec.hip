// C ABI of the picture codecs (include/dcvc_amd_codec.h).
#include "capi_common.h"
#include "codec/dmc_ht.h"
#include "codec/dmc_ld.h"
#include "codec/dmci.h"
#include "dcvc_amd_codec.h"
#include "kernels/arith.h"

#include <cstring>
#include <string>

struct dcvc_dmci {
    dcvc::DmciCodec codec;
    int64_t est_kept[dcvc::DmciCodec::kMaxBatch] = {};      // y symbols of the pictures of the last size probe
    int est_n = 0;
};

struct dcvc_dmcld {
    dcvc::DmcLdCodec codec;
    int64_t est_kept = -1;      // y symbols of the last size probe
};

struct dcvc_dmcht {
    explicit dcvc_dmcht(bool is_hts) : codec(is_hts) {}
    dcvc::DmcHtCodec codec;
    int64_t est_kept = -1;
};

namespace {

dcvc::ParamStore make_store(int n, const char* const* names, const void* const* data, const int* dtypes,
                            const int* ndims, const int64_t* dims)
{
    dcvc::ParamStore ps;
    const int64_t* d = dims;
    for (int i = 0; i < n; ++i) {
        ps.add(names[i], data[i], dtypes[i], d, ndims[i]);
        d += ndims[i];
    }
    return ps;
}

void check_padding16(int height, int width, int padding_b, int padding_r)
{
    const int pb = (height + 15) / 16 * 16 - height, pr = (width + 15) / 16 * 16 - width;
    if (padding_b != pb || padding_r != pr) {
        throw std::invalid_argument("compress: padding must extend the picture to multiples of 16");
    }
}

void check_batch(const dcvc_dmci* c, int n)
{
    if (c == nullptr) throw std::invalid_argument("null codec");
    if (n < 1 || n > dcvc::DmciCodec::kMaxBatch) throw std::invalid_argument("batch size must be in [1, 16]");
}

// ---- the operations the handle types share (each handle has a `codec`; the inter handles also `est_kept`)
hipStream_t hip_stream(void* stream) { return static_cast<hipStream_t>(stream); }

// a call that returns a size: the size, or the negative error code
template <typename F>
int64_t guarded_size(F&& fn)
{
    int64_t n = -1;
    const int rc = dcvc::guarded([&] { n = static_cast<int64_t>(fn()); });
    return rc < 0 ? rc : n;
}

template <typename H>
int set_param(H* c, int n, const char* const* names, const void* const* data, const int* dtypes, const int* ndims,
              const int64_t* dims, float skip_thres)
{
    return dcvc::guarded([&] { c->codec.set_param(make_store(n, names, data, dtypes, ndims, dims), skip_thres); });
}

template <typename H>
int64_t get_stream(H* c, uint8_t* dst, size_t cap)
{
    const auto& s = c->codec.stream_bytes();
    if (dst != nullptr) std::memcpy(dst, s.data(), s.size() < cap ? s.size() : cap);
    return static_cast<int64_t>(s.size());
}

template <typename H>
int set_use_graphs(H* c, int on)
{
    return dcvc::guarded([&] { c->codec.set_use_graphs(on != 0); });
}

template <typename H>
int64_t debug_read(H* c, const char* name, void* dst, size_t cap, void* stream)
{
    return guarded_size([&] { return c->codec.debug_read(name, dst, cap, hip_stream(stream)); });
}

template <typename H>
int add_ref(H* c, const void* frame, int height, int width, int apply_adaptor, void* stream)
{
    return dcvc::guarded([&] {
        c->codec.add_ref_feature_from_frame(static_cast<const dcvc::half_t*>(frame), height, width, apply_adaptor != 0,
                                            hip_stream(stream));
    });
}

template <typename H>
int compress(H* c, const void* x, int height, int width, int qp, int reset_feature_memory, int padding_b, int padding_r,
             void* stream)
{
    int ec = -1;
    const int rc = dcvc::guarded([&] {
        check_padding16(height, width, padding_b, padding_r);
        ec = c->codec.compress(static_cast<const dcvc::half_t*>(x), height, width, qp, reset_feature_memory != 0,
                               hip_stream(stream));
    });
    return rc < 0 ? rc : ec;
}

template <typename H>
int decompress(H* c, const uint8_t* bit_stream, size_t nbytes, int qp, int height, int width, int ec_parallel,
               int reset_feature_memory, void* x_hat, void* stream)
{
    return dcvc::guarded([&] {
        c->codec.decompress(bit_stream, nbytes, qp, height, width, ec_parallel, reset_feature_memory != 0,
                            static_cast<dcvc::half_t*>(x_hat), hip_stream(stream));
    });
}

template <typename H>
int estimate_bits(H* c, const void* x, int height, int width, int qp, int padding_b, int padding_r, int64_t* out_units,
                  void* stream)
{
    return dcvc::guarded([&] {
        if (c == nullptr || x == nullptr || out_units == nullptr) throw std::invalid_argument("estimate_bits: null codec, picture or result pointer");
        check_padding16(height, width, padding_b, padding_r);
        c->est_kept = -1;
        int64_t kept = 0;
        c->codec.estimate_bits(static_cast<const dcvc::half_t*>(x), height, width, qp, out_units, &kept, hip_stream(stream));
        c->est_kept = kept;
    });
}

template <typename H>
int64_t estimate_symbols(H* c)
{
    return guarded_size([&] {
        if (c == nullptr || c->est_kept < 0) throw std::invalid_argument("estimate_symbols: no size probe yet");
        return c->est_kept;
    });
}

template <typename H>
int reconstruct(H* c, const char* entry, void* x_hat, void* stream)
{
    return dcvc::guarded([&] {
        if (c == nullptr || x_hat == nullptr) throw std::invalid_argument(std::string(entry) + ": null codec or x_hat pointer");
        c->codec.reconstruct(static_cast<dcvc::half_t*>(x_hat), hip_stream(stream));
    });
}

template <typename H>
int64_t export_state(H* c, void* dst, size_t cap, void* stream)
{
    return guarded_size([&] { return c->codec.export_state(dst, cap, hip_stream(stream)); });
}

template <typename H>
int import_state(H* c, const void* src, size_t bytes, int height, int width, void* stream)
{
    return dcvc::guarded([&] { c->codec.import_state(src, bytes, height, width, hip_stream(stream)); });
}

}  // namespace

extern "C" {

int dcvc_arith_policy_version(void) { return dcvc::kArithPolicyVersion; }

dcvc_dmci* dcvc_dmci_create(void)
{
    dcvc_dmci* c = nullptr;
    dcvc::guarded([&] { c = new dcvc_dmci(); });
    return c;
}

void dcvc_dmci_destroy(dcvc_dmci* c)
{
    delete c;
}

int dcvc_dmci_set_param(dcvc_dmci* c, int n, const char* const* names, const void* const* data,
                        const int* dtypes, const int* ndims, const int64_t* dims, float skip_thres)
{
    return set_param(c, n, names, data, dtypes, ndims, dims, skip_thres);
}

int dcvc_dmci_compress(dcvc_dmci* c, const void* x, int height, int width, int qp, int padding_b,
                       int padding_r, void* x_hat, void* stream)
{
    int ec = -1;
    const int rc = dcvc::guarded([&] {
        check_padding16(height, width, padding_b, padding_r);
        ec = c->codec.compress(static_cast<const dcvc::half_t*>(x), height, width, qp,
                               static_cast<dcvc::half_t*>(x_hat), static_cast<hipStream_t>(stream));
    });
    return rc < 0 ? rc : ec;
}

int64_t dcvc_dmci_get_stream(dcvc_dmci* c, uint8_t* dst, size_t cap) { return get_stream(c, dst, cap); }

int dcvc_dmci_decompress(dcvc_dmci* c, const uint8_t* bit_stream, size_t nbytes, int qp, int height,
                         int width, int ec_parallel, void* x_hat, void* stream)
{
    return dcvc::guarded([&] {
        c->codec.decompress(bit_stream, nbytes, qp, height, width, ec_parallel,
                            static_cast<dcvc::half_t*>(x_hat), static_cast<hipStream_t>(stream));
    });
}

int dcvc_dmci_compress_batch(dcvc_dmci* c, int n, const void* x, int height, int width, int qp, int padding_b,
                             int padding_r, void* x_hat, int* ec_parallel_out, void* stream)
{
    return dcvc::guarded([&] {
        check_batch(c, n);
        if (x == nullptr || x_hat == nullptr || ec_parallel_out == nullptr) {
            throw std::invalid_argument("compress_batch: null picture, reconstruction or ec_parallel pointer");
        }
        check_padding16(height, width, padding_b, padding_r);
        c->codec.compress_batch(n, static_cast<const dcvc::half_t*>(x), height, width, qp, static_cast<dcvc::half_t*>(x_hat),
                                ec_parallel_out, static_cast<hipStream_t>(stream));
    });
}

int64_t dcvc_dmci_get_stream_at(dcvc_dmci* c, int i, uint8_t* dst, size_t cap)
{
    return guarded_size([&] {
        if (c == nullptr) throw std::invalid_argument("get_stream_at: null codec");
        const auto& s = c->codec.stream_at(i);
        if (dst != nullptr) std::memcpy(dst, s.data(), s.size() < cap ? s.size() : cap);
        return s.size();
    });
}

int dcvc_dmci_decompress_batch(dcvc_dmci* c, int n, const uint8_t* const* streams, const size_t* nbytes,
                               const int* ec_parallel, int qp, int height, int width, void* x_hat, void* stream)
{
    return dcvc::guarded([&] {
        check_batch(c, n);
        if (streams == nullptr || nbytes == nullptr || ec_parallel == nullptr || x_hat == nullptr) {
            throw std::invalid_argument("decompress_batch: null stream list, sizes, ec_parallel or reconstruction pointer");
        }
        for (int i = 0; i < n; ++i) {
            if (streams[i] == nullptr && nbytes[i] > 0) throw std::invalid_argument("decompress_batch: null stream");
            if (ec_parallel[i] < 1 || ec_parallel[i] > dcvc::kMaxEcParallel) {
                throw std::invalid_argument("decompress_batch: ec_parallel must be in [1, 8]");
            }
        }
        c->codec.decompress_batch(n, streams, nbytes, ec_parallel, qp, height, width, static_cast<dcvc::half_t*>(x_hat),
                                  static_cast<hipStream_t>(stream));
    });
}

int dcvc_dmci_estimate_bits_batch(dcvc_dmci* c, int n, const void* x, int height, int width, int qp, int padding_b,
                                  int padding_r, int64_t* out_units, void* stream)
{
    return dcvc::guarded([&] {
        check_batch(c, n);
        if (x == nullptr || out_units == nullptr) throw std::invalid_argument("estimate_bits: null picture or result pointer");
        check_padding16(height, width, padding_b, padding_r);
        c->est_n = 0;
        c->codec.estimate_bits(n, static_cast<const dcvc::half_t*>(x), height, width, qp, out_units, c->est_kept,
                               static_cast<hipStream_t>(stream));
        c->est_n = n;
    });
}

int dcvc_dmci_estimate_bits(dcvc_dmci* c, const void* x, int height, int width, int qp, int padding_b, int padding_r,
                            int64_t* out_units, void* stream)
{
    return dcvc_dmci_estimate_bits_batch(c, 1, x, height, width, qp, padding_b, padding_r, out_units, stream);
}

int64_t dcvc_dmci_estimate_symbols(dcvc_dmci* c, int i)
{
    return guarded_size([&] {
        if (c == nullptr || i < 0 || i >= c->est_n) throw std::invalid_argument("estimate_symbols: no such picture in the last size probe");
        return c->est_kept[i];
    });
}

int dcvc_ec_parallel_for(int64_t symbols)
{
    return dcvc::ec_parallel_for(symbols > 0x7fffffff ? 0x7fffffff : static_cast<int>(symbols < 0 ? 0 : symbols));
}

int dcvc_dmci_set_use_graphs(dcvc_dmci* c, int on) { return set_use_graphs(c, on); }

int64_t dcvc_dmci_debug_read(dcvc_dmci* c, const char* name, void* dst, size_t cap, void* stream)
{
    return debug_read(c, name, dst, cap, stream);
}

// ------------------------------------------------------------------------------------ DMC-LD
dcvc_dmcld* dcvc_dmcld_create(void)
{
    dcvc_dmcld* c = nullptr;
    dcvc::guarded([&] { c = new dcvc_dmcld(); });
    return c;
}

void dcvc_dmcld_destroy(dcvc_dmcld* c)
{
    delete c;
}

int dcvc_dmcld_set_param(dcvc_dmcld* c, int n, const char* const* names, const void* const* data,
                         const int* dtypes, const int* ndims, const int64_t* dims, float skip_thres)
{
    return set_param(c, n, names, data, dtypes, ndims, dims, skip_thres);
}

int dcvc_dmcld_add_ref_feature_from_frame(dcvc_dmcld* c, const void* frame, int height, int width,
                                          int apply_adaptor, void* stream)
{
    return add_ref(c, frame, height, width, apply_adaptor, stream);
}

int dcvc_dmcld_compress(dcvc_dmcld* c, const void* x, int height, int width, int qp,
                        int reset_feature_memory, int padding_b, int padding_r, void* stream)
{
    return compress(c, x, height, width, qp, reset_feature_memory, padding_b, padding_r, stream);
}

int64_t dcvc_dmcld_get_stream(dcvc_dmcld* c, uint8_t* dst, size_t cap) { return get_stream(c, dst, cap); }

int dcvc_dmcld_decompress(dcvc_dmcld* c, const uint8_t* bit_stream, size_t nbytes, int qp, int height,
                          int width, int ec_parallel, int reset_feature_memory, void* x_hat,
                          void* stream)
{
    return decompress(c, bit_stream, nbytes, qp, height, width, ec_parallel, reset_feature_memory, x_hat, stream);
}

int dcvc_dmcld_estimate_bits(dcvc_dmcld* c, const void* x, int height, int width, int qp, int padding_b, int padding_r,
                             int64_t* out_units, void* stream)
{
    return estimate_bits(c, x, height, width, qp, padding_b, padding_r, out_units, stream);
}

int64_t dcvc_dmcld_estimate_symbols(dcvc_dmcld* c) { return estimate_symbols(c); }

int dcvc_dmcld_reconstruct(dcvc_dmcld* c, void* x_hat, void* stream) { return reconstruct(c, "dcvc_dmcld_reconstruct", x_hat, stream); }

int64_t dcvc_dmcld_export_state(dcvc_dmcld* c, void* dst, size_t cap, void* stream) { return export_state(c, dst, cap, stream); }

int dcvc_dmcld_import_state(dcvc_dmcld* c, const void* src, size_t bytes, int height, int width, void* stream)
{
    return import_state(c, src, bytes, height, width, stream);
}

int dcvc_dmcld_set_use_graphs(dcvc_dmcld* c, int on) { return set_use_graphs(c, on); }

int64_t dcvc_dmcld_debug_read(dcvc_dmcld* c, const char* name, void* dst, size_t cap, void* stream)
{
    return debug_read(c, name, dst, cap, stream);
}

// ------------------------------------------------------------------------------------ DMC-HT
dcvc_dmcht* dcvc_dmcht_create(int is_hts)
{
    dcvc_dmcht* c = nullptr;
    dcvc::guarded([&] { c = new dcvc_dmcht(is_hts != 0); });
    return c;
}

void dcvc_dmcht_destroy(dcvc_dmcht* c)
{
    delete c;
}

int dcvc_dmcht_set_param(dcvc_dmcht* c, int n, const char* const* names, const void* const* data,
                         const int* dtypes, const int* ndims, const int64_t* dims, float skip_thres)
{
    return set_param(c, n, names, data, dtypes, ndims, dims, skip_thres);
}

int dcvc_dmcht_add_ref_feature_from_frame(dcvc_dmcht* c, const void* frame, int height, int width,
                                          int apply_adaptor, void* stream)
{
    return add_ref(c, frame, height, width, apply_adaptor, stream);
}

int dcvc_dmcht_compress(dcvc_dmcht* c, const void* x, int height, int width, int qp,
                        int reset_feature_memory, int padding_b, int padding_r, void* stream)
{
    return compress(c, x, height, width, qp, reset_feature_memory, padding_b, padding_r, stream);
}

int64_t dcvc_dmcht_get_stream(dcvc_dmcht* c, uint8_t* dst, size_t cap) { return get_stream(c, dst, cap); }

int dcvc_dmcht_decompress(dcvc_dmcht* c, const uint8_t* bit_stream, size_t nbytes, int qp, int height,
                          int width, int ec_parallel, int reset_feature_memory, void* x_hat,
                          void* stream)
{
    return decompress(c, bit_stream, nbytes, qp, height, width, ec_parallel, reset_feature_memory, x_hat, stream);
}

int dcvc_dmcht_estimate_bits(dcvc_dmcht* c, const void* x, int height, int width, int qp, int padding_b, int padding_r,
                             int64_t* out_units, void* stream)
{
    return estimate_bits(c, x, height, width, qp, padding_b, padding_r, out_units, stream);
}

int64_t dcvc_dmcht_estimate_symbols(dcvc_dmcht* c) { return estimate_symbols(c); }

int dcvc_dmcht_reconstruct(dcvc_dmcht* c, void* x_hat, void* stream) { return reconstruct(c, "dcvc_dmcht_reconstruct", x_hat, stream); }

int64_t dcvc_dmcht_export_state(dcvc_dmcht* c, void* dst, size_t cap, void* stream) { return export_state(c, dst, cap, stream); }

int dcvc_dmcht_import_state(dcvc_dmcht* c, const void* src, size_t bytes, int height, int width, void* stream)
{
    return import_state(c, src, bytes, height, width, stream);
}

int dcvc_dmcht_set_recon_mask(dcvc_dmcht* c, unsigned mask)
{
    return dcvc::guarded([&] { c->codec.set_recon_mask(mask); });
}

int64_t dcvc_dmcht_export_feature(dcvc_dmcht* c, void* dst, size_t cap, void* stream)
{
    return guarded_size([&] { return c->codec.export_feature(dst, cap, hip_stream(stream)); });
}

int dcvc_dmcht_import_feature(dcvc_dmcht* c, const void* src, size_t bytes, int height, int width, void* stream)
{
    return dcvc::guarded([&] { c->codec.import_feature(src, bytes, height, width, hip_stream(stream)); });
}

int dcvc_dmcht_run_recon_heads(dcvc_dmcht* c, unsigned mask, void* x_hat, void* stream)
{
    return dcvc::guarded([&] { c->codec.run_recon_heads(mask, static_cast<dcvc::half_t*>(x_hat), hip_stream(stream)); });
}

int dcvc_dmcht_set_use_graphs(dcvc_dmcht* c, int on) { return set_use_graphs(c, on); }

int64_t dcvc_dmcht_debug_read(dcvc_dmcht* c, const char* name, void* dst, size_t cap, void* stream)
{
    return debug_read(c, name, dst, cap, stream);
}

}  // extern "C"
