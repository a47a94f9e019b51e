// C ABI of the individual kernels (include/dcvc_amd_ops.h).
#include "capi_common.h"
#include <initializer_list>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>
#include "dcvc_amd_ops.h"
#include "kernels/ops.h"
#include "rans/code_length.h"

namespace {

using dcvc::half_t;

inline const half_t* H(const void* p) { return static_cast<const half_t*>(p); }
inline half_t* H(void* p) { return static_cast<half_t*>(p); }
inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }

// one lazily allocated page of zeros for padding taps
const half_t* zero_page()
{
    static half_t* z = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        dcvc::hip_check(hipMalloc(&z, 4096), "hipMalloc(zero page)");
        dcvc::hip_check(hipMemset(z, 0, 4096), "hipMemset(zero page)");
    });
    return z;
}

}  // namespace

extern "C" {

int dcvc_conv1x1(const void* x, int ldx, const void* w, const void* bias, const void* r1, int ldr1,
                 const void* r2, int ldr2, const void* q, const void* q2, void* y, int ldy,
                 int pixels, int cin, int cout, int flags, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::Conv1x1Desc d;
        d.x = H(x); d.ldx = ldx; d.w = H(w); d.bias = H(bias);
        d.r1 = H(r1); d.ldr1 = ldr1; d.r2 = H(r2); d.ldr2 = ldr2;
        d.q = H(q); d.q2 = H(q2); d.y = H(y); d.ldy = ldy;
        d.pixels = pixels; d.cin = cin; d.cout = cout;
        dcvc::kernels_init();
        d.wsilu = (flags & DCVC_CONV_WSILU) != 0;
        d.chunk_add = (flags & DCVC_CONV_CHUNK_ADD) != 0;
        dcvc::conv1x1(d, S(stream));
    });
}

int dcvc_conv_kxk(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy,
                  int in_h, int in_w, int cin, int cout, int ksize, int stride, int pad, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::ConvKxKDesc d;
        d.x = H(x); d.ldx = ldx; d.w = H(w); d.bias = H(bias); d.zeros = zero_page();
        d.y = H(y); d.ldy = ldy; d.in_h = in_h; d.in_w = in_w; d.cin = cin; d.cout = cout;
        d.ksize = ksize; d.stride = stride; d.pad = pad;
        dcvc::conv_kxk(d, S(stream));
    });
}

int dcvc_tconv2x2(const void* x, int ldx, const void* w, void* y, int ldy, int in_h, int in_w,
                  int cin, int cout, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::TConv2x2Desc d;
        d.x = H(x); d.ldx = ldx; d.w = H(w); d.y = H(y); d.ldy = ldy;
        d.in_h = in_h; d.in_w = in_w; d.cin = cin; d.cout = cout;
        dcvc::tconv2x2(d, S(stream));
    });
}

int dcvc_dwconv3x3(const void* x, int ldx, const void* w, void* y, int ldy, int Hh, int W, int C,
                   void* stream)
{
    return dcvc::guarded([&] { dcvc::dwconv3x3(H(x), ldx, H(w), H(y), ldy, Hh, W, C, S(stream)); });
}

// ---- argument checks before any launch, shared by the single and the batched forms of an entry point
namespace {

void check_b(int n, std::initializer_list<const void*> ptrs, std::initializer_list<int> dims, const char* what)
{
    if (n < 1 || n > 16) throw std::invalid_argument(std::string(what) + ": n must be in [1, 16]");
    for (const void* p : ptrs) {
        if (p == nullptr) throw std::invalid_argument(std::string(what) + ": null pointer");
    }
    for (int d : dims) {
        if (d <= 0) throw std::invalid_argument(std::string(what) + ": sizes must be positive");
    }
}

[[noreturn]] void refuse(const char* what, const char* why)
{
    throw std::invalid_argument(std::string(what) + ": " + why);
}

// an operand whose rows the kernel reads or writes 16 bytes at a time: [pixels][ld] halves, `C` of them used
struct Rows {
    const void* p;
    int ld;
};

void check_rows(std::initializer_list<Rows> rows, int C, const char* what)
{
    if (C % 8 != 0) refuse(what, "C must be a multiple of 8");
    for (const Rows& r : rows) {
        if (r.ld < C) refuse(what, "leading dimension below C");
        if (r.ld % 8 != 0 || (reinterpret_cast<uintptr_t>(r.p) & 15) != 0) {
            refuse(what, "16-byte accesses: pointers must be 16-byte aligned and leading dimensions multiples of 8");
        }
    }
}

void check_aligned(std::initializer_list<const void*> ptrs, unsigned bytes, const char* what)
{
    for (const void* p : ptrs) {
        if ((reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0) refuse(what, "misaligned pointer");
    }
}

void check_pad_unshuffle8(const void* x, int Hh, int W, int C3, const void* out, int ldout, int H8, int W8, int n, const char* what)
{
    check_b(n, {x, out}, {Hh, W, C3, H8, W8}, what);
    if (H8 * 8 < Hh || W8 * 8 < W) refuse(what, "output smaller than the picture");
    check_rows({{out, ldout}}, 64 * C3, what);
}

void check_shuffle8(const void* in, int ldin, int H8, int W8, int C3, const void* out, int n, const char* what)
{
    check_b(n, {in, out}, {H8, W8, C3}, what);
    if (ldin < C3 * 64) refuse(what, "ldin below 64 * C3");
    check_rows({{in, ldin}}, 64 * C3, what);
}

void check_replicate_pad(const void* in, int ldin, int Hh, int W, int C, int pad_b, int pad_r, const void* out, int ldout, int n,
                         const char* what)
{
    check_b(n, {in, out}, {Hh, W, C}, what);
    if (pad_b < 0 || pad_r < 0 || C % 8 != 0 || ldin < C || ldout < C) {
        refuse(what, "negative padding, C not a multiple of 8 or ld below C");
    }
    check_rows({{in, ldin}, {out, ldout}}, C, what);
}

void check_crop(const void* in, int ldin, int Hin, int Win, const void* out, int ldout, int Hh, int W, int C, int n, const char* what)
{
    check_b(n, {in, out}, {Hin, Win, Hh, W, C}, what);
    if (Hh > Hin || W > Win || C % 8 != 0 || ldin < C || ldout < C) {
        refuse(what, "crop larger than the input, C not a multiple of 8 or ld below C");
    }
    check_rows({{in, ldin}, {out, ldout}}, C, what);
}

// the 4-step symbol kernels: C/4 symbols per pixel in runs of 8, every picture of a batch the same size
void check_y_step(int n, int Hh, int W, int C, int step, int slot, const char* what)
{
    if (Hh <= 0 || W <= 0 || C <= 0) refuse(what, "sizes must be positive");
    if (C % 32 != 0) refuse(what, "C must be a multiple of 32");
    if (step < 0 || step > 3 || slot < 0 || slot > 3) refuse(what, "step and slot must be in 0..3");
    if (static_cast<long long>(Hh) * W * C * n >= (1LL << 31)) refuse(what, "more than 2^31 elements");
}

void check_strides(int n, long long data_stride, int totals_stride, const char* what)
{
    if (n > 1 && (data_stride <= 0 || totals_stride <= 0)) refuse(what, "a batch needs positive picture strides");
    if (data_stride < 0 || totals_stride < 0) refuse(what, "negative picture stride");
}

}  // namespace

int dcvc_dwconv3x3_b(const void* x, int ldx, const void* w, void* y, int ldy, int Hh, int W, int C, int n, void* stream)
{
    return dcvc::guarded([&] {
        check_b(n, {x, w, y}, {Hh, W, C}, "dwconv3x3_b");
        if (ldx < C || ldy < C) throw std::invalid_argument("dwconv3x3_b: leading dimensions below C");
        dcvc::dwconv3x3_b(H(x), ldx, H(w), H(y), ldy, Hh, W, C, n, S(stream));
    });
}

int dcvc_conv_kxk_b(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy, int in_h, int in_w, int cin,
                    int cout, int ksize, int stride, int pad, int n, void* stream)
{
    return dcvc::guarded([&] {
        check_b(n, {x, w, y}, {in_h, in_w, cin, cout, ksize, stride}, "conv_kxk_b");
        if (pad < 0 || in_h + 2 * pad < ksize || in_w + 2 * pad < ksize) throw std::invalid_argument("conv_kxk_b: bad padding");
        dcvc::ConvKxKDesc d;
        d.x = H(x); d.ldx = ldx; d.w = H(w); d.bias = H(bias); d.zeros = zero_page();
        d.y = H(y); d.ldy = ldy; d.in_h = in_h; d.in_w = in_w; d.cin = cin; d.cout = cout;
        d.ksize = ksize; d.stride = stride; d.pad = pad; d.n = n;
        dcvc::conv_kxk(d, S(stream));
    });
}

int dcvc_tconv2x2_b(const void* x, int ldx, const void* w, void* y, int ldy, int in_h, int in_w, int cin, int cout, int n,
                    void* stream)
{
    return dcvc::guarded([&] {
        check_b(n, {x, w, y}, {in_h, in_w, cin, cout}, "tconv2x2_b");
        dcvc::TConv2x2Desc d;
        d.x = H(x); d.ldx = ldx; d.w = H(w); d.y = H(y); d.ldy = ldy;
        d.in_h = in_h; d.in_w = in_w; d.cin = cin; d.cout = cout; d.n = n;
        dcvc::tconv2x2(d, S(stream));
    });
}

int dcvc_pad_unshuffle8_b(const void* x, int Hh, int W, int C3, void* out, int H8, int W8, int n, void* stream)
{
    return dcvc::guarded([&] {
        check_pad_unshuffle8(x, Hh, W, C3, out, 64 * C3, H8, W8, n, "pad_unshuffle8_b");
        dcvc::pad_unshuffle8_b(H(x), Hh, W, C3, H(out), H8, W8, n, S(stream));
    });
}

int dcvc_shuffle8_b(const void* in, int ldin, int H8, int W8, int C3, int clamp, void* out, int n, void* stream)
{
    return dcvc::guarded([&] {
        check_shuffle8(in, ldin, H8, W8, C3, out, n, "shuffle8_b");
        dcvc::shuffle8_b(H(in), ldin, H8, W8, C3, clamp != 0, H(out), n, S(stream));
    });
}

int dcvc_replicate_pad_b(const void* in, int ldin, int Hh, int W, int C, int pad_b, int pad_r, void* out, int ldout, int n,
                         void* stream)
{
    return dcvc::guarded([&] {
        check_replicate_pad(in, ldin, Hh, W, C, pad_b, pad_r, out, ldout, n, "replicate_pad_b");
        dcvc::replicate_pad_b(H(in), ldin, Hh, W, C, pad_b, pad_r, H(out), ldout, n, S(stream));
    });
}

int dcvc_crop_b(const void* in, int ldin, int Hin, int Win, void* out, int ldout, int Hh, int W, int C, int n, void* stream)
{
    return dcvc::guarded([&] {
        check_crop(in, ldin, Hin, Win, out, ldout, Hh, W, C, n, "crop_b");
        dcvc::crop_b(H(in), ldin, Hin, Win, H(out), ldout, Hh, W, C, n, S(stream));
    });
}

int dcvc_pad_unshuffle8(const void* x, int Hh, int W, int C3, void* out, int H8, int W8, void* stream)
{
    return dcvc::guarded([&] {
        check_pad_unshuffle8(x, Hh, W, C3, out, 64 * C3, H8, W8, 1, "pad_unshuffle8");
        dcvc::pad_unshuffle8(H(x), Hh, W, C3, H(out), H8, W8, S(stream));
    });
}

int dcvc_pad_unshuffle8_ld(const void* x, int Hh, int W, int C3, void* out, int ldout, int H8, int W8, void* stream)
{
    return dcvc::guarded([&] {
        check_pad_unshuffle8(x, Hh, W, C3, out, ldout, H8, W8, 1, "pad_unshuffle8_ld");
        dcvc::pad_unshuffle8(H(x), Hh, W, C3, H(out), H8, W8, S(stream), ldout);
    });
}

int dcvc_shuffle8(const void* in, int ldin, int H8, int W8, int C3, int clamp, void* out, void* stream)
{
    return dcvc::guarded([&] {
        check_shuffle8(in, ldin, H8, W8, C3, out, 1, "shuffle8");
        dcvc::shuffle8(H(in), ldin, H8, W8, C3, clamp != 0, H(out), S(stream));
    });
}

int dcvc_shuffle2(const void* in, int ldin, int Hh, int W, int C, void* out, int ldout, void* stream)
{
    return dcvc::guarded([&] {
        check_b(1, {in, out}, {Hh, W, C}, "shuffle2");
        if (ldin < 4 * C) refuse("shuffle2", "ldin below 4 * C");
        check_rows({{out, ldout}}, C, "shuffle2");
        dcvc::shuffle2(H(in), ldin, Hh, W, C, H(out), ldout, S(stream));
    });
}

int dcvc_replicate_pad(const void* in, int ldin, int Hh, int W, int C, int pad_b, int pad_r,
                       void* out, int ldout, void* stream)
{
    return dcvc::guarded([&] {
        check_replicate_pad(in, ldin, Hh, W, C, pad_b, pad_r, out, ldout, 1, "replicate_pad");
        dcvc::replicate_pad(H(in), ldin, Hh, W, C, pad_b, pad_r, H(out), ldout, S(stream));
    });
}

int dcvc_crop(const void* in, int ldin, int Win, void* out, int ldout, int Hh, int W, int C, void* stream)
{
    return dcvc::guarded([&] {
        check_crop(in, ldin, Hh, Win, out, ldout, Hh, W, C, 1, "crop");       // (one picture: its height is never read)
        dcvc::crop(H(in), ldin, Win, H(out), ldout, Hh, W, C, S(stream));
    });
}

int dcvc_mul_channel(const void* x, int ldx, const void* q, void* y, int ldy, int pixels, int C,
                     void* stream)
{
    return dcvc::guarded([&] {
        check_b(1, {x, q, y}, {pixels, C}, "mul_channel");
        check_rows({{x, ldx}, {q, C}, {y, ldy}}, C, "mul_channel");
        dcvc::mul_channel(H(x), ldx, H(q), H(y), ldy, pixels, C, S(stream));
    });
}

int dcvc_ffn_fused(const void* x, int ldx, const void* w0, const void* b0, const void* w2, const void* b2,
                   const void* r2, int ldr2, const void* q, const void* q2, void* y, int ldy,
                   int pixels, int c, int cffn, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        dcvc::FfnFusedDesc d;
        d.x = H(x); d.ldx = ldx; d.w0 = H(w0); d.b0 = H(b0); d.w2 = H(w2); d.b2 = H(b2);
        d.r2 = H(r2); d.ldr2 = ldr2; d.q = H(q); d.q2 = H(q2); d.y = H(y); d.ldy = ldy;
        d.pixels = pixels; d.c = c; d.cffn = cffn;
        dcvc::ffn_fused(d, S(stream));
    });
}

namespace {
// The N-split kernel wants its per-wave fragment streams, not the reference's row-major matrices. The codecs pack once
// at set_param time (dcvc::DcbW::load). The operator-level entry points below serve tests and tools:
//   dcvc_dcb_nsplit          packs on EVERY call into stream-ordered temporaries (hipMallocAsync / hipFreeAsync on the
//                            caller's stream): always reads the weights as they are now. (Round 3 cached packed copies per
//                            weight POINTER: a caller that rewrote its weights in place, or whose allocator handed the same
//                            address out again, silently got the old weights - advisor, round 3.)
//   dcvc_dcb_nsplit_pack / _packed / _free   explicit handle for callers that launch many times (tools/probes/core_bench).
// Device buffers of the entry points below, released on every path out (advisor, round 4: a throwing pack launch leaked them).
// Stream-ordered temporaries (hipMallocAsync / hipFreeAsync on the caller's stream) or plain allocations of a device.
struct AsyncBuf {
    void* p = nullptr;
    hipStream_t st = nullptr;
    AsyncBuf(size_t bytes, hipStream_t stream, const char* what = "hipMallocAsync(packed weights)") : st(stream)
    {
        dcvc::hip_check(hipMallocAsync(&p, bytes, st), what);
    }
    ~AsyncBuf() { if (p) (void)hipFreeAsync(p, st); }
    AsyncBuf(const AsyncBuf&) = delete;
    AsyncBuf& operator=(const AsyncBuf&) = delete;
    dcvc::half_t* half() const { return static_cast<dcvc::half_t*>(p); }
};

struct NsplitPacked {
    int c = 0, ci = 0, device = 0;
    dcvc::half_t* main = nullptr;
    dcvc::half_t* next = nullptr;
    hipEvent_t packed = nullptr;          // recorded behind the pack launches: dcvc_dcb_nsplit_packed on ANOTHER stream waits for it
    hipStream_t pack_stream = nullptr;    // ... the stream they ran on needs no wait (and may be capturing: advisor, round 5)
    mutable bool settled = false;         // the event has been seen complete: no launch waits for it any more
    NsplitPacked() = default;
    NsplitPacked(const NsplitPacked&) = delete;
    NsplitPacked& operator=(const NsplitPacked&) = delete;
    ~NsplitPacked()
    {
        // on the device that owns the buffers, behind every launch that may still read them
        int cur = 0;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        if (have && cur != device) (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        if (main) (void)hipFree(main);
        if (next) (void)hipFree(next);
        if (packed) (void)hipEventDestroy(packed);
        if (have && cur != device) (void)hipSetDevice(cur);
    }
};

// The four block entries' common part: the pack launches of the weights that are given (null: none) into their buffers
struct NsplitStreams { dcvc::half_t* main = nullptr; dcvc::half_t* next = nullptr; dcvc::half_t* fin = nullptr; };
void nsplit_pack(const NsplitStreams& out, const void* w3, const void* w0, const void* w2, const void* w1n, const void* wfin, int nfin,
                 int c, int ci, hipStream_t st)
{
    dcvc::dcb_nsplit_pack_main(H(w3), H(w0), H(w2), c, ci, out.main, st);
    if (w1n != nullptr) dcvc::dcb_nsplit_pack_dc0(H(w1n), c, ci, out.next, st);
    if (wfin != nullptr) dcvc::dcb_nsplit_pack_fin(H(wfin), c, nfin, out.fin, st);
}

// ... as temporaries that live exactly as long as a call's launches (stream-ordered, freed on every path out), named in its descriptor
struct NsplitTemps {
    AsyncBuf main;
    std::unique_ptr<AsyncBuf> next, fin;
    dcvc::DcbNsplitDesc d;
    NsplitTemps(const void* w3, const void* w0, const void* w2, const void* w1n, const void* wfin, int nfin, int c, int ci, hipStream_t st)
        : main(dcvc::dcb_nsplit_main_halves(c, ci) * 2, st)
    {
        if (w1n != nullptr) next = std::make_unique<AsyncBuf>(dcvc::dcb_nsplit_dc0_halves(c, ci) * 2, st);
        if (wfin != nullptr) fin = std::make_unique<AsyncBuf>(dcvc::dcb_nsplit_fin_halves(c, nfin) * 2, st);
        const NsplitStreams out{main.half(), next ? next->half() : nullptr, fin ? fin->half() : nullptr};
        nsplit_pack(out, w3, w0, w2, w1n, wfin, nfin, c, ci, st);
        d.wmain = out.main; d.wnext = out.next; d.wfin = out.fin; d.nfin = fin ? nfin : 0; d.c = c; d.ci = ci;
    }
};

// what every block launch takes besides its weights and its entry operand (t2 / t1)
void nsplit_common(dcvc::DcbNsplitDesc& d, const void* x, int ldx, const void* b3, const void* b0, const void* b2, const void* q,
                   const void* q2, void* y, int ldy, int pixels, int shortcut)
{
    d.x = H(x); d.ldx = ldx; d.b3 = H(b3); d.b0 = H(b0); d.b2 = H(b2); d.q = H(q); d.q2 = H(q2);
    d.y = H(y); d.ldy = ldy; d.pixels = pixels; d.shortcut = shortcut != 0;
}
}  // namespace

int dcvc_dcb_nsplit(const void* t2, int ldt, const void* x, int ldx, const void* w3, const void* b3,
                    const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                    const void* w1n, const void* b1n, void* t1n, int ldt1, void* y, int ldy,
                    int pixels, int c, int ci, int shortcut, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        dcvc::dcb_nsplit_check_shape(c, ci);
        if (!w3 || !w0 || !w2) throw std::invalid_argument("dcb_nsplit: missing operand");
        NsplitTemps temps(w3, w0, w2, w1n, nullptr, 0, c, ci, S(stream));
        dcvc::DcbNsplitDesc& d = temps.d;
        nsplit_common(d, x, ldx, b3, b0, b2, q, q2, y, ldy, pixels, shortcut);
        d.t2 = H(t2); d.ldt = ldt; d.b1n = H(b1n); d.t1n = H(t1n); d.ldt1 = ldt1;
        dcvc::dcb_nsplit(d, S(stream));
    });
}

int dcvc_dcb_pair_supported(int cin, int c, int ci)
{
    return dcvc::dcb_pair_supported(cin, c, ci) ? 1 : 0;
}

int dcvc_dcb_pair(const void* x, int ldx, const void* wa, const void* ba, const void* w1, const void* b1,
                  void* y, int ldy, void* t1, int ldt1, int pixels, int cin, int c, int ci, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        if (!dcvc::dcb_pair_supported(cin, c, ci)) throw std::invalid_argument("dcb_pair: no kernel variant for this shape");
        if (!x || !wa || !ba || !w1 || !b1 || !y || !t1) throw std::invalid_argument("dcb_pair: missing operand");
        if (x == y) throw std::invalid_argument("dcb_pair: the adaptor output must not alias its input");
        hipStream_t st = S(stream);
        const AsyncBuf pa(dcvc::dcb_pair_adaptor_halves(cin, c) * 2, st);
        dcvc::dcb_pair_pack_adaptor(H(wa), cin, c, pa.half(), st);
        const AsyncBuf p1(dcvc::dcb_nsplit_dc0_halves(c, ci) * 2, st);
        dcvc::dcb_nsplit_pack_dc0(H(w1), c, ci, p1.half(), st);
        dcvc::DcbPairDesc d;
        d.x = H(x); d.ldx = ldx; d.wa = pa.half(); d.ba = H(ba); d.w1 = p1.half(); d.b1 = H(b1);
        d.y = H(y); d.ldy = ldy; d.t1 = H(t1); d.ldt1 = ldt1; d.pixels = pixels; d.cin = cin; d.c = c; d.ci = ci;
        dcvc::dcb_pair(d, st);
    });
}

int dcvc_dcb_nsplit_fin_supported(int c, int ci, int nfin)
{
    return dcvc::dcb_nsplit_fin_supported(c, ci, nfin) ? 1 : 0;
}

int dcvc_dcb_nsplit_fin(const void* t2, int ldt, const void* x, int ldx, const void* w3, const void* b3,
                        const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                        const void* wfin, const void* bfin, const void* qfin, void* yfin, int ldyfin, int nfin,
                        void* y, int ldy, int pixels, int c, int ci, int shortcut, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        dcvc::dcb_nsplit_check_shape(c, ci);
        if (!w3 || !w0 || !w2 || !wfin || !bfin || !yfin) throw std::invalid_argument("dcb_nsplit_fin: missing operand");
        if (!dcvc::dcb_nsplit_fin_supported(c, ci, nfin)) throw std::invalid_argument("dcb_nsplit_fin: no kernel variant for this closing conv");
        NsplitTemps temps(w3, w0, w2, nullptr, wfin, nfin, c, ci, S(stream));
        dcvc::DcbNsplitDesc& d = temps.d;
        nsplit_common(d, x, ldx, b3, b0, b2, q, q2, y, ldy, pixels, shortcut);
        d.t2 = H(t2); d.ldt = ldt;
        d.bfin = H(bfin); d.qfin = H(qfin); d.yfin = H(yfin); d.ldyfin = ldyfin;
        dcvc::dcb_nsplit(d, S(stream));
    });
}

int dcvc_dcb_nsplit_dw_supported(int c, int ci, int pixels)
{
    return dcvc::dcb_nsplit_dw_supported(c, ci, pixels) ? 1 : 0;
}

int dcvc_dcb_nsplit_dw(const void* t1, int ldt, const void* wdw, int width, const void* x, int ldx, const void* w3, const void* b3,
                       const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                       const void* w1n, const void* b1n, void* t1n, int ldt1,
                       const void* wfin, const void* bfin, const void* qfin, void* yfin, int ldyfin, int nfin,
                       void* y, int ldy, int pixels, int c, int ci, int shortcut, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        dcvc::dcb_nsplit_check_shape(c, ci);
        if (!t1 || !wdw || !w3 || !w0 || !w2) throw std::invalid_argument("dcb_nsplit_dw: missing operand");
        if (!dcvc::dcb_nsplit_dw_supported(c, ci, pixels)) throw std::invalid_argument("dcb_nsplit_dw: no kernel variant with the depthwise conv inside for this block shape");
        if (wfin != nullptr && !dcvc::dcb_nsplit_fin_supported(c, ci, nfin)) throw std::invalid_argument("dcb_nsplit_dw: no kernel variant for this closing conv");
        if (static_cast<long long>(pixels) * ldt * 2 >= (1LL << 31)) throw std::invalid_argument("dcb_nsplit_dw: dc.0's output must span less than 2 GiB (32-bit byte offsets inside the launch)");
        NsplitTemps temps(w3, w0, w2, w1n, wfin, nfin, c, ci, S(stream));
        dcvc::DcbNsplitDesc& d = temps.d;
        nsplit_common(d, x, ldx, b3, b0, b2, q, q2, y, ldy, pixels, shortcut);
        d.t1 = H(t1); d.ldt = ldt; d.wdw = H(wdw); d.width = width;
        d.b1n = H(b1n); d.t1n = H(t1n); d.ldt1 = ldt1;
        if (wfin != nullptr) { d.bfin = H(bfin); d.qfin = H(qfin); d.yfin = H(yfin); d.ldyfin = ldyfin; }
        dcvc::dcb_nsplit(d, S(stream));
    });
}

int dcvc_dcb_nsplit_pack(const void* w3, const void* w0, const void* w2, const void* w1n, int c, int ci, void* stream, void** handle)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        dcvc::dcb_nsplit_check_shape(c, ci);
        if (!w3 || !w0 || !w2 || !handle) throw std::invalid_argument("dcb_nsplit_pack: missing operand");
        auto pk = std::make_unique<NsplitPacked>();          // its destructor frees whatever has been allocated when a step below throws
        pk->c = c; pk->ci = ci;
        dcvc::hip_check(hipGetDevice(&pk->device), "hipGetDevice");
        // (each buffer is the handle's as soon as it exists)
        dcvc::hip_check(hipMalloc(reinterpret_cast<void**>(&pk->main), dcvc::dcb_nsplit_main_halves(c, ci) * 2), "hipMalloc(packed weights)");
        if (w1n != nullptr) dcvc::hip_check(hipMalloc(reinterpret_cast<void**>(&pk->next), dcvc::dcb_nsplit_dc0_halves(c, ci) * 2), "hipMalloc(packed weights)");
        nsplit_pack(NsplitStreams{pk->main, pk->next, nullptr}, w3, w0, w2, w1n, nullptr, 0, c, ci, S(stream));
        dcvc::hip_check(hipEventCreateWithFlags(&pk->packed, hipEventDisableTiming), "hipEventCreate");
        dcvc::hip_check(hipEventRecord(pk->packed, S(stream)), "hipEventRecord(packed)");
        pk->pack_stream = S(stream);
        *handle = pk.release();
    });
}

int dcvc_dcb_nsplit_free(void* handle)
{
    return dcvc::guarded([&] {
        if (handle == nullptr) return;
        // ~NsplitPacked: synchronises the OWNING device (not whichever is current), then frees
        std::unique_ptr<NsplitPacked> pk(static_cast<NsplitPacked*>(handle));
        // a failure of an earlier launch surfaces at this synchronisation: report it (the destructor cannot), then free anyway
        int cur = 0;
        dcvc::hip_check(hipGetDevice(&cur), "hipGetDevice");
        if (cur != pk->device) dcvc::hip_check(hipSetDevice(pk->device), "hipSetDevice");
        const hipError_t e = hipDeviceSynchronize();
        if (cur != pk->device) (void)hipSetDevice(cur);
        pk.reset();
        dcvc::hip_check(e, "hipDeviceSynchronize(dcb_nsplit_free)");
    });
}

int dcvc_dcb_nsplit_packed(const void* handle, const void* t2, int ldt, const void* x, int ldx, const void* b3, const void* b0,
                           const void* b2, const void* q, const void* q2, const void* b1n, void* t1n, int ldt1,
                           void* y, int ldy, int pixels, int shortcut, int with_next, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        if (handle == nullptr) throw std::invalid_argument("dcb_nsplit_packed: null handle");
        const NsplitPacked* pk = static_cast<const NsplitPacked*>(handle);
        int dev = 0;
        dcvc::hip_check(hipGetDevice(&dev), "hipGetDevice");
        if (dev != pk->device) throw std::invalid_argument("dcb_nsplit_packed: the handle was packed on another device");
        if (with_next && pk->next == nullptr) throw std::invalid_argument("dcb_nsplit_packed: packed without the next block's dc.0");
        // the pack launches ran on the stream given to _pack: any OTHER stream orders itself behind them here, until the event has
        // been seen complete once (a wait per launch is a barrier packet per launch; and a stream that is being captured must not
        // wait for an event recorded outside the capture - pack and first launch belong in front of a capture)
        if (S(stream) != pk->pack_stream && !pk->settled) {
            if (hipEventQuery(pk->packed) == hipSuccess) pk->settled = true;
            else dcvc::hip_check(hipStreamWaitEvent(S(stream), pk->packed, 0), "hipStreamWaitEvent(packed)");
        }
        dcvc::DcbNsplitDesc d;
        d.c = pk->c; d.ci = pk->ci; d.wmain = pk->main; d.wnext = with_next ? pk->next : nullptr;
        nsplit_common(d, x, ldx, b3, b0, b2, q, q2, y, ldy, pixels, shortcut);
        d.t2 = H(t2); d.ldt = ldt; d.b1n = H(b1n); d.t1n = H(t1n); d.ldt1 = ldt1;
        dcvc::dcb_nsplit(d, S(stream));
    });
}

int dcvc_dcb_tail(const void* w1, const void* b1, const void* t, int ldt, const void* dw, const void* x, int ldx,
                  const void* w3, const void* b3,
                  const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                  void* y, int ldy, int Hh, int W, int c, int cdc, int cffn, int shortcut, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::kernels_init();
        dcvc::DcbTailDesc d;
        d.w1 = H(w1); d.b1 = H(b1); d.t = H(t); d.ldt = ldt; d.dw = H(dw); d.x = H(x); d.ldx = ldx; d.w3 = H(w3); d.b3 = H(b3);
        d.w0 = H(w0); d.b0 = H(b0); d.w2 = H(w2); d.b2 = H(b2); d.q = H(q); d.q2 = H(q2);
        d.y = H(y); d.ldy = ldy; d.H = Hh; d.W = W; d.c = c; d.cdc = cdc; d.cffn = cffn; d.shortcut = shortcut != 0;
        if (d.w1 != nullptr && d.x == d.y) throw std::invalid_argument("dcb_tail with dc.0 inside cannot run in place");
        dcvc::dcb_tail(d, S(stream));
    });
}

int dcvc_dcb_tail_b(const void* w1, const void* b1, const void* t, int ldt, const void* dw, const void* x, int ldx,
                    const void* w3, const void* b3,
                    const void* w0, const void* b0, const void* w2, const void* b2, const void* q, const void* q2,
                    void* y, int ldy, int Hh, int W, int c, int cdc, int cffn, int shortcut, int n, void* stream)
{
    return dcvc::guarded([&] {
        check_b(n, {w1 != nullptr ? w1 : t, x, w3, b3, w0, b0, w2, b2, y}, {Hh, W, c, cdc, cffn}, "dcb_tail_b");
        if (w1 != nullptr && (b1 == nullptr || dw == nullptr)) throw std::invalid_argument("dcb_tail_b: dc.0 inside needs its bias and the depthwise taps");
        if (ldx < c || ldy < c || (w1 == nullptr && ldt < cdc)) throw std::invalid_argument("dcb_tail_b: leading dimensions below the channel counts");
        if (w1 != nullptr && x == y) throw std::invalid_argument("dcb_tail_b with dc.0 inside cannot run in place");
        dcvc::kernels_init();
        dcvc::DcbTailDesc d;
        d.w1 = H(w1); d.b1 = H(b1); d.t = H(t); d.ldt = ldt; d.dw = H(dw); d.x = H(x); d.ldx = ldx; d.w3 = H(w3); d.b3 = H(b3);
        d.w0 = H(w0); d.b0 = H(b0); d.w2 = H(w2); d.b2 = H(b2); d.q = H(q); d.q2 = H(q2);
        d.y = H(y); d.ldy = ldy; d.H = Hh; d.W = W; d.c = c; d.cdc = cdc; d.cffn = cffn; d.shortcut = shortcut != 0; d.n = n;
        dcvc::dcb_tail(d, S(stream));
    });
}

int dcvc_scale_clamped(const void* x, int ldx, const void* q, int ldq, void* y, int ldy, int pixels,
                       int C, int reciprocal, void* stream)
{
    return dcvc::guarded([&] {
        check_b(1, {x, q, y}, {pixels, C}, "scale_clamped");
        check_rows({{x, ldx}, {q, ldq}, {y, ldy}}, C, "scale_clamped");
        dcvc::scale_clamped(H(x), ldx, H(q), ldq, H(y), ldy, pixels, C, reciprocal != 0, S(stream));
    });
}

int dcvc_yuv420_to_x(const void* y, const void* uv, int H_, int W_, void* x, int ldx, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::yuv420_to_x(static_cast<const uint8_t*>(y), static_cast<const uint8_t*>(uv), H_, W_, H(x), ldx,
                          S(stream));
    });
}

int dcvc_x_to_yuv420(const void* x_hat, int row_pixels, int H_, int W_, void* y16, void* uv16, void* y8,
                     void* uv8, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::x_to_yuv420(H(x_hat), row_pixels, H_, W_, H(y16), H(uv16), static_cast<uint8_t*>(y8),
                          static_cast<uint8_t*>(uv8), S(stream));
    });
}

int dcvc_yuv420p16_to_x(const void* y, const void* uv, int H_, int W_, int bit_depth, void* x, int ldx, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::yuv420p16_to_x(static_cast<const uint16_t*>(y), static_cast<const uint16_t*>(uv), H_, W_, bit_depth, H(x), ldx,
                             S(stream));
    });
}

int dcvc_x_to_yuv420p16(const void* x_hat, int row_pixels, int H_, int W_, int bit_depth, void* dist32, void* yuv16, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::x_to_yuv420p16(H(x_hat), row_pixels, H_, W_, bit_depth, static_cast<float*>(dist32), static_cast<uint16_t*>(yuv16),
                             S(stream));
    });
}

long long dcvc_pix_picture_samples(int fmt, int H_, int W_)
{
    long long n = -1;
    const int rc = dcvc::guarded([&] { n = dcvc::pix_picture_samples(fmt, H_, W_); });
    return rc < 0 ? rc : n;
}

int dcvc_pix_to_x(const void* src, int fmt, int bit_depth, int H_, int W_, void* x, int ldx, void* planar, void* stream)
{
    return dcvc::guarded([&] { dcvc::pix_to_x(src, fmt, bit_depth, H_, W_, H(x), ldx, planar, S(stream)); });
}

int dcvc_x_to_pix(const void* x_hat, int row_pixels, int H_, int W_, int fmt, int bit_depth, void* dist32, void* out, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::x_to_pix(H(x_hat), row_pixels, H_, W_, fmt, bit_depth, static_cast<float*>(dist32), out, S(stream));
    });
}

int dcvc_wire_carrier(int wire)
{
    int fmt = -1;
    const int rc = dcvc::guarded([&] { fmt = dcvc::wire_carrier(wire); });
    return rc < 0 ? rc : fmt;
}

long long dcvc_wire_picture_bytes(int wire, int bit_depth, int H_, int W_)
{
    long long n = -1;
    const int rc = dcvc::guarded([&] { n = dcvc::wire_picture_bytes(wire, bit_depth, H_, W_); });
    return rc < 0 ? rc : n;
}

int dcvc_wire_unpack(const void* src, int wire, int bit_depth, int H_, int W_, void* carrier, void* stream)
{
    return dcvc::guarded([&] { dcvc::wire_unpack(src, wire, bit_depth, H_, W_, carrier, S(stream)); });
}

int dcvc_wire_pack(const void* carrier, int wire, int bit_depth, int H_, int W_, void* dst, void* stream)
{
    return dcvc::guarded([&] { dcvc::wire_pack(carrier, wire, bit_depth, H_, W_, dst, S(stream)); });
}

namespace {

// the operands of the dcvc_msssim* entries and of the dcvc_sse* entries: n_planes pairs of H x W planes
dcvc::MsssimDesc msssim_desc(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_, int row_stride,
                             long long plane_stride, double* out, double data_range = 255.0)
{
    dcvc::MsssimDesc d;
    d.src = src; d.src_dtype = src_dtype; d.rec = rec; d.rec_dtype = rec_dtype;
    d.n_planes = n_planes; d.H = H_; d.W = W_; d.row_stride = row_stride; d.plane_stride = plane_stride; d.out = out;
    d.data_range = data_range;
    return d;
}

dcvc::SseDesc sse_desc(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_, int row_stride,
                       long long plane_stride, double* out)
{
    dcvc::SseDesc d;
    d.src = src; d.src_dtype = src_dtype; d.rec = rec; d.rec_dtype = rec_dtype;
    d.n_planes = n_planes; d.H = H_; d.W = W_; d.row_stride = row_stride; d.plane_stride = plane_stride; d.out = out;
    return d;
}

dcvc::RgbToXDesc rgb_source(const void* src, long long row_stride, long long pixel_stride, long long channel_stride, int H_, int W_,
                             void* x, int ldx, void* planar)
{
    dcvc::RgbToXDesc d;
    d.src = static_cast<const uint8_t*>(src);
    d.row_stride = row_stride; d.pixel_stride = pixel_stride; d.channel_stride = channel_stride;
    d.H = H_; d.W = W_; d.x = H(x); d.ldx = ldx; d.planar = static_cast<uint8_t*>(planar);
    return d;
}

}  // namespace

int dcvc_msssim(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_,
                int row_stride, long long plane_stride, double* out, void* stream)
{
    return dcvc::guarded([&] {
        // this entry's contract: u8 and fp16 samples in 0..255 only (dcvc_msssim_range takes the others)
        for (int t : {src_dtype, rec_dtype}) {
            if (t != dcvc::kSampleU8 && t != dcvc::kSampleF16) {
                throw std::invalid_argument("msssim: sample type must be DCVC_SAMPLE_U8 or DCVC_SAMPLE_F16");
            }
        }
        const dcvc::MsssimDesc d = msssim_desc(src, src_dtype, rec, rec_dtype, n_planes, H_, W_, row_stride, plane_stride, out);
        dcvc::msssim_validate(d);      // before the workspace is sized: a bad geometry never reaches the allocator
        const AsyncBuf ws(dcvc::msssim_workspace_bytes(n_planes, H_, W_), S(stream), "hipMallocAsync(msssim workspace)");
        dcvc::msssim(d, ws.p, S(stream));
    });
}

int dcvc_msssim_range(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_,
                      int row_stride, long long plane_stride, double data_range, double* out, void* stream)
{
    return dcvc::guarded([&] {
        const dcvc::MsssimDesc d = msssim_desc(src, src_dtype, rec, rec_dtype, n_planes, H_, W_, row_stride, plane_stride, out, data_range);
        dcvc::msssim_validate(d);
        const AsyncBuf ws(dcvc::msssim_workspace_bytes(n_planes, H_, W_), S(stream), "hipMallocAsync(msssim workspace)");
        dcvc::msssim(d, ws.p, S(stream));
    });
}

long long dcvc_msssim_workspace_bytes(int n_planes, int H_, int W_)
{
    if (n_planes < 1 || n_planes > 65535 || H_ < 88 || W_ < 88) return 0;
    return static_cast<long long>(dcvc::msssim_workspace_bytes(n_planes, H_, W_));
}

int dcvc_msssim_range_ws(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_, int row_stride,
                         long long plane_stride, double data_range, double* out, void* workspace, long long workspace_bytes, void* stream)
{
    return dcvc::guarded([&] {
        const dcvc::MsssimDesc d = msssim_desc(src, src_dtype, rec, rec_dtype, n_planes, H_, W_, row_stride, plane_stride, out, data_range);
        dcvc::msssim_validate(d);
        if (workspace == nullptr || workspace_bytes < 0 ||
            static_cast<unsigned long long>(workspace_bytes) < dcvc::msssim_workspace_bytes(n_planes, H_, W_)) {
            throw std::invalid_argument("msssim: workspace missing or smaller than dcvc_msssim_workspace_bytes");
        }
        if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) throw std::invalid_argument("msssim: the workspace must be 16-byte aligned");
        dcvc::msssim(d, workspace, S(stream));
    });
}

int dcvc_rgb_to_x(const void* src, long long row_stride, long long pixel_stride, long long channel_stride, int H_, int W_,
                  void* x, int ldx, void* planar, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::rgb_to_x(rgb_source(src, row_stride, pixel_stride, channel_stride, H_, W_, x, ldx, planar), S(stream));
    });
}

int dcvc_x_to_rgb(const void* x_hat, int row_pixels, int H_, int W_, void* rgb16, void* rgb8, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::x_to_rgb(H(x_hat), row_pixels, H_, W_, H(rgb16), static_cast<uint8_t*>(rgb8), S(stream));
    });
}

int dcvc_rgb_to_x_cs(const void* src, long long row_stride, long long pixel_stride, long long channel_stride, int H_, int W_,
                     void* x, int ldx, void* planar, int matrix, int range, int yuv_bit_depth, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::rgb_to_x_cs(rgb_source(src, row_stride, pixel_stride, channel_stride, H_, W_, x, ldx, planar),
                          dcvc::ColourSpace{matrix, range, yuv_bit_depth}, S(stream));
    });
}

int dcvc_x_to_rgb_cs(const void* x_hat, int row_pixels, int H_, int W_, void* rgb16, void* rgb8, int matrix, int range,
                     int yuv_bit_depth, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::x_to_rgb_cs(H(x_hat), row_pixels, H_, W_, H(rgb16), static_cast<uint8_t*>(rgb8),
                          dcvc::ColourSpace{matrix, range, yuv_bit_depth}, S(stream));
    });
}

int dcvc_rgb16_to_x_cs(const void* src, long long row_stride, long long pixel_stride, long long channel_stride, int bit_depth, int H_,
                       int W_, void* x, int ldx, void* planar16, int matrix, int range, int yuv_bit_depth, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::Rgb16ToXDesc d;
        d.src = static_cast<const uint16_t*>(src);
        d.row_stride = row_stride; d.pixel_stride = pixel_stride; d.channel_stride = channel_stride;
        d.bit_depth = bit_depth; d.H = H_; d.W = W_; d.x = H(x); d.ldx = ldx; d.planar = static_cast<uint16_t*>(planar16);
        dcvc::rgb16_to_x_cs(d, dcvc::ColourSpace{matrix, range, yuv_bit_depth}, S(stream));
    });
}

int dcvc_x_to_rgb16_cs(const void* x_hat, int row_pixels, int H_, int W_, int bit_depth, void* dist32, void* rgb16u, int matrix,
                       int range, int yuv_bit_depth, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::x_to_rgb16_cs(H(x_hat), row_pixels, H_, W_, bit_depth, static_cast<float*>(dist32), static_cast<uint16_t*>(rgb16u),
                            dcvc::ColourSpace{matrix, range, yuv_bit_depth}, S(stream));
    });
}

int dcvc_sse(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_, int row_stride,
             long long plane_stride, double* out, void* stream)
{
    return dcvc::guarded([&] {
        const dcvc::SseDesc d = sse_desc(src, src_dtype, rec, rec_dtype, n_planes, H_, W_, row_stride, plane_stride, out);
        dcvc::sse_validate(d);         // before the workspace is sized: a bad geometry never reaches the allocator
        const AsyncBuf ws(dcvc::sse_workspace_bytes(n_planes, H_, W_), S(stream), "hipMallocAsync(sse workspace)");
        dcvc::sse(d, ws.p, S(stream));
    });
}

long long dcvc_sse_workspace_bytes(int n_planes, int H_, int W_)
{
    if (n_planes <= 0 || H_ <= 0 || W_ <= 0) return 0;
    return static_cast<long long>(dcvc::sse_workspace_bytes(n_planes, H_, W_));
}

int dcvc_sse_ws(const void* src, int src_dtype, const void* rec, int rec_dtype, int n_planes, int H_, int W_, int row_stride,
                long long plane_stride, double* out, void* workspace, long long workspace_bytes, void* stream)
{
    return dcvc::guarded([&] {
        const dcvc::SseDesc d = sse_desc(src, src_dtype, rec, rec_dtype, n_planes, H_, W_, row_stride, plane_stride, out);
        dcvc::sse_validate(d);
        if (workspace == nullptr || workspace_bytes < 0 ||
            static_cast<unsigned long long>(workspace_bytes) < dcvc::sse_workspace_bytes(n_planes, H_, W_)) {
            throw std::invalid_argument("sse: workspace missing or smaller than dcvc_sse_workspace_bytes");
        }
        dcvc::sse(d, workspace, S(stream));
    });
}

int dcvc_luma_sad(const void* x, int ldx, int H_, int W_, const void* prev_luma8, void* luma8_out, void* sad_out, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::LumaSadDesc d;
        d.x = H(x); d.ldx = ldx; d.H = H_; d.W = W_;
        d.prev = static_cast<const uint8_t*>(prev_luma8); d.luma = static_cast<uint8_t*>(luma8_out); d.sad = sad_out;
        dcvc::luma_sad(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_crc32_segments(const void* base, const long long* offsets, const long long* lengths, int n, void* crc_out, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::Crc32Desc d;
        d.base = base; d.offsets = offsets; d.lengths = lengths; d.n = n; d.out = crc_out;
        dcvc::crc32_segments(d, S(stream));      // validates before it enqueues anything
    });
}

uint32_t dcvc_crc32_combine(uint32_t crc_a, uint32_t crc_b, long long len_b)
{
    uint32_t crc = 0;
    dcvc::guarded([&] { crc = dcvc::crc32_combine(crc_a, crc_b, len_b); });
    return crc;
}

int dcvc_resample_ntaps(int n_in, int n_out) { return dcvc::resample_ntaps(n_in, n_out); }

int dcvc_resample_taps(int n_in, int n_out, int16_t* coef, int32_t* first)
{
    return dcvc::guarded([&] { dcvc::resample_taps(n_in, n_out, coef, first); });
}

int dcvc_resample_plan_create(int in_h, int in_w, int out_h, int out_w, void** plan)
{
    return dcvc::guarded([&] {
        if (plan == nullptr) throw std::invalid_argument("resample: null plan pointer");
        *plan = nullptr;
        *plan = dcvc::resample_plan_create(in_h, in_w, out_h, out_w);
    });
}

int dcvc_resample_plan_free(void* plan)
{
    return dcvc::guarded([&] { dcvc::resample_plan_free(static_cast<dcvc::ResamplePlan*>(plan)); });
}

long long dcvc_resample_workspace_bytes(const void* plan, int n_planes)
{
    if (plan == nullptr || n_planes < 1 || n_planes > 65535) return 0;
    return static_cast<long long>(dcvc::resample_workspace_bytes(*static_cast<const dcvc::ResamplePlan*>(plan), n_planes));
}

int dcvc_resample_planes(const void* plan, const void* src, int src_dtype, int src_row_stride, long long src_plane_stride, void* dst,
                         int dst_dtype, int dst_row_stride, long long dst_plane_stride, int n_planes, int max_val, void* workspace,
                         long long workspace_bytes, void* stream)
{
    return dcvc::guarded([&] {
        if (plan == nullptr) throw std::invalid_argument("resample: null plan");
        dcvc::ResampleDesc d;
        d.src = src; d.src_dtype = src_dtype; d.src_row_stride = src_row_stride; d.src_plane_stride = src_plane_stride;
        d.dst = dst; d.dst_dtype = dst_dtype; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.n_planes = n_planes; d.max_val = max_val; d.workspace = workspace; d.workspace_bytes = workspace_bytes;
        dcvc::resample_planes(*static_cast<const dcvc::ResamplePlan*>(plan), d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_denoise_planes(const void* src, int src_row_stride, long long src_plane_stride, const void* prev, int prev_row_stride,
                        long long prev_plane_stride, void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int bit_depth,
                        int H, int W, int n_planes, int spatial, int temporal, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::DenoiseDesc d;
        d.src = src; d.src_row_stride = src_row_stride; d.src_plane_stride = src_plane_stride;
        d.prev = prev; d.prev_row_stride = prev_row_stride; d.prev_plane_stride = prev_plane_stride;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.n_planes = n_planes; d.spatial = spatial; d.temporal = temporal;
        dcvc::denoise_planes(d, S(stream));      // validates before it enqueues anything
    });
}

long long dcvc_motion_search_workspace_bytes(int H, int W)
{
    if (H < 1 || W < 1 || H > dcvc::kMotionMaxSide || W > dcvc::kMotionMaxSide) return 0;
    return static_cast<long long>(dcvc::motion_search_workspace_bytes(H, W));
}

int dcvc_motion_search(const void* cur, int cur_row_stride, const void* ref, int ref_row_stride, int dtype, int bit_depth, int H, int W,
                       int range, int lambda, void* mv, int mv_bh, int mv_bw, void* sad, void* moved, void* workspace,
                       long long workspace_bytes, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::MotionSearchDesc d;
        d.cur = cur; d.cur_row_stride = cur_row_stride; d.ref = ref; d.ref_row_stride = ref_row_stride;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.range = range; d.lambda = lambda;
        d.mv = mv; d.mv_bh = mv_bh; d.mv_bw = mv_bw; d.sad = sad; d.moved = moved; d.workspace = workspace; d.workspace_bytes = workspace_bytes;
        dcvc::motion_search(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_motion_compensate_planes(const void* prev, int prev_row_stride, long long prev_plane_stride, void* dst, int dst_row_stride,
                                  long long dst_plane_stride, int dtype, int H, int W, int n_planes, int sx, int sy, const void* mv,
                                  int mv_bh, int mv_bw, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::MotionCompensateDesc d;
        d.prev = prev; d.prev_row_stride = prev_row_stride; d.prev_plane_stride = prev_plane_stride;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.dtype = dtype; d.H = H; d.W = W; d.n_planes = n_planes; d.sx = sx; d.sy = sy; d.mv = mv; d.mv_bh = mv_bh; d.mv_bw = mv_bw;
        dcvc::motion_compensate_planes(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_interp_select(const void* a, int a_row_stride, const void* b, int b_row_stride, int dtype, int bit_depth, int H, int W,
                       const void* mv, int mv_bh, int mv_bw, int k, int n, int limit, void* plan, void* wb, int plan_bh, int plan_bw,
                       void* sad, void* fallen, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::InterpSelectDesc d;
        d.a = a; d.a_row_stride = a_row_stride; d.b = b; d.b_row_stride = b_row_stride;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.mv = mv; d.mv_bh = mv_bh; d.mv_bw = mv_bw;
        d.k = k; d.n = n; d.limit = limit; d.plan = plan; d.wb = wb; d.plan_bh = plan_bh; d.plan_bw = plan_bw; d.sad = sad; d.fallen = fallen;
        dcvc::interp_select(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_interp_planes(const void* a, int a_row_stride, long long a_plane_stride, const void* b, int b_row_stride, long long b_plane_stride,
                       void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int H, int W, int n_planes, int sx, int sy,
                       const void* plan, const void* wb, int plan_bh, int plan_bw, int k, int n, const void* fallen, int n_blocks,
                       void* stream)
{
    return dcvc::guarded([&] {
        dcvc::InterpPlanesDesc d;
        d.a = a; d.a_row_stride = a_row_stride; d.a_plane_stride = a_plane_stride;
        d.b = b; d.b_row_stride = b_row_stride; d.b_plane_stride = b_plane_stride;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.dtype = dtype; d.H = H; d.W = W; d.n_planes = n_planes; d.sx = sx; d.sy = sy;
        d.plan = plan; d.wb = wb; d.plan_bh = plan_bh; d.plan_bw = plan_bw; d.k = k; d.n = n; d.fallen = fallen; d.n_blocks = n_blocks;
        dcvc::interp_planes(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_deinterlace_planes(const void* cur, int cur_row_stride, long long cur_plane_stride, const void* prev, int prev_row_stride,
                            long long prev_plane_stride, void* dst, int dst_row_stride, long long dst_plane_stride, int dtype,
                            int bit_depth, int H, int W, int n_planes, int keep, int weave_from_prev, int threshold, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::DeinterlaceDesc d;
        d.cur = cur; d.cur_row_stride = cur_row_stride; d.cur_plane_stride = cur_plane_stride;
        d.prev = prev; d.prev_row_stride = prev_row_stride; d.prev_plane_stride = prev_plane_stride;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.n_planes = n_planes;
        d.keep = keep; d.weave_from_prev = weave_from_prev; d.threshold = threshold;
        dcvc::deinterlace_planes(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_field_match(const void* cur, int cur_row_stride, const void* prev, int prev_row_stride, int dtype, int bit_depth, int H, int W,
                     int first, int cthresh, void* out8, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::FieldMatchDesc d;
        d.cur = cur; d.cur_row_stride = cur_row_stride; d.prev = prev; d.prev_row_stride = prev_row_stride;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.first = first; d.cthresh = cthresh; d.out8 = out8;
        dcvc::field_match(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_weave_fields(const void* a, int a_row_stride, long long a_plane_stride, const void* b, int b_row_stride, long long b_plane_stride,
                      void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int H, int W, int n_planes, int first, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::WeaveFieldsDesc d;
        d.a = a; d.a_row_stride = a_row_stride; d.a_plane_stride = a_plane_stride;
        d.b = b; d.b_row_stride = b_row_stride; d.b_plane_stride = b_plane_stride;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.dtype = dtype; d.H = H; d.W = W; d.n_planes = n_planes; d.first = first;
        dcvc::weave_fields(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_crop_stats(const void* luma, int row_stride, int dtype, int bit_depth, int H, int W, int limit, void* counts, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::CropStatsDesc d;
        d.luma = luma; d.row_stride = row_stride; d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.limit = limit;
        d.counts = counts;
        dcvc::crop_stats(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_window_planes(const void* src, int src_row_stride, long long src_plane_stride, int Hs, int Ws, void* dst, int dst_row_stride,
                       long long dst_plane_stride, int Hd, int Wd, int dtype, int n_planes, int ox, int oy, const int* fill, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::WindowPlanesDesc d;
        d.src = src; d.src_row_stride = src_row_stride; d.src_plane_stride = src_plane_stride; d.Hs = Hs; d.Ws = Ws;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride; d.Hd = Hd; d.Wd = Wd;
        d.dtype = dtype; d.n_planes = n_planes; d.ox = ox; d.oy = oy; d.fill = fill;
        dcvc::window_planes(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_grain_apply(const void* rec, int rec_row_stride, long long rec_plane_stride, const void* luma, int luma_row_stride, int Hl, int Wl,
                     void* dst, int dst_row_stride, long long dst_plane_stride, int dtype, int bit_depth, int H, int W, int n_planes,
                     int first_plane, int sx, int sy, const int16_t* template_y, const int16_t* template_u, const int16_t* template_v,
                     const uint8_t* lut, uint32_t seed, uint32_t pic, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::GrainApplyDesc d;
        d.rec = rec; d.rec_row_stride = rec_row_stride; d.rec_plane_stride = rec_plane_stride;
        d.luma = luma; d.luma_row_stride = luma_row_stride; d.Hl = Hl; d.Wl = Wl;
        d.dst = dst; d.dst_row_stride = dst_row_stride; d.dst_plane_stride = dst_plane_stride;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.n_planes = n_planes; d.first_plane = first_plane; d.sx = sx; d.sy = sy;
        d.templates[0] = template_y; d.templates[1] = template_u; d.templates[2] = template_v;
        d.lut = lut; d.seed = seed; d.pic = pic;
        dcvc::grain_apply(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_grain_stats(const void* src, int src_row_stride, long long src_plane_stride, const void* den, int den_row_stride,
                     long long den_plane_stride, const void* luma, int luma_row_stride, int Hl, int Wl, int dtype, int bit_depth, int H,
                     int W, int n_planes, int sx, int sy, int flat, int accumulate, void* words, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::GrainStatsDesc d;
        d.src = src; d.src_row_stride = src_row_stride; d.src_plane_stride = src_plane_stride;
        d.den = den; d.den_row_stride = den_row_stride; d.den_plane_stride = den_plane_stride;
        d.luma = luma; d.luma_row_stride = luma_row_stride; d.Hl = Hl; d.Wl = Wl;
        d.dtype = dtype; d.bit_depth = bit_depth; d.H = H; d.W = W; d.n_planes = n_planes; d.sx = sx; d.sy = sy;
        d.flat = flat; d.accumulate = accumulate; d.words = words;
        dcvc::grain_stats(d, S(stream));      // validates before it enqueues anything
    });
}

int dcvc_mask_step_enc(void* y, int ldy, const void* q_dec, int ldq, const void* scales, int lds,
                       const void* means, int ldm, void* y_hat, int ldh, void* sym, void* cond,
                       void* block_count, void* compact_out, void* totals, int Hh, int W, int C,
                       int nsteps, int step, float skip_thres, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::symbols_init();
        dcvc::MaskStepEnc d;
        d.y = H(y); d.ldy = ldy; d.q_dec = H(q_dec); d.ldq = ldq; d.scales = H(scales); d.lds = lds;
        d.means = H(means); d.ldm = ldm; d.y_hat = H(y_hat); d.ldh = ldh;
        d.sym = static_cast<int16_t*>(sym); d.cond = static_cast<uint8_t*>(cond);
        d.block_count = static_cast<int32_t*>(block_count);
        d.H = Hh; d.W = W; d.C = C; d.nsteps = nsteps; d.step = step; d.skip_thres = skip_thres;
        dcvc::mask_step_enc(d, S(stream));
        if (step == nsteps - 1) {
            dcvc::compact(sym, 2, d.cond, d.block_count, Hh * W * C, compact_out, static_cast<int32_t*>(totals), 0,
                          S(stream));
        }
    });
}

int dcvc_mask_dec_index(const void* scales, int lds, void* index, void* cond, void* block_count,
                        void* compact_out, void* totals, int Hh, int W, int C, float skip_thres, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::symbols_init();
        dcvc::MaskDecIndex d;
        d.scales = H(scales); d.lds = lds; d.index = static_cast<uint8_t*>(index);
        d.cond = static_cast<uint8_t*>(cond); d.block_count = static_cast<int32_t*>(block_count);
        d.H = Hh; d.W = W; d.C = C; d.skip_thres = skip_thres;
        dcvc::mask_dec_index(d, S(stream));
        dcvc::compact(index, 1, d.cond, d.block_count, Hh * W * C, compact_out, static_cast<int32_t*>(totals), 0,
                      S(stream));
    });
}

int dcvc_mask_step_dec(const void* decoded, const void* cond, const void* block_count, const void* totals,
                       void* yq, const void* means, int ldm, const void* q_dec, int ldq, void* y_hat, int ldh,
                       int Hh, int W, int C, int nsteps, int step, void* stream)
{
    return dcvc::guarded([&] {
        dcvc::MaskStepDec d;
        d.decoded = static_cast<const int8_t*>(decoded); d.cond = static_cast<const uint8_t*>(cond);
        d.block_count = static_cast<const int32_t*>(block_count); d.totals = static_cast<const int32_t*>(totals);
        d.yq = static_cast<int8_t*>(yq); d.means = H(means); d.ldm = ldm; d.q_dec = H(q_dec); d.ldq = ldq;
        d.y_hat = H(y_hat); d.ldh = ldh; d.H = Hh; d.W = W; d.C = C; d.nsteps = nsteps; d.step = step;
        dcvc::mask_step_dec(d, S(stream));
    });
}

int dcvc_dcb_tail_debug_buffer(void* device_buffer)
{
    return dcvc::guarded([&] { dcvc::dcb_tail_debug_buffer(static_cast<dcvc::half_t*>(device_buffer)); });
}

int dcvc_gemm_timeline_buffer(void* device_buffer)
{
    return dcvc::guarded([&] { dcvc::gemm_timeline_buffer(static_cast<long long*>(device_buffer)); });
}

int dcvc_dcb_nsplit_timeline_buffer(void* device_buffer)
{
    return dcvc::guarded([&] { dcvc::dcb_nsplit_timeline_buffer(static_cast<long long*>(device_buffer)); });
}

int dcvc_dcb_nsplit_dw_hook(const void* t1, const void* wdw, int width)
{
    return dcvc::guarded([&] {
        if (t1 != nullptr && (wdw == nullptr || width <= 0)) throw std::invalid_argument("dcb_nsplit_dw_hook: taps and a width");
        dcvc::dcb_nsplit_dw_hook(H(t1), H(wdw), width);
    });
}

int dcvc_round_z(const void* z, void* z_hat, void* z_i8, int count, void* stream)
{
    return dcvc::guarded([&] {
        check_b(1, {z, z_hat, z_i8}, {count}, "round_z");
        check_aligned({z, z_hat}, 2, "round_z");
        dcvc::round_z(H(z), H(z_hat), static_cast<int8_t*>(z_i8), count, S(stream));
    });
}

int dcvc_int8_to_half(const void* in, void* out, int count, void* stream)
{
    return dcvc::guarded([&] {
        check_b(1, {in, out}, {count}, "int8_to_half");
        check_aligned({out}, 2, "int8_to_half");
        dcvc::int8_to_half(static_cast<const int8_t*>(in), H(out), count, S(stream));
    });
}

int dcvc_symbol_blocks(int count)
{
    return dcvc::symbol_blocks(count);
}

namespace {

void y_step_enc_n(const char* what, const void* y, int ldy, const void* scales, int lds, const void* means, int ldm, void* y_hat_acc,
                  int ldacc, void* sym, void* cond, void* block_count, void* compact_out, long long out_stride, void* totals,
                  int totals_stride, int slot, int Hh, int W, int C, int step, float skip_thres, int n, void* stream)
{
    check_b(n, {y, scales, means, y_hat_acc, sym, cond, block_count, compact_out, totals}, {Hh, W, C}, what);
    check_y_step(n, Hh, W, C, step, slot, what);
    check_rows({{y, ldy}, {scales, lds}, {means, ldm}, {y_hat_acc, ldacc}}, C, what);
    check_aligned({sym}, 16, what);
    check_aligned({block_count, totals}, 4, what);
    check_aligned({compact_out}, 2, what);
    check_strides(n, out_stride, totals_stride, what);
    dcvc::symbols_init();
    dcvc::YStepEnc d;
    d.y = H(y); d.ldy = ldy; d.scales = H(scales); d.lds = lds; d.means = H(means); d.ldm = ldm;
    d.y_hat_acc = H(y_hat_acc); d.ldacc = ldacc;
    d.sym = static_cast<int16_t*>(sym); d.cond = static_cast<uint8_t*>(cond);
    d.block_count = static_cast<int32_t*>(block_count);
    d.H = Hh; d.W = W; d.C = C; d.step = step; d.skip_thres = skip_thres; d.first = (step == 0); d.n = n;
    dcvc::y_step_enc(d, S(stream));
    dcvc::compact_b(sym, 2, d.cond, d.block_count, Hh * W * (C / 4), compact_out, out_stride, static_cast<int32_t*>(totals),
                    totals_stride, slot, n, S(stream));
}

void y_step_dec_index_n(const char* what, const void* scales, int lds, void* index, void* cond, void* block_count, void* compact_out,
                        long long out_stride, void* totals, int totals_stride, int slot, int Hh, int W, int C, int step,
                        float skip_thres, int n, void* stream)
{
    check_b(n, {scales, index, cond, block_count, compact_out, totals}, {Hh, W, C}, what);
    check_y_step(n, Hh, W, C, step, slot, what);
    check_rows({{scales, lds}}, C, what);
    check_aligned({index}, 8, what);
    check_aligned({block_count, totals}, 4, what);
    check_strides(n, out_stride, totals_stride, what);
    dcvc::symbols_init();
    dcvc::YStepDecIndex d;
    d.scales = H(scales); d.lds = lds;
    d.index = static_cast<uint8_t*>(index); d.cond = static_cast<uint8_t*>(cond);
    d.block_count = static_cast<int32_t*>(block_count);
    d.H = Hh; d.W = W; d.C = C; d.step = step; d.skip_thres = skip_thres; d.n = n;
    dcvc::y_step_dec_index(d, S(stream));
    dcvc::compact_b(index, 1, d.cond, d.block_count, Hh * W * (C / 4), compact_out, out_stride, static_cast<int32_t*>(totals),
                    totals_stride, slot, n, S(stream));
}

void y_step_dec_restore_n(const char* what, const void* decoded, long long decoded_stride, const void* cond, const void* block_count,
                          const void* totals, int totals_stride, int slot, const void* means, int ldm, void* y_hat_acc, int ldacc,
                          int Hh, int W, int C, int step, int n, void* stream)
{
    check_b(n, {decoded, cond, block_count, totals, means, y_hat_acc}, {Hh, W, C}, what);
    check_y_step(n, Hh, W, C, step, slot, what);
    check_rows({{means, ldm}, {y_hat_acc, ldacc}}, C, what);
    check_aligned({block_count, totals}, 4, what);
    check_strides(n, decoded_stride, totals_stride, what);
    dcvc::YStepDecRestore d;
    d.decoded = static_cast<const int8_t*>(decoded);
    d.cond = static_cast<const uint8_t*>(cond);
    d.block_count = static_cast<const int32_t*>(block_count);
    d.totals = static_cast<const int32_t*>(totals); d.slot = slot;
    d.means = H(means); d.ldm = ldm; d.y_hat_acc = H(y_hat_acc); d.ldacc = ldacc;
    d.H = Hh; d.W = W; d.C = C; d.step = step; d.first = (step == 0);
    d.n = n; d.decoded_stride = decoded_stride; d.totals_stride = totals_stride;
    dcvc::y_step_dec_restore(d, S(stream));
}

}  // namespace

int dcvc_y_step_enc(const void* y, int ldy, const void* scales, int lds, const void* means, int ldm,
                    void* y_hat_acc, int ldacc, void* sym, void* cond, void* block_count,
                    void* compact_out, void* totals, int Hh, int W, int C, int step,
                    float skip_thres, void* stream)
{
    return dcvc::guarded([&] {
        y_step_enc_n("y_step_enc", y, ldy, scales, lds, means, ldm, y_hat_acc, ldacc, sym, cond, block_count, compact_out, 0, totals,
                     0, step, Hh, W, C, step, skip_thres, 1, stream);
    });
}

int dcvc_y_step_enc_b(const void* y, int ldy, const void* scales, int lds, const void* means, int ldm, void* y_hat_acc, int ldacc,
                      void* sym, void* cond, void* block_count, void* compact_out, long long out_stride, void* totals,
                      int totals_stride, int slot, int Hh, int W, int C, int step, float skip_thres, int n, void* stream)
{
    return dcvc::guarded([&] {
        y_step_enc_n("y_step_enc_b", y, ldy, scales, lds, means, ldm, y_hat_acc, ldacc, sym, cond, block_count, compact_out,
                     out_stride, totals, totals_stride, slot, Hh, W, C, step, skip_thres, n, stream);
    });
}

int dcvc_y_step_dec_index(const void* scales, int lds, void* index, void* cond, void* block_count,
                          void* compact_out, void* totals, int Hh, int W, int C, int step,
                          float skip_thres, void* stream)
{
    return dcvc::guarded([&] {
        y_step_dec_index_n("y_step_dec_index", scales, lds, index, cond, block_count, compact_out, 0, totals, 0, step, Hh, W, C,
                           step, skip_thres, 1, stream);
    });
}

int dcvc_y_step_dec_index_b(const void* scales, int lds, void* index, void* cond, void* block_count, void* compact_out,
                            long long out_stride, void* totals, int totals_stride, int slot, int Hh, int W, int C, int step,
                            float skip_thres, int n, void* stream)
{
    return dcvc::guarded([&] {
        y_step_dec_index_n("y_step_dec_index_b", scales, lds, index, cond, block_count, compact_out, out_stride, totals,
                           totals_stride, slot, Hh, W, C, step, skip_thres, n, stream);
    });
}

int dcvc_y_step_dec_restore(const void* decoded, const void* cond, const void* block_count,
                            const void* totals, const void* means, int ldm, void* y_hat_acc,
                            int ldacc, int Hh, int W, int C, int step, void* stream)
{
    return dcvc::guarded([&] {
        y_step_dec_restore_n("y_step_dec_restore", decoded, 0, cond, block_count, totals, 0, step, means, ldm, y_hat_acc, ldacc,
                             Hh, W, C, step, 1, stream);
    });
}

int dcvc_y_step_dec_restore_b(const void* decoded, long long decoded_stride, const void* cond, const void* block_count,
                              const void* totals, int totals_stride, int slot, const void* means, int ldm, void* y_hat_acc,
                              int ldacc, int Hh, int W, int C, int step, int n, void* stream)
{
    return dcvc::guarded([&] {
        y_step_dec_restore_n("y_step_dec_restore_b", decoded, decoded_stride, cond, block_count, totals, totals_stride, slot, means,
                             ldm, y_hat_acc, ldacc, Hh, W, C, step, n, stream);
    });
}

int dcvc_gemm_profile_enable(int on)
{
    return dcvc::guarded([&] { dcvc::gemm_profile_enable(on != 0); });
}

int dcvc_gemm_profile_reset(void)
{
    return dcvc::guarded([&] { dcvc::gemm_profile_reset(); });
}

int dcvc_gemm_profile_collect(double* ms, double* flops, long long* launches)
{
    return dcvc::guarded([&] { dcvc::gemm_profile_collect(ms, flops, launches); });
}

long long dcvc_gemm_profile_launches(void* records, long long cap)
{
    long long n = -1;
    dcvc::guarded([&] {
        n = static_cast<long long>(dcvc::gemm_profile_launches(static_cast<dcvc::GemmLaunchInfo*>(records),
                                                                 static_cast<size_t>(cap)));
    });
    return n;
}

// ---- code length (host tables: rans/code_length.cpp; sums: kernels/code_length.hip)
int dcvc_code_length_table(const int32_t* cdfs, int num_cdf, int stride, const int32_t* cdf_sizes, int cols, uint32_t* out)
{
    return dcvc::guarded([&] { dcvc::code_length_table(cdfs, num_cdf, stride, cdf_sizes, cols, out); });
}

uint32_t dcvc_code_length_cost(int freq, int bypass_groups)
{
    return dcvc::code_length_cost(freq, bypass_groups);
}

long long dcvc_predicted_stream_bytes(long long y_units, long long z_units, int ec_parallel)
{
    long long n = -1;
    dcvc::guarded([&] { n = dcvc::predicted_stream_bytes(y_units, z_units, ec_parallel); });
    return n;
}

int dcvc_code_length_y(const void* sym, long long sym_stride, const void* cond, long long cond_stride, const void* totals,
                       int totals_stride, int n_totals, int count, const void* table, int num_cdf, void* out, int n,
                       void* stream)
{
    return dcvc::guarded([&] {
        if (n < 1 || n > 65535 || out == nullptr) throw std::invalid_argument("code_length_y: bad batch size or null output");
        dcvc::CodeLengthY d;
        d.sym = static_cast<const int16_t*>(sym); d.sym_stride = sym_stride;
        d.cond = static_cast<const uint8_t*>(cond); d.cond_stride = cond_stride;
        d.totals = static_cast<const int32_t*>(totals); d.totals_stride = totals_stride; d.n_totals = n_totals;
        d.count = count; d.table = static_cast<const uint32_t*>(table); d.num_cdf = num_cdf;
        d.out = static_cast<unsigned long long*>(out); d.out_stride = 2; d.kept_slot = 1; d.n = n;
        dcvc::hip_check(hipMemsetAsync(out, 0, sizeof(unsigned long long) * 2 * n, S(stream)), "hipMemsetAsync(code length)");
        dcvc::code_length_y(d, S(stream));
    });
}

int dcvc_code_length_z(const void* z, int count, int ch, const void* table, void* out, int n, void* stream)
{
    return dcvc::guarded([&] {
        if (n < 1 || n > 65535 || out == nullptr) throw std::invalid_argument("code_length_z: bad batch size or null output");
        dcvc::CodeLengthZ d;
        d.z = static_cast<const int8_t*>(z); d.count = count; d.ch = ch;
        d.table = static_cast<const uint32_t*>(table);
        d.out = static_cast<unsigned long long*>(out); d.out_stride = 1; d.n = n;
        dcvc::hip_check(hipMemsetAsync(out, 0, sizeof(unsigned long long) * n, S(stream)), "hipMemsetAsync(code length)");
        dcvc::code_length_z(d, S(stream));
    });
}

}  // extern "C"
