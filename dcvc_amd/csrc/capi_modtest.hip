// TEST SURFACE (include/dcvc_amd_modtest.h): the module layer of codec/modules.h behind a C ABI, for tests/test_modules_gpu.py.
// Nothing in the product calls it. Every *_forward entry only forwards its arguments: no allocation, no synchronisation.
#include "capi_common.h"
#include <deque>
#include <memory>
#include <stdexcept>
#include <vector>
#include "dcvc_amd_modtest.h"
#include "codec/modules.h"

using dcvc::DcbW;
using dcvc::FinCall;
using dcvc::View;
using dcvc::half_t;

struct dcvc_modtest {
    enum Kind { kBlocks, kChain, kStride2, kUpsample, kSubpel, kFin };
    struct Module {
        Kind kind = kBlocks;
        std::vector<DcbW> blocks;      // kBlocks
        dcvc::DcbChain chain;          // kChain
        dcvc::Stride2W s2;
        dcvc::UpsampleW up;
        dcvc::SubpelW sp;
        dcvc::FinW fin;
    };
    dcvc::ParamStore ps;
    dcvc::DeviceArena mem;
    dcvc::Scratch s;
    half_t* zeros = nullptr;
    std::deque<Module> modules;        // (a deque: blocks are named by pointer across calls)

    Module& module(int m)
    {
        if (m < 0 || m >= static_cast<int>(modules.size())) throw std::invalid_argument("modtest: no such module");
        return modules[m];
    }
    const std::vector<DcbW>* array(Module& mod)
    {
        return mod.kind == kBlocks ? &mod.blocks : mod.kind == kChain ? &mod.chain.blocks : nullptr;
    }
    // (module, index) -> block; module < 0: none
    const DcbW* block(int m, int i)
    {
        if (m < 0) return nullptr;
        Module& mod = module(m);
        if (mod.kind == kStride2 && i == 0) return &mod.s2.block;
        if (mod.kind == kUpsample && i == 0) return &mod.up.block;
        const std::vector<DcbW>* a = array(mod);
        if (a == nullptr || i < 0 || i >= static_cast<int>(a->size())) throw std::invalid_argument("modtest: no such block");
        return &(*a)[i];
    }
    const dcvc::FinW* fin(int m)
    {
        if (m < 0) return nullptr;
        Module& mod = module(m);
        if (mod.kind != kFin) throw std::invalid_argument("modtest: module is not a closing conv");
        return &mod.fin;
    }
};

namespace {

inline half_t* H(void* p) { return static_cast<half_t*>(p); }
inline const half_t* H(const void* p) { return static_cast<const half_t*>(p); }
inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }
inline View V(void* p, int ld, int c) { return p == nullptr ? View() : View(H(p), ld, c); }

// FinCall as the codecs build it (null: no closing conv)
bool make_fin(dcvc_modtest* h, int fin_module, const void* q, void* y, int ldy, int keep, FinCall* out)
{
    const dcvc::FinW* w = h->fin(fin_module);
    if (w == nullptr) return false;
    *out = FinCall(*w, H(y), ldy, H(q));
    out->keep_block_output = keep != 0;
    return true;
}

}  // namespace

extern "C" {

dcvc_modtest* dcvc_modtest_create(long long scratch_elems, int batch)
{
    dcvc_modtest* h = nullptr;
    const int rc = dcvc::guarded([&] {
        if (scratch_elems <= 0 || batch < 1) throw std::invalid_argument("modtest: scratch_elems and batch must be positive");
        dcvc::kernels_init();
        std::unique_ptr<dcvc_modtest> p(new dcvc_modtest);
        p->s.elems = static_cast<size_t>(scratch_elems);
        p->s.batch = batch;
        p->s.t1 = p->mem.alloc_half(p->s.elems);
        p->s.t2 = p->mem.alloc_half(p->s.elems);
        p->s.t3 = p->mem.alloc_half(p->s.elems);
        p->zeros = p->mem.alloc_half(2048);
        h = p.release();
    });
    return rc == 0 ? h : nullptr;
}

void dcvc_modtest_destroy(dcvc_modtest* h)
{
    if (h == nullptr) return;
    (void)hipDeviceSynchronize();
    delete h;
}

int dcvc_modtest_set_param(dcvc_modtest* h, const char* name, const void* data, int dtype, const int64_t* dims, int ndim)
{
    return dcvc::guarded([&] { h->ps.add(name, data, dtype, dims, ndim); });
}

int dcvc_modtest_load_blocks(dcvc_modtest* h, const char* prefix, int n)
{
    int id = -1;
    const int rc = dcvc::guarded([&] {
        h->modules.emplace_back();
        dcvc_modtest::Module& m = h->modules.back();
        const std::string p(prefix);
        if (n == 0) {
            m.kind = dcvc_modtest::kChain;
            m.chain.load(h->ps, h->mem, p);
        } else if (n < 0) {
            m.blocks.resize(1);
            m.blocks[0].load(h->ps, h->mem, p);
        } else {
            m.blocks.resize(n);
            for (int i = 0; i < n; ++i) m.blocks[i].load(h->ps, h->mem, p + std::to_string(i) + ".");
        }
        id = static_cast<int>(h->modules.size()) - 1;
    });
    return rc == 0 ? id : rc;
}

int dcvc_modtest_load_stride2(dcvc_modtest* h, const char* prefix, int shortcut)
{
    int id = -1;
    const int rc = dcvc::guarded([&] {
        h->modules.emplace_back();
        h->modules.back().kind = dcvc_modtest::kStride2;
        h->modules.back().s2.load(h->ps, h->mem, prefix, shortcut != 0);
        id = static_cast<int>(h->modules.size()) - 1;
    });
    return rc == 0 ? id : rc;
}

int dcvc_modtest_load_upsample(dcvc_modtest* h, const char* prefix, int shortcut)
{
    int id = -1;
    const int rc = dcvc::guarded([&] {
        h->modules.emplace_back();
        h->modules.back().kind = dcvc_modtest::kUpsample;
        h->modules.back().up.load(h->ps, h->mem, prefix, shortcut != 0);
        id = static_cast<int>(h->modules.size()) - 1;
    });
    return rc == 0 ? id : rc;
}

int dcvc_modtest_load_subpel(dcvc_modtest* h, const char* prefix)
{
    int id = -1;
    const int rc = dcvc::guarded([&] {
        h->modules.emplace_back();
        h->modules.back().kind = dcvc_modtest::kSubpel;
        h->modules.back().sp.load(h->ps, h->mem, prefix);
        id = static_cast<int>(h->modules.size()) - 1;
    });
    return rc == 0 ? id : rc;
}

int dcvc_modtest_load_fin(dcvc_modtest* h, const char* prefix)
{
    int id = -1;
    const int rc = dcvc::guarded([&] {
        h->modules.emplace_back();
        h->modules.back().kind = dcvc_modtest::kFin;
        h->modules.back().fin.load(h->ps, h->mem, prefix);
        id = static_cast<int>(h->modules.size()) - 1;
    });
    return rc == 0 ? id : rc;
}

int dcvc_modtest_blocks(dcvc_modtest* h, int module)
{
    int n = -1;
    const int rc = dcvc::guarded([&] {
        dcvc_modtest::Module& m = h->module(module);
        const std::vector<DcbW>* a = h->array(m);
        n = a != nullptr ? static_cast<int>(a->size())
                         : (m.kind == dcvc_modtest::kStride2 || m.kind == dcvc_modtest::kUpsample) ? 1 : 0;
    });
    return rc == 0 ? n : rc;
}

int dcvc_modtest_block_info(dcvc_modtest* h, int module, int index, int Hh, int W, int next_module, int next_index, int* out)
{
    return dcvc::guarded([&] {
        const DcbW* b = h->block(module, index);
        if (b == nullptr || out == nullptr) throw std::invalid_argument("modtest: block_info needs a block and an output");
        const DcbW* next = h->block(next_module, next_index);
        out[0] = b->nsplit();
        out[1] = b->packed_adaptor != nullptr;
        out[2] = b->one_launch(Hh, W);
        out[3] = next != nullptr && b->feeds(*next);
        out[4] = b->c; out[5] = b->cdc; out[6] = b->cffn;
        out[7] = b->has_adaptor ? b->adaptor.cin : 0;
    });
}

int dcvc_modtest_fin_info(dcvc_modtest* h, int module, int* out)
{
    return dcvc::guarded([&] {
        const dcvc::FinW* f = h->fin(module);
        if (f == nullptr || out == nullptr) throw std::invalid_argument("modtest: fin_info needs a closing conv and an output");
        out[0] = f->packed != nullptr; out[1] = f->conv.cin; out[2] = f->conv.cout;
    });
}

long long dcvc_modtest_read(dcvc_modtest* h, int module, int index, int what, void* dst, long long cap)
{
    long long count = -1;
    const int rc = dcvc::guarded([&] {
        const half_t* src = nullptr;
        if (what == DCVC_MODTEST_TAPS || what == DCVC_MODTEST_FOLDED) {
            const DcbW* b = h->block(module, index);
            if (b == nullptr) throw std::invalid_argument("modtest: read needs a block");
            src = what == DCVC_MODTEST_TAPS ? b->dw : b->dc3.b;
            count = what == DCVC_MODTEST_TAPS ? 9LL * b->cdc : b->c;
        } else if (what == DCVC_MODTEST_STRIDE2) {
            dcvc_modtest::Module& m = h->module(module);
            if (m.kind != dcvc_modtest::kStride2) throw std::invalid_argument("modtest: module is not a stride-2 block");
            src = m.s2.w;
            count = 4LL * m.s2.cout * m.s2.cin;
        } else if (what == DCVC_MODTEST_SUBPEL) {
            dcvc_modtest::Module& m = h->module(module);
            if (m.kind != dcvc_modtest::kSubpel && m.kind != dcvc_modtest::kUpsample) {
                throw std::invalid_argument("modtest: module has no sub-pixel conv");
            }
            const dcvc::SubpelW& sp = m.kind == dcvc_modtest::kSubpel ? m.sp : m.up.up;
            src = sp.w;
            count = 4LL * sp.cout * sp.cin * sp.k * sp.k;
        } else {
            throw std::invalid_argument("modtest: unknown tensor");
        }
        const long long n = count < cap ? count : cap;
        if (n > 0) {
            if (dst == nullptr) throw std::invalid_argument("modtest: null destination");
            dcvc::hip_check(hipMemcpy(dst, src, static_cast<size_t>(n) * sizeof(half_t), hipMemcpyDeviceToHost), "hipMemcpy(read)");
        }
    });
    return rc == 0 ? count : rc;
}

int dcvc_modtest_scratch(dcvc_modtest* h, void** t1, void** t2, void** t3, int* hand)
{
    return dcvc::guarded([&] {
        if (t1 != nullptr) *t1 = h->s.t1;
        if (t2 != nullptr) *t2 = h->s.t2;
        if (t3 != nullptr) *t3 = h->s.t3;
        if (hand != nullptr) *hand = h->s.hand;
    });
}

int dcvc_modtest_block_forward(dcvc_modtest* h, int module, int index, void* x, int ldx, int cx, void* y, int ldy, int cy,
                               int Hh, int W, int shortcut, const void* q_fused, const void* q_after,
                               void* alt, int ldalt, int calt, int next_module, int next_index, int dc0_done,
                               int fin_module, const void* fin_q, void* fin_y, int fin_ldy, int keep_block_output, void* stream)
{
    return dcvc::guarded([&] {
        const DcbW* b = h->block(module, index);
        if (b == nullptr) throw std::invalid_argument("modtest: block_forward needs a block");
        FinCall fin;
        const bool has_fin = make_fin(h, fin_module, fin_q, fin_y, fin_ldy, keep_block_output, &fin);
        dcvc::DcbCall c;
        c.shortcut = shortcut != 0; c.q_fused = H(q_fused); c.q_after = H(q_after); c.alt = V(alt, ldalt, calt);
        c.next = h->block(next_module, next_index); c.dc0_done = dc0_done != 0; c.fin = has_fin ? &fin : nullptr;
        b->forward(V(x, ldx, cx), V(y, ldy, cy), Hh, W, h->s, S(stream), c);
    });
}

int dcvc_modtest_chain_forward_qa(dcvc_modtest* h, int module, int first, int n, void* x, int ldx, int cx,
                                  void* tmp, int ldtmp, int ctmp, void* y, int ldy, int cy, int Hh, int W,
                                  const void* q_fused_last, const void* q_after_last, void* tmp2, int ldtmp2, int ctmp2,
                                  int fin_module, const void* fin_q, void* fin_y, int fin_ldy, int keep_block_output,
                                  int after_module, int after_index, int first_dc0_done, void* stream)
{
    return dcvc::guarded([&] {
        dcvc_modtest::Module& m = h->module(module);
        const std::vector<DcbW>* a = h->array(m);
        if (a == nullptr) throw std::invalid_argument("modtest: module is not a chain of blocks");
        const int total = static_cast<int>(a->size());
        const int count = n == 0 ? total - first : n;
        if (first < 0 || count < 1 || first + count > total) throw std::invalid_argument("modtest: no such range of blocks");
        FinCall fin;
        const bool has_fin = make_fin(h, fin_module, fin_q, fin_y, fin_ldy, keep_block_output, &fin);
        dcvc::ChainCall c;
        c.q_fused_last = H(q_fused_last); c.q_after_last = H(q_after_last); c.tmp2 = V(tmp2, ldtmp2, ctmp2);
        c.fin = has_fin ? &fin : nullptr; c.after = h->block(after_module, after_index); c.first_dc0_done = first_dc0_done != 0;
        if (m.kind == dcvc_modtest::kChain && first == 0 && count == total) {
            m.chain.forward(V(x, ldx, cx), V(tmp, ldtmp, ctmp), V(y, ldy, cy), Hh, W, h->s, S(stream), c);
            return;
        }
        dcvc::run_dcb_chain(a->data() + first, count, V(x, ldx, cx), V(tmp, ldtmp, ctmp), V(y, ldy, cy), Hh, W, h->s, S(stream), c);
    });
}

int dcvc_modtest_chain_forward(dcvc_modtest* h, int module, int first, int n, void* x, int ldx, int cx,
                               void* tmp, int ldtmp, int ctmp, void* y, int ldy, int cy, int Hh, int W,
                               const void* q_fused_last, void* tmp2, int ldtmp2, int ctmp2,
                               int fin_module, const void* fin_q, void* fin_y, int fin_ldy, int keep_block_output,
                               int after_module, int after_index, int first_dc0_done, void* stream)
{
    return dcvc_modtest_chain_forward_qa(h, module, first, n, x, ldx, cx, tmp, ldtmp, ctmp, y, ldy, cy, Hh, W, q_fused_last, nullptr,
                                         tmp2, ldtmp2, ctmp2, fin_module, fin_q, fin_y, fin_ldy, keep_block_output, after_module,
                                         after_index, first_dc0_done, stream);
}

int dcvc_modtest_stride2_forward(dcvc_modtest* h, int module, void* x, int ldx, int cx, void* tmp, int ldtmp, int ctmp,
                                 void* y, int ldy, int cy, int Hh, int W, void* stream)
{
    return dcvc::guarded([&] {
        dcvc_modtest::Module& m = h->module(module);
        if (m.kind != dcvc_modtest::kStride2) throw std::invalid_argument("modtest: module is not a stride-2 block");
        m.s2.forward(V(x, ldx, cx), V(tmp, ldtmp, ctmp), V(y, ldy, cy), Hh, W, h->zeros, h->s, S(stream));
    });
}

int dcvc_modtest_upsample_forward(dcvc_modtest* h, int module, void* x, int ldx, int cx, void* tmp, int ldtmp, int ctmp,
                                  void* y, int ldy, int cy, int Hh, int W, void* up_tmp, int with_zeros,
                                  int next_module, int next_index, void* stream)
{
    return dcvc::guarded([&] {
        dcvc_modtest::Module& m = h->module(module);
        if (m.kind != dcvc_modtest::kUpsample) throw std::invalid_argument("modtest: module is not an up-sampling block");
        m.up.forward(V(x, ldx, cx), V(tmp, ldtmp, ctmp), V(y, ldy, cy), Hh, W, h->s, S(stream), H(up_tmp),
                     with_zeros != 0 ? h->zeros : nullptr, h->block(next_module, next_index));
    });
}

int dcvc_modtest_subpel_forward(dcvc_modtest* h, int module, void* x, int ldx, int cx, void* y, int ldy, int cy, int Hh, int W,
                                void* up_tmp, int with_zeros, int n, void* stream)
{
    return dcvc::guarded([&] {
        dcvc_modtest::Module& m = h->module(module);
        if (m.kind != dcvc_modtest::kSubpel) throw std::invalid_argument("modtest: module is not a sub-pixel conv");
        m.sp.forward(V(x, ldx, cx), V(y, ldy, cy), Hh, W, S(stream), H(up_tmp), with_zeros != 0 ? h->zeros : nullptr, n);
    });
}

long long dcvc_modtest_pack_stream(int kind, const void* w0, const void* w1, const void* w2, int a, int b, void* out, long long cap,
                                   void* stream)
{
    long long halves = -1;
    const int rc = dcvc::guarded([&] {
        dcvc::kernels_init();
        if (!w0 || !out || (kind == DCVC_MODTEST_PACK_MAIN && (!w1 || !w2))) throw std::invalid_argument("modtest: missing operand");
        size_t n = 0;
        switch (kind) {
        case DCVC_MODTEST_PACK_MAIN: n = dcvc::dcb_nsplit_main_halves(a, b); break;
        case DCVC_MODTEST_PACK_DC0: n = dcvc::dcb_nsplit_dc0_halves(a, b); break;
        case DCVC_MODTEST_PACK_FIN: n = dcvc::dcb_nsplit_fin_halves(a, b); break;
        case DCVC_MODTEST_PACK_ADAPTOR: n = dcvc::dcb_pair_adaptor_halves(a, b); break;
        default: throw std::invalid_argument("modtest: no such stream kind");
        }
        if (static_cast<long long>(n) > cap) throw std::invalid_argument("modtest: the stream does not fit the buffer");
        switch (kind) {
        case DCVC_MODTEST_PACK_MAIN: dcvc::dcb_nsplit_pack_main(H(w0), H(w1), H(w2), a, b, H(out), S(stream)); break;
        case DCVC_MODTEST_PACK_DC0: dcvc::dcb_nsplit_pack_dc0(H(w0), a, b, H(out), S(stream)); break;
        case DCVC_MODTEST_PACK_FIN: dcvc::dcb_nsplit_pack_fin(H(w0), a, b, H(out), S(stream)); break;
        default: dcvc::dcb_pair_pack_adaptor(H(w0), a, b, H(out), S(stream)); break;
        }
        halves = static_cast<long long>(n);
    });
    return rc == 0 ? halves : -1;
}

}  // extern "C"
