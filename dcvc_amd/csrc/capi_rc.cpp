// C ABI of the rate control (include/dcvc_amd_rc.h).
#include "capi_common.h"
#include "codec/grain.h"
#include "codec/rate_control.h"
#include "dcvc_amd_rc.h"

#include <stdexcept>

struct dcvc_rc {
    dcvc::TargetBpp ctl;
};

struct dcvc_rc_vbv {
    dcvc::Vbv vbv;
};

struct dcvc_scd {
    dcvc::SceneCut scd;
};

struct dcvc_ivtc {
    dcvc::Ivtc ivtc;
};

struct dcvc_cropdet {
    dcvc::CropDetect det;
};

extern "C" {

dcvc_rc* dcvc_rc_create(double target_bpp, double pixels_per_picture, double qp0, int horizon, int intra_bonus,
                        int qp_min, int qp_max, double slope)
{
    dcvc_rc* rc = nullptr;
    dcvc::guarded([&] {
        rc = new dcvc_rc{dcvc::TargetBpp(target_bpp, pixels_per_picture, qp0, horizon, intra_bonus, qp_min, qp_max, slope)};
    });
    return rc;
}

void dcvc_rc_destroy(dcvc_rc* rc)
{
    delete rc;
}

int dcvc_rc_next_qp(const dcvc_rc* rc, int is_intra)
{
    int qp = -1;
    const int e = dcvc::guarded([&] {
        if (rc == nullptr) throw std::invalid_argument("null rate controller");
        qp = rc->ctl.next_qp(is_intra != 0);
    });
    return e < 0 ? e : qp;
}

int dcvc_rc_update(dcvc_rc* rc, double bits, int pictures, int is_intra)
{
    return dcvc::guarded([&] {
        if (rc == nullptr) throw std::invalid_argument("null rate controller");
        rc->ctl.update(bits, pictures, is_intra != 0);
    });
}

int dcvc_rc_update_at(dcvc_rc* rc, double bits, int pictures, int is_intra, int qp)
{
    return dcvc::guarded([&] {
        if (rc == nullptr) throw std::invalid_argument("null rate controller");
        rc->ctl.update_at(bits, pictures, is_intra != 0, qp);
    });
}

double dcvc_rc_state_qp(const dcvc_rc* rc)
{
    return rc ? rc->ctl.qp() : -1.0;
}

dcvc_rc_vbv* dcvc_rc_vbv_create(double maxrate_bpp, double bufsize_pictures, double init, long long pixels)
{
    dcvc_rc_vbv* v = nullptr;
    dcvc::guarded([&] { v = new dcvc_rc_vbv{dcvc::Vbv(maxrate_bpp, bufsize_pictures, init, pixels)}; });
    return v;
}

void dcvc_rc_vbv_destroy(dcvc_rc_vbv* v)
{
    delete v;
}

int64_t dcvc_rc_vbv_available(const dcvc_rc_vbv* v)
{
    int64_t avail = -1;
    const int e = dcvc::guarded([&] {
        if (v == nullptr) throw std::invalid_argument("null vbv model");
        avail = v->vbv.available();
    });
    return e < 0 ? e : avail;
}

int dcvc_rc_vbv_admit(dcvc_rc_vbv* v, int64_t bits, int pictures)
{
    int violated = 0;
    const int e = dcvc::guarded([&] {
        if (v == nullptr) throw std::invalid_argument("null vbv model");
        violated = v->vbv.admit(bits, pictures) ? 1 : 0;
    });
    return e < 0 ? e : violated;
}

double dcvc_rc_vbv_fullness(const dcvc_rc_vbv* v)
{
    return v ? v->vbv.fullness() : -1.0;
}

double dcvc_rc_vbv_capacity(const dcvc_rc_vbv* v)
{
    return v ? v->vbv.capacity() : -1.0;
}

double dcvc_rc_vbv_rate(const dcvc_rc_vbv* v)
{
    return v ? v->vbv.rate() : -1.0;
}

int64_t dcvc_rc_vbv_underflow(const dcvc_rc_vbv* v)
{
    return v ? v->vbv.underflow() : -1;
}

int dcvc_rc_pick_qp_for_budget(dcvc_rc_estimate_fn estimate, void* user, int64_t budget_bits, int qp_min, int qp_max,
                               int* probes)
{
    int qp = -1;
    const int e = dcvc::guarded([&] {
        if (estimate == nullptr) throw std::invalid_argument("pick_qp_for_budget: null estimate");
        qp = dcvc::pick_qp_for_budget([&](int q) { return estimate(q, user); }, budget_bits, qp_min, qp_max, probes);
    });
    return e < 0 ? e : qp;
}

int dcvc_rc_pick_qp_near(dcvc_rc_estimate_fn estimate, void* user, int64_t budget_bits, int start, int qp_min, int qp_max,
                         int* probes)
{
    int qp = -1;
    const int e = dcvc::guarded([&] {
        if (estimate == nullptr) throw std::invalid_argument("pick_qp_near: null estimate");
        qp = dcvc::pick_qp_near([&](int q) { return estimate(q, user); }, budget_bits, start, qp_min, qp_max, probes);
    });
    return e < 0 ? e : qp;
}

int dcvc_rc_pick_qp_for_quality(dcvc_rc_quality_fn measure, void* user, double target, int start, int qp_min, int qp_max,
                                int* trials)
{
    int qp = -1;
    const int e = dcvc::guarded([&] {
        if (measure == nullptr) throw std::invalid_argument("pick_qp_for_quality: null measure");
        qp = dcvc::pick_qp_for_quality([&](int q) { return measure(q, user); }, target, start, qp_min, qp_max, trials);
    });
    return e < 0 ? e : qp;
}

int64_t dcvc_rc_unit_budget_bits(double target_bpp, double pixels_per_picture, int pictures_coded, int64_t spent_bits, int horizon,
                                 int n)
{
    int64_t bits = -1;
    const int e = dcvc::guarded([&] {
        bits = dcvc::unit_budget_bits(target_bpp, pixels_per_picture, pictures_coded, spent_bits, horizon, n);
    });
    return e < 0 ? e : bits;
}

int64_t dcvc_rc_intra_budget_bits(double target_bpp, double pixels_per_picture, int k, int64_t spent_bits)
{
    return dcvc::intra_budget_bits(target_bpp, pixels_per_picture, k, spent_bits);
}

dcvc_scd* dcvc_scd_create(double threshold, int min_gap, long long pixels)
{
    dcvc_scd* s = nullptr;
    dcvc::guarded([&] { s = new dcvc_scd{dcvc::SceneCut(threshold, min_gap, pixels)}; });
    return s;
}

void dcvc_scd_destroy(dcvc_scd* s)
{
    delete s;
}

int dcvc_scd_push(dcvc_scd* s, int idx, long long sad, int scheduled_intra)
{
    int intra = 0;
    const int e = dcvc::guarded([&] {
        if (s == nullptr) throw std::invalid_argument("null scene-cut detector");
        intra = s->scd.push(idx, sad, scheduled_intra != 0) ? 1 : 0;
    });
    return e < 0 ? e : intra;
}

int dcvc_scd_last(const dcvc_scd* s, double* mafd, double* score, int* detected)
{
    return dcvc::guarded([&] {
        if (s == nullptr) throw std::invalid_argument("null scene-cut detector");
        if (mafd) *mafd = s->scd.mafd();
        if (score) *score = s->scd.score();
        if (detected) *detected = s->scd.detected() ? 1 : 0;
    });
}

dcvc_ivtc* dcvc_ivtc_create(int cycle, int mi)
{
    dcvc_ivtc* t = nullptr;
    dcvc::guarded([&] { t = new dcvc_ivtc{dcvc::Ivtc(cycle, mi)}; });
    return t;
}

void dcvc_ivtc_destroy(dcvc_ivtc* t)
{
    delete t;
}

int dcvc_ivtc_push(dcvc_ivtc* t, int idx, int has_prev, const uint64_t m[8])
{
    int r = 0;
    const int e = dcvc::guarded([&] {
        if (t == nullptr) throw std::invalid_argument("null ivtc handle");
        r = t->ivtc.push(idx, has_prev != 0, m);
    });
    return e < 0 ? e : r;
}

int dcvc_ivtc_drop(const dcvc_ivtc* t)
{
    return t ? t->ivtc.drop() : -1;
}

dcvc_cropdet* dcvc_cropdet_create(int H, int W, int frac, int min_bar, int ax, int ay)
{
    dcvc_cropdet* t = nullptr;
    dcvc::guarded([&] { t = new dcvc_cropdet{dcvc::CropDetect(H, W, frac, min_bar, ax, ay)}; });
    return t;
}

void dcvc_cropdet_destroy(dcvc_cropdet* t)
{
    delete t;
}

int dcvc_cropdet_push(dcvc_cropdet* t, const uint32_t* counts)
{
    int r = 0;
    const int e = dcvc::guarded([&] {
        if (t == nullptr) throw std::invalid_argument("null cropdet handle");
        r = t->det.push(counts) ? 1 : 0;
    });
    return e < 0 ? e : r;
}

int dcvc_cropdet_result(const dcvc_cropdet* t, int* x, int* y, int* w, int* h)
{
    int r = 0;
    const int e = dcvc::guarded([&] {
        if (t == nullptr || x == nullptr || y == nullptr || w == nullptr || h == nullptr) throw std::invalid_argument("cropdet: null operand");
        r = t->det.result(*x, *y, *w, *h);
    });
    return e < 0 ? e : r;
}

int dcvc_grain_template(uint32_t seed, int plane, int size, int16_t* out)
{
    return dcvc::guarded([&] { dcvc::grain_template(seed, plane, size, out); });
}

int dcvc_grain_fit(const uint64_t* words, int bit_depth, int gain_percent, long long min_count, uint8_t* lut_out)
{
    return dcvc::guarded([&] { dcvc::grain_fit(words, bit_depth, gain_percent, min_count, lut_out); });
}

}  // extern "C"
