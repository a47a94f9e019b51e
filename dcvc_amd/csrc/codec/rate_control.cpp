// See rate_control.h; dcvc_amd/rate_control.py has the reasoning behind every step of the controller.
#include "codec/rate_control.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

namespace dcvc {

TargetBpp::TargetBpp(double target_bpp, double pixels_per_picture, double qp0, int horizon, int intra_bonus, int qp_min,
                     int qp_max, double slope)
    : m_target_bits(target_bpp * pixels_per_picture), m_qp(qp0), m_slope(slope), m_horizon(std::max(1, horizon)),
      m_intra_bonus(intra_bonus), m_qp_min(qp_min), m_qp_max(qp_max)
{
    if (!(target_bpp > 0) || !(pixels_per_picture > 0)) {
        throw std::invalid_argument("target_bpp and pixels_per_picture must be positive");
    }
}

int TargetBpp::next_qp(bool is_intra) const
{
    const double q = m_qp + (is_intra ? m_intra_bonus : 0);
    const double r = std::rint(q);                                  // half to even, as Python's round()
    return static_cast<int>(std::min<double>(m_qp_max, std::max<double>(m_qp_min, r)));
}

void TargetBpp::update(double bits, int pictures, bool is_intra)
{
    update(bits, pictures, is_intra, next_qp(is_intra));
}

void TargetBpp::update_at(double bits, int pictures, bool is_intra, int qp)
{
    update(bits, pictures, is_intra, qp);
}

void TargetBpp::update(double bits, int pictures, bool is_intra, int used_qp)
{
    if (pictures <= 0) return;
    const bool moved = !is_intra && used_qp != next_qp(false);      // coded at another q_index than the controller's
    m_spent += bits;
    m_pictures += pictures;
    double per_picture = std::max(bits / pictures, 1.0);
    if (!is_intra) {
        if (m_has_last && used_qp != m_last_qp) {
            const double s = (std::log2(per_picture) - m_last_log) / (used_qp - m_last_qp);
            if (0.005 < s && s < 0.5) m_slope = 0.75 * m_slope + 0.25 * s;
        }
        m_has_last = true;
        m_last_qp = used_qp;
        m_last_log = std::log2(per_picture);
    }
    const double budget = m_target_bits * (m_pictures + m_horizon) - m_spent;
    const double want = std::max(budget / m_horizon, m_target_bits / 64.0);
    if (is_intra) {
        if (!m_has_last) return;
        per_picture = std::pow(2.0, m_last_log + m_slope * (m_qp - m_last_qp));
    } else if (moved) {
        per_picture = std::pow(2.0, m_last_log + m_slope * (m_qp - m_last_qp));      // the unit just stored, at the controller's q_index
    }
    const double step = (std::log2(want) - std::log2(per_picture)) / m_slope;
    m_qp += std::min(m_max_step, std::max(-m_max_step, step));
    m_qp = std::min(static_cast<double>(m_qp_max), std::max(static_cast<double>(m_qp_min), m_qp));
}

int pick_qp_for_budget(const std::function<int64_t(int)>& estimate, int64_t budget_bits, int qp_min, int qp_max, int* probes)
{
    if (qp_min > qp_max) throw std::invalid_argument("pick_qp_for_budget: qp_min above qp_max");
    int lo = qp_min - 1, hi = qp_max + 1, count = 0;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;             // (lo + hi) floored, lo may be -1
        const int64_t bits = estimate(mid);
        ++count;
        if (bits < 0) {
            if (probes) *probes = count;
            throw std::runtime_error("pick_qp_for_budget: the size probe failed");
        }
        if (bits <= budget_bits) lo = mid; else hi = mid;
    }
    if (probes) *probes = count;
    return lo < qp_min ? qp_min : lo;
}

int pick_qp_near(const std::function<int64_t(int)>& estimate, int64_t budget_bits, int start, int qp_min, int qp_max, int* probes)
{
    if (qp_min > qp_max) throw std::invalid_argument("pick_qp_near: qp_min above qp_max");
    int count = 0;
    auto fits = [&](int qp) {
        const int64_t bits = estimate(qp);
        ++count;
        if (probes) *probes = count;
        if (bits < 0) throw std::runtime_error("pick_qp_near: the size probe failed");
        return bits <= budget_bits;
    };
    if (probes) *probes = 0;
    const int s = std::min(qp_max, std::max(qp_min, start));
    int lo = qp_min - 1, hi = qp_max + 1, step = 1;
    if (fits(s)) {
        lo = s;
        while (lo < qp_max) {
            const int q = std::min(lo + step, qp_max);
            if (!fits(q)) {
                hi = q;
                break;
            }
            lo = q;
            step *= 2;
        }
    } else {
        hi = s;
        while (hi > qp_min) {
            const int q = std::max(hi - step, qp_min);
            if (fits(q)) {
                lo = q;
                break;
            }
            hi = q;
            step *= 2;
        }
    }
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (fits(mid)) lo = mid; else hi = mid;
    }
    return lo < qp_min ? qp_min : lo;
}

int pick_qp_for_quality(const std::function<double(int)>& measure, double target, int start, int qp_min, int qp_max, int* trials)
{
    if (qp_min > qp_max) throw std::invalid_argument("pick_qp_for_quality: qp_min above qp_max");
    const int flip = qp_min + qp_max;
    const int s = std::min(qp_max, std::max(qp_min, start));
    // reflected index r = flip - q: "meets" falls where "fits" falls, 0 bits against a budget of 0
    const int r = pick_qp_near([&](int rq) -> int64_t {
        const double quality = measure(flip - rq);
        if (std::isnan(quality)) {
            if (trials) *trials += 1;             // pick_qp_near counts a probe when it returns
            throw std::runtime_error("pick_qp_for_quality: the trial failed");
        }
        return quality >= target ? 0 : 1;
    }, 0, flip - s, qp_min, qp_max, trials);
    return flip - r;
}

int64_t unit_budget_bits(double target_bpp, double pixels_per_picture, int pictures_coded, int64_t spent_bits, int horizon, int n)
{
    if (horizon < 1 || n < 0) throw std::invalid_argument("unit_budget_bits: horizon must be positive, n not negative");
    const double share = target_bpp * pixels_per_picture;
    const double budget = share * (pictures_coded + horizon) - static_cast<double>(spent_bits);
    const double want = std::max(budget / horizon, share / 64.0);
    return static_cast<int64_t>(std::floor(want * n));
}

int64_t intra_budget_bits(double target_bpp, double pixels_per_picture, int k, int64_t spent_bits)
{
    const double share = target_bpp * pixels_per_picture;
    const double budget = std::max(share * (k + 1) - static_cast<double>(spent_bits), share / 4.0);
    return static_cast<int64_t>(std::floor(budget));
}

Vbv::Vbv(double maxrate_bpp, double bufsize_pictures, double init, long long pixels)
{
    if (!std::isfinite(maxrate_bpp) || !(maxrate_bpp > 0.0)) throw std::invalid_argument("vbv: maxrate must be a positive number of bits per pixel");
    if (!std::isfinite(bufsize_pictures) || !(bufsize_pictures > 0.0)) {
        throw std::invalid_argument("vbv: bufsize must be a positive number of picture periods");
    }
    if (!std::isfinite(init) || !(init > 0.0) || init > 1.0) throw std::invalid_argument("vbv: init must be in (0, 1] (a fraction of the capacity)");
    if (pixels < 1) throw std::invalid_argument("vbv: pixels must be at least 1");
    m_rate = maxrate_bpp * static_cast<double>(pixels);
    m_capacity = bufsize_pictures * m_rate;
    if (!(m_capacity < 4611686018427387904.0)) throw std::invalid_argument("vbv: the capacity must be below 2^62 bits");
    m_fullness = init * m_capacity;
}

int64_t Vbv::available() const
{
    return static_cast<int64_t>(std::floor(m_fullness));
}

bool Vbv::admit(int64_t bits, int pictures)
{
    if (bits < 0 || pictures < 1) throw std::invalid_argument("vbv: a unit has bits >= 0 and at least 1 picture");
    const int64_t avail = available();
    const double refill = static_cast<double>(pictures) * m_rate;      // a statement of its own: never fused into the sum below
    const double left = m_fullness - static_cast<double>(bits);
    if (bits <= avail) {
        m_underflow = 0;
        m_fullness = std::min(m_capacity, left + refill);
        return false;
    }
    m_underflow = bits - avail;
    m_fullness = std::min(m_capacity, std::max(0.0, left) + refill);
    return true;
}

SceneCut::SceneCut(double threshold, int min_gap, long long pixels) : m_threshold(threshold), m_min_gap(min_gap), m_pixels(pixels)
{
    if (!std::isfinite(threshold) || !(threshold > 0.0) || threshold > 100.0) {
        throw std::invalid_argument("scene cut: the threshold must be in (0, 100] (percent of full range)");
    }
    if (min_gap < 1) throw std::invalid_argument("scene cut: min_gap must be at least 1");
    if (pixels < 1) throw std::invalid_argument("scene cut: pixels must be at least 1");
}

bool SceneCut::push(int idx, long long sad, bool scheduled_intra)
{
    if (idx != m_next) {
        throw std::invalid_argument("scene cut: picture " + std::to_string(idx) + " pushed, " + std::to_string(m_next) + " is next");
    }
    if (idx > 0 && (sad < 0 || sad / 255 > m_pixels || (sad / 255 == m_pixels && sad % 255 != 0))) {      // sad > 255 * pixels
        throw std::invalid_argument("scene cut: sad " + std::to_string(sad) + " is outside [0, 255 * pixels]");
    }
    m_next = idx + 1;
    if (idx == 0) {
        m_mafd = m_score = 0.0;
        m_detected = false;
    } else {
        m_mafd = 100.0 * static_cast<double>(sad) / (256.0 * static_cast<double>(m_pixels));
        m_score = m_has_base ? m_mafd - m_base : 0.0;
        m_detected = m_score >= m_threshold;
        if (!m_detected) {
            m_base = m_mafd;
            m_has_base = true;
        }
    }
    const bool intra = scheduled_intra || (m_detected && (!m_has_intra || idx - m_last_intra >= m_min_gap));
    if (intra) {
        m_last_intra = idx;
        m_has_intra = true;
    }
    return intra;
}

Ivtc::Ivtc(int cycle, int mi) : m_cycle(cycle), m_mi(mi)
{
    if (cycle != 0 && (cycle < 2 || cycle > 32)) throw std::invalid_argument("ivtc: the cycle must be 0 (no decimation) or in 2..32");
    if (mi < 0 || mi > 512) throw std::invalid_argument("ivtc: mi must be in 0..512");
}

int Ivtc::push(int idx, bool has_prev, const uint64_t m[8])
{
    if (m == nullptr) throw std::invalid_argument("ivtc: null words");
    if (idx != m_next) throw std::invalid_argument("ivtc: frame " + std::to_string(idx) + " pushed, " + std::to_string(m_next) + " is next");
    if (idx == 0 && has_prev) throw std::invalid_argument("ivtc: frame 0 has no previous frame");
    if (m[2] > static_cast<uint64_t>(kMaxSamples) || m[3] > static_cast<uint64_t>(kMaxSamples)) {
        throw std::invalid_argument("ivtc: a comb count is above the samples of the largest plane");
    }
    m_next = idx + 1;
    const int match = has_prev && m[1] < m[0] ? 1 : 0;
    const int is_combed = m[4 + match] > static_cast<uint64_t>(m_mi) ? 1 : 0;
    if (m_cycle > 0) {
        const int pos = idx % m_cycle;
        if (pos == 0) m_best_pos = -1;
        if (has_prev && (m_best_pos < 0 || m[6] < m_best)) {
            m_best = m[6];
            m_best_pos = pos;
        }
        m_drop = pos == m_cycle - 1 ? m_best_pos : -1;
    }
    return match | 2 * is_combed;
}

int Ivtc::drop() const { return m_drop; }

CropDetect::CropDetect(int H, int W, int frac, int min_bar, int ax, int ay) : m_H(H), m_W(W), m_frac(frac), m_min_bar(min_bar), m_ax(ax), m_ay(ay)
{
    if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide) throw std::invalid_argument("cropdet: H and W must be in 1..16384");
    if (frac < 0 || frac > 255) throw std::invalid_argument("cropdet: frac must be in 0..255");
    if (min_bar < 0 || min_bar > 4096) throw std::invalid_argument("cropdet: min_bar must be in 0..4096");
    if ((ax != 1 && ax != 2 && ax != 4) || (ay != 1 && ay != 2 && ay != 4)) throw std::invalid_argument("cropdet: ax and ay must be 1, 2 or 4");
    if (H % ay != 0 || W % ax != 0) throw std::invalid_argument("cropdet: H must be a multiple of ay and W of ax");
}

bool CropDetect::push(const uint32_t* counts)
{
    if (counts == nullptr) throw std::invalid_argument("cropdet: null words");
    for (int r = 0; r < m_H; ++r) {
        if (counts[r] > static_cast<uint32_t>(m_W)) throw std::invalid_argument("cropdet: a row count is above the width");
    }
    for (int c = 0; c < m_W; ++c) {
        if (counts[m_H + c] > static_cast<uint32_t>(m_H)) throw std::invalid_argument("cropdet: a column count is above the height");
    }
    // counts <= 2^14 and sides <= 2^14: both products are below 2^22
    const uint32_t row_t = static_cast<uint32_t>(m_W) * static_cast<uint32_t>(m_frac), col_t = static_cast<uint32_t>(m_H) * static_cast<uint32_t>(m_frac);
    int top = -1, bottom = -1, left = -1, right = -1;
    for (int r = 0; r < m_H; ++r) {
        if (counts[r] * 256u > row_t) {
            if (top < 0) top = r;
            bottom = r;
        }
    }
    for (int c = 0; c < m_W; ++c) {
        if (counts[m_H + c] * 256u > col_t) {
            if (left < 0) left = c;
            right = c;
        }
    }
    if (top < 0 || left < 0) return false;
    if (m_votes == 0) {
        m_top = top; m_bottom = bottom; m_left = left; m_right = right;
    } else {
        m_top = std::min(m_top, top); m_bottom = std::max(m_bottom, bottom);
        m_left = std::min(m_left, left); m_right = std::max(m_right, right);
    }
    ++m_votes;
    return true;
}

int CropDetect::result(int& x, int& y, int& w, int& h) const
{
    int T = 0, B = 0, L = 0, R = 0;
    if (m_votes > 0) {
        T = m_top; B = m_H - 1 - m_bottom; L = m_left; R = m_W - 1 - m_right;
    }
    auto bar = [&](int v, int a) { return v < m_min_bar ? 0 : v - v % a; };
    T = bar(T, m_ay); B = bar(B, m_ay); L = bar(L, m_ax); R = bar(R, m_ax);
    x = L; y = T; w = m_W - L - R; h = m_H - T - B;
    return m_votes;
}

}  // namespace dcvc
