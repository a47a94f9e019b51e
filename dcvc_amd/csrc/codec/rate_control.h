// Rate control of the native tool: the one-pass feedback controller of dcvc_amd/rate_control.py (TargetBpp) and the
// search for the largest q_index whose predicted stream fits a budget, on top of a size probe. Plain host code; the
// Python module is the restatement the tests compare with, so the arithmetic here follows it operation for operation
// (double, rint where Python's round() rounds half to even).
#pragma once

#include <cstdint>
#include <functional>

namespace dcvc {

class TargetBpp {
public:
    TargetBpp(double target_bpp, double pixels_per_picture, double qp0 = 32, int horizon = 8, int intra_bonus = 0,
              int qp_min = 0, int qp_max = 63, double slope = 0.049);
    int next_qp(bool is_intra) const;
    void update(double bits, int pictures, bool is_intra);
    // ... of a unit that was coded at `qp`, not at next_qp(is_intra) (a decoder-buffer cap lowered it): the slope
    // estimate and the last P unit take `qp`, and the size the step compares is projected from `qp` to the q_index the
    // controller stands at, 2^(log2(per_picture) + slope (m_qp - qp)), as the update behind an I picture projects the last P unit
    void update_at(double bits, int pictures, bool is_intra, int qp);
    double qp() const { return m_qp; }
    double spent() const { return m_spent; }
    int pictures() const { return m_pictures; }

private:
    void update(double bits, int pictures, bool is_intra, int used_qp);
    double m_target_bits, m_qp, m_slope, m_max_step = 4.0, m_spent = 0.0;
    int m_horizon, m_intra_bonus, m_qp_min, m_qp_max, m_pictures = 0;
    bool m_has_last = false;
    int m_last_qp = 0;
    double m_last_log = 0.0;
};

// Bisection over the q_index. estimate(qp) = predicted bits of the stream at qp (negative = failure, passed on).
// lo = qp_min - 1 counts as fitting, hi = qp_max + 1 as not; while hi - lo > 1: mid = (lo + hi) / 2 (floor), probed,
// lo = mid if estimate(mid) <= budget_bits, else hi = mid. Returns lo, or qp_min when lo never moved; at most
// ceil(log2(qp_max - qp_min + 2)) probes. probes (may be null) receives their number.
int pick_qp_for_budget(const std::function<int64_t(int)>& estimate, int64_t budget_bits, int qp_min, int qp_max, int* probes);

// The same answer from a start value, for P units whose neighbours have neighbouring size curves. s = start clamped to the
// range is probed. It fits: gallop upward - min(lo + step, qp_max) with step = 1, 2, 4, ... from lo = s, lo moving to every
// value that fits - to the first value that does not fit (hi) or until lo = qp_max. It does not: gallop downward from hi = s -
// max(hi - step, qp_min), hi moving to every value that does not fit - to the first value that fits (lo) or until hi = qp_min.
// Then the bisection of pick_qp_for_budget on (lo, hi). No q_index is probed twice; 2 probes when the answer is start, at
// most 2 ceil(log2(qp_max - qp_min + 2)) + 1 in any range (12 over 0 .. 63).
int pick_qp_near(const std::function<int64_t(int)>& estimate, int64_t budget_bits, int start, int qp_min, int qp_max, int* probes);

// The mirror image, for coding to a quality: the smallest bracketed q_index whose trial meets, measure(qp) >=
// target (NaN = failure, thrown). pick_qp_near under the index reflection q -> qp_min + qp_max - q, "fits" = "meets": s is
// tried; it meets: gallop downward with step 1, 2, 4, ... to the first value that does not meet or to qp_min; it does not:
// gallop upward to the first value that meets or to qp_max; then the bisection. qp_max when nothing meets. The same trial
// counts: none twice, 2 when the answer is start, at most 12 over 0 .. 63. trials (may be null) receives their number.
int pick_qp_for_quality(const std::function<double(int)>& measure, double target, int start, int qp_min, int qp_max, int* trials);

// Budget of a P unit of n pictures in a run towards target_bpp, from what TargetBpp::update aims at: with share =
// target_bpp * pixels_per_picture, want = max((share * (pictures_coded + horizon) - spent_bits) / horizon, share / 64) bits
// per picture; floor(want * n) in double arithmetic.
int64_t unit_budget_bits(double target_bpp, double pixels_per_picture, int pictures_coded, int64_t spent_bits, int horizon, int n);

// Budget of picture k (0-based) of an all-intra run towards target_bpp: what the k + 1 pictures may take together minus what
// the first k took, floored at a quarter of one picture's share. floor() of the double value.
int64_t intra_budget_bits(double target_bpp, double pixels_per_picture, int k, int64_t spent_bits);

// Decoder-buffer model of dcvc encode --vbv-maxrate / --vbv-bufsize (rate_control.Vbv is the restatement): a
// bucket of capacity C = bufsize_pictures * r bits that fills with r = maxrate_bpp * pixels bits per picture period and starts
// at F = init * C. A unit of `bits` bits that holds n source pictures must be whole in the bucket when its first picture is
// due: it conforms iff bits <= avail = floor(F). Behind it F = min(C, (F - bits) + n * r); behind a unit that does not conform
// F = min(C, max(0.0, F - bits) + n * r), and underflow = bits - avail. Nothing is padded at the top: a cap, not filler CBR.
// All in double, in this operation order.
class Vbv {
public:
    // every value finite and positive, init in (0, 1], pixels >= 1, and a capacity below 2^62 bits
    Vbv(double maxrate_bpp, double bufsize_pictures, double init, long long pixels);
    int64_t available() const;
    bool admit(int64_t bits, int pictures);      // true: a violation. bits >= 0, pictures >= 1 (std::invalid_argument)
    double fullness() const { return m_fullness; }
    double capacity() const { return m_capacity; }
    double rate() const { return m_rate; }
    int64_t underflow() const { return m_underflow; }

private:
    double m_rate = 0.0, m_capacity = 0.0, m_fullness = 0.0;
    int64_t m_underflow = 0;
};

// Scene-cut decisions of dcvc encode --scene-cut (dcvc_amd/scene.py SceneCut is the restatement). Pictures
// are pushed in source order with the luma SAD against their predecessor (dcvc_luma_sad). mafd = 100.0 * sad /
// (256.0 * pixels) in double, in this operation order; score = mafd - base, base = the mafd of the most recent pair that
// was not detected (no base yet: score 0, and the pair becomes the base); detected = score >= threshold. A detected pair
// leaves the base alone, so the picture after a cut is measured against the motion before it, not against the spike.
class SceneCut {
public:
    SceneCut(double threshold, int min_gap, long long pixels);      // threshold in (0, 100], min_gap >= 1, pixels >= 1
    // true: code picture idx as an I picture - it is scheduled as one, or it is detected and at least min_gap pictures
    // after the last picture this returned true for (none yet: far enough). idx must follow the previous one (0 first);
    // sad in [0, 255 * pixels], ignored for idx 0. A refused push (std::invalid_argument) changes nothing.
    bool push(int idx, long long sad, bool scheduled_intra);
    double mafd() const { return m_mafd; }
    double score() const { return m_score; }
    bool detected() const { return m_detected; }

private:
    double m_threshold, m_base = 0.0, m_mafd = 0.0, m_score = 0.0;
    int m_min_gap, m_next = 0, m_last_intra = 0;
    long long m_pixels;
    bool m_has_base = false, m_has_intra = false, m_detected = false;
};

// Inverse-telecine decisions of dcvc encode --ivtc (dcvc_amd/ivtc.py Ivtc is the restatement). Source frames
// are pushed in order with the eight words of dcvc_field_match against their predecessor: m = [match_c, match_p, comb_c,
// comb_p, blkmax_c, blkmax_p, dup, 0]. The match is p when has_prev and match_p < match_c (strictly), else c; the frame is
// combed when the chosen match's blkmax > mi. The cycle grid is fixed from frame 0: frames cycle k .. cycle k + cycle - 1 are
// one cycle, and once all of them are pushed drop() names the one with the smallest dup (ties: the lowest position; a frame
// without prev has no dup and is never dropped).
class Ivtc {
public:
    static constexpr long long kMaxSamples = 16384LL * 16384;      // the largest plane dcvc_field_match takes
    Ivtc(int cycle, int mi);                         // cycle 0 (no decimation) or 2..32, mi 0..512
    // match | 2 * combed. idx must follow the previous one (0 first), has_prev is false at idx 0, comb_c and comb_p at most
    // kMaxSamples. A refused push (std::invalid_argument) changes nothing.
    int push(int idx, bool has_prev, const uint64_t m[8]);
    int drop() const;                                // the position in the cycle just completed; -1: incomplete, or cycle 0

private:
    int m_cycle, m_mi, m_next = 0, m_drop = -1;
    uint64_t m_best = 0;
    int m_best_pos = -1;
};

// Black-bar decision of dcvc encode --crop auto (dcvc_amd/crop.py CropDetect is the restatement). Pictures are
// pushed, in any order, with the H + W words of dcvc_crop_stats: rowcnt, then colcnt. Row r is active iff rowcnt[r] * 256 >
// W * frac, column c iff colcnt[c] * 256 > H * frac; a picture without an active row or column casts no vote, a voting one's
// rectangle runs from its first to its last active row and column, and the result is the union of the rectangles. The bars
// T, B, L, R around it: one below min_bar becomes 0, then each is rounded down to a multiple of ay (T, B) or ax (L, R), so
// picture content is never cut. Without a vote the window is the whole picture.
class CropDetect {
public:
    static constexpr int kMaxSide = 16384;           // the largest plane dcvc_crop_stats takes
    // H, W 1..16384 and multiples of ay, ax; frac 0..255; min_bar 0..4096; ax, ay each 1, 2 or 4
    CropDetect(int H, int W, int frac, int min_bar, int ax, int ay);
    // true: the picture voted. A row count above W or a column count above H is refused (std::invalid_argument), the state unchanged.
    bool push(const uint32_t* counts);
    int result(int& x, int& y, int& w, int& h) const;      // the number of votes
    int words() const { return m_H + m_W; }

private:
    int m_H, m_W, m_frac, m_min_bar, m_ax, m_ay, m_votes = 0;
    int m_top = 0, m_bottom = 0, m_left = 0, m_right = 0;  // the union, valid with m_votes > 0
};

}  // namespace dcvc
