/* Rate control of the dcvc tool (no reference counterpart): the one-pass controller towards a target rate and the
 * q_index search on a size probe. Host code only, no GPU. dcvc_amd/rate_control.py is the same arithmetic in Python
 * (TargetBpp, pick_qp_for_budget, pick_qp_for_quality, intra_budget_bits, Vbv); the two are tested against each other.
 *
 * Errors: a negative return code, message through dcvc_last_error() (dcvc_amd_ops.h). */
#ifndef DCVC_AMD_RC_H
#define DCVC_AMD_RC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dcvc_rc dcvc_rc;

/* rate_control.TargetBpp(target_bpp, pixels_per_picture, qp0, horizon, intra_bonus, qp_min, qp_max, slope); NULL on
 * a non-positive target or picture size. */
dcvc_rc* dcvc_rc_create(double target_bpp, double pixels_per_picture, double qp0, int horizon, int intra_bonus,
                        int qp_min, int qp_max, double slope);
void dcvc_rc_destroy(dcvc_rc* rc);
/* q_index of the next coded unit (an I picture gets intra_bonus steps on top) */
int dcvc_rc_next_qp(const dcvc_rc* rc, int is_intra);
/* the unit took `bits` for `pictures` pictures */
int dcvc_rc_update(dcvc_rc* rc, double bits, int pictures, int is_intra);
/* ... of a unit that was coded at qp instead of dcvc_rc_next_qp (a decoder-buffer cap lowered it, below): the slope estimate
 * and the last P unit take qp, and the size the step compares is the unit's projected to the q_index the controller stands
 * at, 2^(log2(bits / pictures) + slope (state_qp - qp)). With qp = dcvc_rc_next_qp(rc, is_intra) it is dcvc_rc_update. */
int dcvc_rc_update_at(dcvc_rc* rc, double bits, int pictures, int is_intra, int qp);
double dcvc_rc_state_qp(const dcvc_rc* rc);      /* the controller's fractional q_index */

/* Largest q_index in [qp_min, qp_max] whose predicted stream fits budget_bits, by bisection on
 * estimate(qp, user) = predicted bits (negative = failure): lo = qp_min - 1 (fits), hi = qp_max + 1 (does not); while
 * hi - lo > 1: mid = floor((lo + hi) / 2) is probed, lo = mid if it fits (estimate <= budget_bits), else hi = mid.
 * Returns lo, or qp_min when nothing fits; at most ceil(log2(qp_max - qp_min + 2)) probes, their number in *probes
 * (may be NULL). Negative on failure. */
typedef int64_t (*dcvc_rc_estimate_fn)(int qp, void* user);
int dcvc_rc_pick_qp_for_budget(dcvc_rc_estimate_fn estimate, void* user, int64_t budget_bits, int qp_min, int qp_max,
                               int* probes);
/* The same answer as dcvc_rc_pick_qp_for_budget on a size curve that rises with the q_index, from a start value (the
 * q_index of the previous P unit): s = start clamped to [qp_min, qp_max] is probed; if it fits, min(lo + step, qp_max) with
 * step = 1, 2, 4, ... is probed from lo = s upward, lo moving to every value that fits, until one does not (hi) or
 * lo = qp_max; if it does not, max(hi - step, qp_min) from hi = s downward until one fits (lo) or hi = qp_min; then the
 * bisection above on (lo, hi). Ends like it: lo fits or is qp_min - 1, lo + 1 was probed and does not fit or is
 * qp_max + 1; returns lo, or qp_min when nothing fits. No q_index is probed twice; 2 probes when the answer is start, at
 * most 4 within 2 of it, at most 2 ceil(log2(qp_max - qp_min + 2)) + 1 (12 over 0 .. 63). */
int dcvc_rc_pick_qp_near(dcvc_rc_estimate_fn estimate, void* user, int64_t budget_bits, int start, int qp_min, int qp_max,
                         int* probes);
/* Coding to a quality, the mirror image of dcvc_rc_pick_qp_near: the smallest q_index whose trial meets the
 * target. measure(qp, user) = the quality of a trial coding at qp (NaN = failure); qp "meets" when measure >= target.
 * s = start clamped to [qp_min, qp_max] is tried first; if it meets, max(s - 1, qp_min), then 2, 4, ... further down from the
 * last value that met, until one does not meet or qp_min met; if it does not, upward in the same way until one meets or
 * qp_max did not; then the bracket is bisected. Returns the smallest bracketed q_index that meets, qp_max when nothing
 * meets: it is dcvc_rc_pick_qp_near under the index reflection q -> qp_min + qp_max - q with "fits" = "meets", so the
 * trial counts are its probe counts: no q_index tried twice, 2 trials when the answer is start, at most 12 over 0 .. 63.
 * The quality of a real model rises with the q_index; the function does not assume it, its result is defined by the
 * procedure. *trials (may be NULL) receives the number of trials. Negative on failure. */
typedef double (*dcvc_rc_quality_fn)(int qp, void* user);
int dcvc_rc_pick_qp_for_quality(dcvc_rc_quality_fn measure, void* user, double target, int start, int qp_min, int qp_max,
                                int* trials);
/* Budget of a P unit of n pictures: share = target_bpp * pixels, want = max((share * (pictures_coded + horizon) -
 * spent_bits) / horizon, share / 64) (what dcvc_rc_update steers towards), floor(want * n), in double arithmetic.
 * Negative on failure (horizon < 1, n < 0). */
int64_t dcvc_rc_unit_budget_bits(double target_bpp, double pixels_per_picture, int pictures_coded, int64_t spent_bits,
                                 int horizon, int n);
/* Budget of picture k (0-based) of an all-intra run: floor(max(target_bpp * pixels * (k + 1) - spent_bits,
 * target_bpp * pixels / 4)) in double arithmetic. */
int64_t dcvc_rc_intra_budget_bits(double target_bpp, double pixels_per_picture, int k, int64_t spent_bits);

/* Decoder-buffer (VBV) model of dcvc encode --vbv-maxrate / --vbv-bufsize (rate_control.Vbv is the same
 * arithmetic in Python, compared with == on the fullness). All in IEEE double, in the operation order written here:
 *   r = maxrate_bpp * pixels         bits that arrive per picture period (pixels = W * H of the coded size)
 *   C = bufsize_pictures * r         the capacity
 *   F = init * C                     the start fullness
 * A unit of `bits` bits - 8 times every byte it adds to the output: container header, payload, and a parameter set written
 * in front of it - that holds n source pictures (an I picture or an LD P unit 1, an HT chunk 8, a ragged last chunk what
 * the source really held) must be whole in the buffer when its first picture is due: it conforms iff bits <= avail =
 * floor(F) as int64. Behind a unit that conforms F = min(C, (F - bits) + n * r). Behind one that does not, underflow = bits -
 * avail is recorded and F = min(C, max(0.0, F - bits) + n * r). Nothing is padded when the buffer would overflow: a cap (VBR
 * under a ceiling), not filler CBR.
 * dcvc_rc_vbv_create returns NULL, with a message, for a value that is not finite or not positive, init outside (0, 1],
 * pixels < 1, or a capacity of 2^62 bits or more. */
typedef struct dcvc_rc_vbv dcvc_rc_vbv;
dcvc_rc_vbv* dcvc_rc_vbv_create(double maxrate_bpp, double bufsize_pictures, double init, long long pixels);
void dcvc_rc_vbv_destroy(dcvc_rc_vbv* v);
/* avail = floor(F): the bits the next unit may take; negative on a null handle */
int64_t dcvc_rc_vbv_available(const dcvc_rc_vbv* v);
/* the unit took `bits` for `pictures` source pictures: 0 = it conforms, 1 = a violation (F and the underflow as above);
 * negative, the model unchanged, for bits < 0 or pictures < 1 */
int dcvc_rc_vbv_admit(dcvc_rc_vbv* v, int64_t bits, int pictures);
double dcvc_rc_vbv_fullness(const dcvc_rc_vbv* v);      /* F */
double dcvc_rc_vbv_capacity(const dcvc_rc_vbv* v);      /* C */
double dcvc_rc_vbv_rate(const dcvc_rc_vbv* v);          /* r */
/* bits - avail of the last admitted unit when it was a violation, else 0 */
int64_t dcvc_rc_vbv_underflow(const dcvc_rc_vbv* v);


/* Scene-cut decisions of dcvc encode --scene-cut (dcvc_amd/scene.py SceneCut is the same arithmetic in
 * Python). Pictures are pushed in source order, idx = 0, 1, ..., with sad = dcvc_luma_sad of picture idx against idx - 1
 * (ignored for idx 0, where mafd = score = 0).
 *   mafd = 100.0 * sad / (256.0 * pixels), in this operation order, in double: the mean absolute luma difference in
 *   percent of full range. score = mafd - base, base = the mafd of the most recent pushed pair that was not detected; with
 *   no base yet (idx <= 1) the score is 0 and the pair sets the base. detected = score >= threshold. A detected pair does not
 *   update the base: the picture after a cut is measured against the motion level before it, not against the spike.
 * dcvc_scd_push returns 1 = code picture idx as an I picture: scheduled_intra is set, or the pair is detected and
 * idx - last_intra >= min_gap, last_intra = the last picture 1 was returned for (none yet: the distance counts as
 * enough); 0 = as scheduled; negative = refused, the detector unchanged: sad < 0 or sad > 255 * pixels, or an idx that is
 * not the previous one plus 1. dcvc_scd_create returns NULL for a threshold that is not finite or outside (0, 100],
 * min_gap < 1 or pixels < 1. dcvc_scd_last: the last pushed picture's figures (NULL pointers are skipped). */
typedef struct dcvc_scd dcvc_scd;
dcvc_scd* dcvc_scd_create(double threshold, int min_gap, long long pixels);
int dcvc_scd_push(dcvc_scd* scd, int idx, long long sad, int scheduled_intra);
int dcvc_scd_last(const dcvc_scd* scd, double* mafd, double* score, int* detected);
void dcvc_scd_destroy(dcvc_scd* scd);

/* Inverse-telecine decisions of dcvc encode --ivtc (dcvc_amd/ivtc.py Ivtc is the same arithmetic in Python).
 * Source frames are pushed in order, idx = 0, 1, ..., with the eight words m = [match_c, match_p, comb_c, comb_p, blkmax_c,
 * blkmax_p, dup, 0] of dcvc_field_match of frame idx against idx - 1 (has_prev = 0: the frame was measured alone).
 *   match: p (1) when has_prev and match_p < match_c, strictly; else c (0). combed: the chosen match's blkmax > mi.
 *   dcvc_ivtc_push returns match | 2 * combed; negative = refused, the state unchanged: an idx that is not the previous one
 *   plus 1, has_prev at idx 0, a comb count above 16384 * 16384 (the samples of the largest plane dcvc_field_match takes), a
 *   NULL handle or NULL words.
 *   The cycle grid is fixed from frame 0: frames cycle * k .. cycle * k + cycle - 1 are one cycle. dcvc_ivtc_drop is valid
 *   once all `cycle` frames of a cycle are pushed, until the next push: the position 0 .. cycle - 1 of the frame with the
 *   smallest dup, ties to the lowest position; a frame pushed without prev (frame 0 of the clip) has no dup and is never
 *   dropped. -1 while the cycle is incomplete, when cycle == 0, or on a NULL handle. A ragged last cycle drops nothing.
 * dcvc_ivtc_create returns NULL for a cycle that is neither 0 (no decimation) nor in 2..32, or mi outside 0..512. */
typedef struct dcvc_ivtc dcvc_ivtc;
dcvc_ivtc* dcvc_ivtc_create(int cycle, int mi);
int dcvc_ivtc_push(dcvc_ivtc* t, int idx, int has_prev, const uint64_t m[8]);
int dcvc_ivtc_drop(const dcvc_ivtc* t);
void dcvc_ivtc_destroy(dcvc_ivtc* t);

/* Black-bar decision of dcvc encode --crop auto (dcvc_amd/crop.py CropDetect is the same arithmetic in Python).
 * counts = the H + W words of dcvc_crop_stats of a probed picture: rowcnt, then colcnt. Exact integers:
 *   row r is active iff rowcnt[r] * 256 > W * frac, column c iff colcnt[c] * 256 > H * frac. A picture with no active row or
 *   no active column casts no vote (a fade, a black leader); a voting picture's rectangle runs from its first to its last
 *   active row and column; the result is the union over the voting pictures. The bars T = top, B = H - 1 - bottom, L = left,
 *   R = W - 1 - right: one below min_bar becomes 0, then each is rounded DOWN to a multiple of ay (T, B) or ax (L, R), so
 *   picture content is never cut. The window is x = L, y = T, w = W - L - R, h = H - T - B; with no vote the whole picture.
 *   dcvc_cropdet_push returns 1 (voted) or 0 (no vote); negative = refused, the state unchanged: NULL, a row count above W or
 *   a column count above H. dcvc_cropdet_result returns the number of votes (negative: a NULL argument).
 * dcvc_cropdet_create returns NULL for H or W outside 1..16384, frac outside 0..255, min_bar outside 0..4096, ax or ay other
 * than 1, 2 or 4, or H / W that are not multiples of ay / ax. */
typedef struct dcvc_cropdet dcvc_cropdet;
dcvc_cropdet* dcvc_cropdet_create(int H, int W, int frac, int min_bar, int ax, int ay);
int dcvc_cropdet_push(dcvc_cropdet* t, const uint32_t* counts);
int dcvc_cropdet_result(const dcvc_cropdet* t, int* x, int* y, int* w, int* h);
void dcvc_cropdet_destroy(dcvc_cropdet* t);

/* Film grain, the host side (dcvc_amd/grain.py grain_template and grain_fit are the same arithmetic in Python).
 *   dcvc_grain_template: out (host, int16 [64][64]) = the grain template of (seed, plane 0..2, size 0..37) that
 *   dcvc_grain_apply (dcvc_amd_ops.h) tiles over a plane. s = seed*0x9E3779B1 + plane*0xC2B2AE3D + 1 (u32, wrapping); per
 *   position in row-major order four draws s = s*1664525 + 1013904223, byte = s >> 24, w = the four bytes' sum - 510; with
 *   a = size, b = 128 - 2a: h = a w[x-1] + b w[x] + a w[x+1], then the same pass down the columns of h gives f, both on the
 *   64 x 64 torus; rms = isqrt(sum f^2 / 4096), T = floor((128 f + rms) / (2 rms)): a standard deviation of about 64, a lag-1
 *   correlation of about 2ab / (2a^2 + b^2). Refused: NULL out, plane outside 0..2, size outside 0..37, rms == 0, |T| > 1023.
 *   dcvc_grain_fit: words (host, [3][16]: the words of dcvc_grain_stats of Y, U, V, summed over a window of pictures) ->
 *   lut_out (host, uint8 [3][9]). Per plane and bin with n >= min_count the value is min(255, isqrt((256 S gain_percent^2) /
 *   (n 10000 << 2 (bit_depth - 8)))), floor division in 128 bits: the residual's standard deviation in sixteenths of an 8-bit
 *   code value. A bin below min_count takes the nearest valid bin's value, ties to the lower bin; a plane without a valid bin
 *   gets zeros. lut[0] = bin 0, lut[8] = bin 7, lut[k] = (bin[k-1] + bin[k] + 1) >> 1. Refused: a NULL pointer, bit_depth
 *   outside 8..16, gain_percent outside 1..400, min_count below 1, a word of 2^63 or above. */
int dcvc_grain_template(uint32_t seed, int plane, int size, int16_t* out);
int dcvc_grain_fit(const uint64_t* words, int bit_depth, int gain_percent, long long min_count, uint8_t* lut_out);

#ifdef __cplusplus
}
#endif
#endif /* DCVC_AMD_RC_H */
