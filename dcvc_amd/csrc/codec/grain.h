// Host side of film grain (no reference counterpart): the 64 x 64 grain template that dcvc_grain_apply tiles over
// a plane, and the fit of per-luma-bin tables to the words of dcvc_grain_stats. Exact integers; dcvc_amd/grain.py restates both
// (grain_template, grain_fit) and tests/grain_np.py restates them once more in numpy.
#pragma once

#include <cstdint>

namespace dcvc {

constexpr int kGrainMaxSize = 37;                    // the correlation model 2ab / (2a^2 + b^2) is monotone up to a = 37
constexpr int kGrainTemplateSide = 64;

// out [64][64]: white noise from an LCG seeded by (seed, plane) - four bytes a position, w = their sum - 510 - through the
// separable kernel [a, b, a], a = size, b = 128 - 2a, on the torus, normalised to a standard deviation of about 64:
// T = floor((128 f + rms) / (2 rms)), rms = isqrt(sum f^2 / 4096). Throws std::invalid_argument for out == nullptr, plane
// outside 0..2, size outside 0..37; std::runtime_error for rms == 0 or |T| > 1023 (neither happens for these sizes).
void grain_template(uint32_t seed, int plane, int size, int16_t* out);

// words [3][16] (dcvc_grain_stats of Y, U, V, summed over a window) -> lut_out [3][9]. Per plane and bin with n >= min_count:
// min(255, isqrt((256 S gain^2) / (n 10000 << 2 sh))); a bin below min_count takes the nearest valid bin's value, ties to the
// lower bin; no valid bin: the plane's table is 0. Nodes: lut[0] = bin 0, lut[8] = bin 7, lut[k] = (bin[k-1] + bin[k] + 1) >> 1.
// Throws std::invalid_argument for a null pointer, bit_depth outside 8..16, gain_percent outside 1..400, min_count below 1, or
// a word of 2^63 or above.
void grain_fit(const uint64_t* words, int bit_depth, int gain_percent, long long min_count, uint8_t* lut_out);

}  // namespace dcvc
