// Host side of film grain (grain.h).
#include "codec/grain.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace dcvc {

namespace {

uint64_t isqrt64(uint64_t v)
{
    uint64_t r = 0;
    for (uint64_t bit = 1ull << 31; bit; bit >>= 1) {
        const uint64_t c = r | bit;
        if (c * c <= v) r = c;
    }
    return r;
}

int64_t floor_div(int64_t a, int64_t b)     // b > 0
{
    int64_t q = a / b;
    if (a % b < 0) --q;
    return q;
}

}  // namespace

void grain_template(uint32_t seed, int plane, int size, int16_t* out)
{
    if (out == nullptr) throw std::invalid_argument("grain_template: null out");
    if (plane < 0 || plane > 2) throw std::invalid_argument("grain_template: plane must be in 0..2, got " + std::to_string(plane));
    if (size < 0 || size > kGrainMaxSize) throw std::invalid_argument("grain_template: size must be in 0..37, got " + std::to_string(size));
    constexpr int N = kGrainTemplateSide;
    uint32_t s = seed * 0x9E3779B1u + static_cast<uint32_t>(plane) * 0xC2B2AE3Du + 1u;
    std::vector<int64_t> w(N * N), h(N * N), f(N * N);
    for (int i = 0; i < N * N; ++i) {
        int sum = 0;
        for (int k = 0; k < 4; ++k) {
            s = s * 1664525u + 1013904223u;
            sum += static_cast<int>(s >> 24);
        }
        w[i] = sum - 510;
    }
    const int64_t a = size, b = 128 - 2 * size;
    for (int y = 0; y < N; ++y) {
        for (int x = 0; x < N; ++x) h[y * N + x] = a * w[y * N + ((x + N - 1) & (N - 1))] + b * w[y * N + x] + a * w[y * N + ((x + 1) & (N - 1))];
    }
    int64_t Q = 0;                           // |f| <= 128 * 128 * 510 < 2^23.1: 4096 squares sum below 2^59
    for (int y = 0; y < N; ++y) {
        for (int x = 0; x < N; ++x) {
            const int64_t v = a * h[((y + N - 1) & (N - 1)) * N + x] + b * h[y * N + x] + a * h[((y + 1) & (N - 1)) * N + x];
            f[y * N + x] = v;
            Q += v * v;
        }
    }
    const int64_t rms = static_cast<int64_t>(isqrt64(static_cast<uint64_t>(Q / (N * N))));
    if (rms == 0) throw std::runtime_error("grain_template: the filtered noise is zero");
    for (int i = 0; i < N * N; ++i) {
        const int64_t t = floor_div(128 * f[i] + rms, 2 * rms);
        if (t < -1023 || t > 1023) throw std::runtime_error("grain_template: a template value is outside -1023..1023");
        out[i] = static_cast<int16_t>(t);
    }
}

void grain_fit(const uint64_t* words, int bit_depth, int gain_percent, long long min_count, uint8_t* lut_out)
{
    if (words == nullptr || lut_out == nullptr) throw std::invalid_argument("grain_fit: null operand");
    if (bit_depth < 8 || bit_depth > 16) throw std::invalid_argument("grain_fit: bit_depth must be in 8..16, got " + std::to_string(bit_depth));
    if (gain_percent < 1 || gain_percent > 400) {
        throw std::invalid_argument("grain_fit: gain_percent must be in 1..400, got " + std::to_string(gain_percent));
    }
    if (min_count < 1) throw std::invalid_argument("grain_fit: min_count must be at least 1, got " + std::to_string(min_count));
    for (int i = 0; i < 48; ++i) {
        if (words[i] >> 63) throw std::invalid_argument("grain_fit: a word is 2^63 or above");
    }
    const int sh = bit_depth - 8;
    for (int p = 0; p < 3; ++p) {
        const uint64_t* n = words + 16 * p;
        const uint64_t* S = n + 8;
        int bin[8];
        bool valid[8], any = false;
        for (int k = 0; k < 8; ++k) {
            valid[k] = n[k] >= static_cast<uint64_t>(min_count);
            bin[k] = 0;
            if (!valid[k]) continue;
            any = true;
            // S < 2^63, 256 gain^2 < 2^26, n 10000 << 16 < 2^93
            const unsigned __int128 num = static_cast<unsigned __int128>(S[k]) * 256u * static_cast<unsigned>(gain_percent * gain_percent);
            const unsigned __int128 den = (static_cast<unsigned __int128>(n[k]) * 10000u) << (2 * sh);
            const unsigned __int128 q = num / den;
            bin[k] = q >= 256u * 256u ? 255 : static_cast<int>(isqrt64(static_cast<uint64_t>(q)));
        }
        uint8_t* lut = lut_out + 9 * p;
        if (!any) {
            for (int k = 0; k < 9; ++k) lut[k] = 0;
            continue;
        }
        int full[8] = {};
        for (int k = 0; k < 8; ++k) {
            for (int dist = 0; dist < 8; ++dist) {       // the nearest valid bin, the lower one first
                if (k - dist >= 0 && valid[k - dist]) { full[k] = bin[k - dist]; break; }
                if (k + dist < 8 && valid[k + dist]) { full[k] = bin[k + dist]; break; }
            }
        }
        lut[0] = static_cast<uint8_t>(full[0]);
        lut[8] = static_cast<uint8_t>(full[7]);
        for (int k = 1; k < 8; ++k) lut[k] = static_cast<uint8_t>((full[k - 1] + full[k] + 1) >> 1);
    }
}

}  // namespace dcvc
