// picture_io.h - what the host sides of the picture kernels (picture_yuv.hip, rgb_cs.hip, sse.hip) share: one thread per 8
// samples of a row in 256-thread workgroups, 32-bit thread indices, vector accesses behind aligned bases.
#pragma once

#include "ops.h"

namespace dcvc {

constexpr int kPictureThreads = 256;

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// workgroups of `rows` rows of W samples, one thread per 8 samples of a row
inline unsigned grid_of(int rows, int W)
{
    const long long n = static_cast<long long>(rows) * ((W + 7) / 8);
    return static_cast<unsigned>((n + kPictureThreads - 1) / kPictureThreads);
}

// throws std::invalid_argument: sides not positive and even, or too large
inline void picture_validate(int H, int W, const char* what)
{
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) {
        throw std::invalid_argument(std::string(what) + ": the picture sides must be positive and even, got " +
                                    std::to_string(W) + "x" + std::to_string(H));
    }
    // one thread per 8 pixels of a row, 32-bit thread indices (addresses are 64-bit)
    if (static_cast<long long>(H) * ((W + 7) / 8) + kPictureThreads > (1LL << 31)) throw std::invalid_argument(std::string(what) + ": picture too large");
}

}  // namespace dcvc
