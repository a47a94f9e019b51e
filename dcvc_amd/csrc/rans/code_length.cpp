// See code_length.h. The symbol -> value mapping, the escape and the bypass group count restate enc_symbol
// (rans_coder.cpp); tests/test_code_length_cpu.py holds the tables against the coder's real output.
#include "rans/code_length.h"

#include "rans/rans_coder.h"

#include <cmath>
#include <stdexcept>

namespace dcvc {

uint32_t code_length_cost(int freq, int bypass_groups)
{
    if (freq < 1 || freq > (1 << kRansProbBits) || bypass_groups < 0) return kCodeLengthUncodable;
    const double unit = static_cast<double>(1 << kCodeLengthUnitBits);
    const double bits = static_cast<double>(kRansProbBits) - std::log2(static_cast<double>(freq));
    return static_cast<uint32_t>(std::rint(unit * bits)) +
           static_cast<uint32_t>(bypass_groups * kBypassBits) * (1u << kCodeLengthUnitBits);
}

void code_length_table(const int32_t* cdfs, int num_cdf, int stride, const int32_t* cdf_sizes, int cols, uint32_t* out)
{
    if (cdfs == nullptr || cdf_sizes == nullptr || out == nullptr) throw std::invalid_argument("code_length_table: null pointer");
    if (cols != kCodeLengthYCols && cols != kCodeLengthZCols) throw std::invalid_argument("code_length_table: 256 (y) or 128 (z) columns");
    if (num_cdf < 1 || stride < 2) throw std::invalid_argument("code_length_table: empty CDF family");
    for (int i = 0; i < num_cdf; ++i) {
        const int32_t* row = cdfs + static_cast<size_t>(i) * stride;
        const int max_value = static_cast<int8_t>(cdf_sizes[i] - 2);       // as CdfTable::load keeps it
        if (cdf_sizes[i] < 2 || cdf_sizes[i] > stride || max_value < 0) {      // a row the coder cannot use
            for (int col = 0; col < cols; ++col) out[static_cast<size_t>(i) * cols + col] = kCodeLengthUncodable;
            continue;
        }
        for (int col = 0; col < cols; ++col) {
            const int sym = cols == kCodeLengthYCols ? static_cast<int8_t>(static_cast<uint8_t>(col)) : col - 64;
            int value = (sym < 0 ? -sym : sym) * 2 - (sym > 0);
            int groups = 0;
            if (value >= max_value) {
                const uint32_t raw = static_cast<uint32_t>(value - max_value);
                value = max_value;
                int n_groups = 0;
                while ((raw >> (n_groups * kBypassBits)) != 0) ++n_groups;
                groups = n_groups + 1 + n_groups / ((1 << kBypassBits) - 1);
            }
            const int freq = static_cast<uint16_t>(row[value + 1] - row[value]);
            out[static_cast<size_t>(i) * cols + col] = code_length_cost(freq, groups);
        }
    }
}

int64_t code_length_fixed_bits(int ec_parallel)
{
    if (ec_parallel < 1 || ec_parallel > kMaxEcParallel) throw std::invalid_argument("ec_parallel must be in [1, 8]");
    const int n = ec_parallel;
    const int n_offsets = n == 1 ? 0 : n / 2 - 1 + n % 2;
    return 32LL * n + 32LL * n_offsets;
}

int64_t predicted_stream_bytes(int64_t y_units, int64_t z_units, int ec_parallel)
{
    if (y_units < 0 || z_units < 0) throw std::invalid_argument("predicted_stream_bytes: negative code length");
    const int64_t unit = 1LL << kCodeLengthUnitBits;
    const int64_t units = y_units + z_units + code_length_fixed_bits(ec_parallel) * unit;
    return (units + 8 * unit - 1) / (8 * unit);
}

}  // namespace dcvc
