// Code length of the symbols the rANS coder codes (rans_coder.cpp enc_symbol), as plain tables: what a stream will
// take is decided once the symbols and their CDF indexes exist, long before the coder has run. Host side only; the
// tables are summed on the device by kernels/code_length.hip.
//
// Unit: 2^-16 bit (kCodeLengthUnit per bit). A symbol coded with frequency f out of 2^16 costs
//   rint(65536 * (16 - log2(f)))                                     (double arithmetic)
// and an escaped one (value >= max_value = cdf_len - 2) the cost of max_value's own frequency plus 2 bits for each
// bypass group enc_symbol emits: n_groups raw groups, one count group and n_groups / 3 continuation groups.
#pragma once

#include <cstddef>
#include <cstdint>

namespace dcvc {

constexpr int kCodeLengthUnitBits = 16;
constexpr int kCodeLengthYCols = 256;     // y family: column = uint8(symbol), symbol = int8
constexpr int kCodeLengthZCols = 128;     // z family: column = z + 64, z in [-64, 63]
constexpr uint32_t kCodeLengthUncodable = 0xFFFFFFFFu;   // a value whose frequency is 0

// cost of one value of frequency freq (1 .. 65536) followed by `bypass_groups` 2-bit groups
uint32_t code_length_cost(int freq, int bypass_groups);

// Cost table of one CDF family (the arguments of RansEncoder::set_cdf): out[num_cdf][cols], cols = 256 with
// column uint8(symbol) (y) or 128 with column symbol + 64 (z).
void code_length_table(const int32_t* cdfs, int num_cdf, int stride, const int32_t* cdf_sizes, int cols, uint32_t* out);

// Ideal code length -> bytes of the stream RansEncoder::flush builds from it with `ec_parallel` sub-streams: every
// sub-stream ends with its 32-bit state (encode_substream), and a container of n >= 3 sub-streams starts with
// n / 2 - 1 + n % 2 32-bit offsets (flush). The byte-sharing of a sub-stream pair only shortens the stream.
int64_t code_length_fixed_bits(int ec_parallel);
int64_t predicted_stream_bytes(int64_t y_units, int64_t z_units, int ec_parallel);

}  // namespace dcvc
