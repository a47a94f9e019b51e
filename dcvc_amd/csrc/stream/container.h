// Bit-stream container of a coded sequence (host code). Format and reference: include/dcvc_amd_stream.h
// (stream_helper.py:37-154). C++ face of the C ABI, used by the standalone encoder / decoder.
#pragma once

#include "dcvc_amd_stream.h"

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace dcvc {
namespace stream {

enum NalType : int { kSps = 0, kIntra = 1, kInter = 2 };

struct StreamError : std::runtime_error {
    int code;        // -1 range / space, -2 truncated, -3 malformed
    StreamError(int c, const char* what) : std::runtime_error(what), code(c) {}
};

// appends to `out`
void put_uint(std::vector<uint8_t>& out, uint32_t value);
void put_sps(std::vector<uint8_t>& out, int sps_id, int height, int width);
void put_ip(std::vector<uint8_t>& out, bool is_i, int sps_id, int qp, int ec_part, bool reset,
            const uint8_t* payload, size_t payload_bytes);

// bytes put_ip adds around a payload of that length - 3 header bytes and the varuint length - plus, with_sps, the bytes of the
// put_sps in front of it: what a unit adds to the stream is payload_bytes + unit_overhead(...). Refuses what the two refuse.
// Never smaller for a longer payload: a varuint grows with its value.
size_t unit_overhead(size_t payload_bytes, bool with_sps, int height, int width);

// sequential reader over caller memory
class Reader {
public:
    Reader(const uint8_t* p, size_t n) : m_p(p), m_n(n) {}
    bool at_end() const { return m_pos >= m_n; }
    size_t position() const { return m_pos; }
    void header(int& nal_type, int& sps_id);
    void sps_remaining(int& height, int& width);
    void ip_remaining(int& qp, int& ec_part, bool& reset, const uint8_t*& payload, size_t& payload_bytes);
    uint32_t get_uint();

private:
    const uint8_t* take(size_t k);
    const uint8_t* m_p;
    size_t m_n;
    size_t m_pos = 0;
};

// feed-style parser over a buffer that may end inside a unit (dcvc_stream_next_unit, include/dcvc_amd_stream.h): the bytes of
// the unit at src, or 0 with u.need set (at_eof: 0 with u.need 0 at n == 0, else StreamError -2); StreamError -3 where
// Reader::header refuses
int64_t next_unit(const uint8_t* src, size_t n, bool at_eof, dcvc_stream_unit& u);

// sequence parameter sets by picture size, ids 0..15 (SPSHelper, stream_helper.py:157-192)
class SpsTable {
public:
    struct Sps { int id, height, width; };
    // id of the set for this size; is_new = it has to be written to the stream first
    int id_for(int height, int width, bool& is_new);
    void add(int id, int height, int width);          // decoder side: replaces an existing id
    const Sps* find(int id) const;

private:
    std::vector<Sps> m_sets;
};

}  // namespace stream
}  // namespace dcvc
