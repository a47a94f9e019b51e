// Stand-alone host check of the feed-style container parser (dcvc_stream_next_unit, dcvc_amd/csrc/stream/container.cpp), meant
// for a sanitizer build on the CPU - no GPU, no Python:
//
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I dcvc_amd/csrc \
//       tools/stream_feed_check.cpp dcvc_amd/csrc/stream/container.cpp -o /tmp/stream_feed_check && /tmp/stream_feed_check
//
// The prefix and feeding cases of tests/test_stream_units_cpu.py, with every buffer handed to the parser allocated at exactly
// the length it is told, so that a read past the end is an error the sanitizer reports. Exit status 0 and "ok" when all holds.
#include "capi_common.h"
#include "dcvc_amd_stream.h"
#include "stream/container.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

extern "C" const char* dcvc_last_error(void) { return dcvc::last_error().c_str(); }

namespace {

int failures = 0;

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            if (++failures < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
        }                                                                                \
    } while (0)

struct Unit {
    size_t start, bytes;
    bool sps;
    std::vector<uint8_t> payload;
};

// the parser on a copy of exactly n bytes
int64_t parse(const uint8_t* src, size_t n, int at_eof, dcvc_stream_unit* u)
{
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n]);
    if (n) std::memcpy(exact.get(), src, n);
    return dcvc_stream_next_unit(exact.get(), n, at_eof, u);
}

}  // namespace

int main()
{
    std::vector<uint8_t> data;
    std::vector<Unit> units;
    unsigned seed = 12345;
    auto rnd = [&]() { return static_cast<uint8_t>((seed = seed * 1103515245u + 12345u) >> 16); };
    auto add_sps = [&](int id, int h, int w) {
        const size_t at = data.size();
        dcvc::stream::put_sps(data, id, h, w);
        units.push_back(Unit{at, data.size() - at, true, {}});
    };
    const size_t lengths[] = {0, 1, 127, 128, 16383, 16384, 70000};
    add_sps(0, 1080, 1920);
    for (size_t i = 0; i < 7; ++i) {
        if (i == 3) add_sps(1, 96, 128);
        std::vector<uint8_t> pl(lengths[i]);
        for (uint8_t& b : pl) b = rnd();
        const size_t at = data.size();
        dcvc::stream::put_ip(data, i % 3 == 0, static_cast<int>(i % 2), rnd(), rnd() & 127, rnd() & 1, pl.data(), pl.size());
        units.push_back(Unit{at, data.size() - at, false, pl});
    }
    dcvc_stream_unit u;
    // every strict prefix of every unit
    for (const Unit& un : units) {
        for (size_t k = 0; k < un.bytes; ++k) {
            CHECK(parse(data.data() + un.start, k, 0, &u) == 0 && u.need > k && u.need <= un.bytes && u.unit_bytes == 0);
            const int64_t rc = parse(data.data() + un.start, k, 1, &u);
            CHECK(k == 0 ? (rc == 0 && u.need == 0) : rc == -2);
        }
        CHECK(parse(data.data() + un.start, un.bytes, 0, &u) == static_cast<int64_t>(un.bytes));
        CHECK(un.sps ? u.nal_type == DCVC_NAL_SPS
                     : (u.payload_bytes == un.payload.size() && u.payload_offset + u.payload_bytes == un.bytes &&
                        (un.payload.empty() ||
                         std::memcmp(data.data() + un.start + u.payload_offset, un.payload.data(), un.payload.size()) == 0)));
    }
    // feeding: one byte at a time, and in reads of exactly `need`
    for (int by_need = 0; by_need < 2; ++by_need) {
        size_t start = 0, have = 0, seen = 0;
        for (;;) {
            const int64_t rc = parse(data.data() + start, have - start, have == data.size(), &u);
            CHECK(rc >= 0);
            if (rc < 0) break;
            if (rc > 0) {
                CHECK(seen < units.size() && units[seen].start == start && units[seen].bytes == static_cast<size_t>(rc));
                ++seen;
                start += static_cast<size_t>(rc);
                continue;
            }
            if (u.need == 0) break;
            have = by_need ? start + u.need : have + 1;
            CHECK(have <= data.size());
            if (have > data.size()) break;
        }
        CHECK(seen == units.size() && start == data.size());
    }
    // malformed: an unknown unit type, whatever follows
    const uint8_t bad[] = {0x70, 1, 2, 3};
    CHECK(parse(bad, 1, 0, &u) == -3 && std::strstr(dcvc_last_error(), "unknown unit type") != nullptr);
    CHECK(parse(bad, sizeof(bad), 1, &u) == -3);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ok: %zu units, %zu bytes\n", units.size(), data.size());
    return 0;
}
