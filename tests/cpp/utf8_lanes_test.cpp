// utf8_lanes_test.cpp -- the lane logic of gx_utf8.hip's count / write kernel on the CPU, g++ alone: 16 lanes take a line 256 bytes
// a pass, each with one aligned 16-byte chunk, the bytes either side from the neighbouring lanes' words (here: array elements in
// place of __shfl) or, at the group's edges, from utf8_edge_prev / utf8_edge_next; a group scan gives each lane its first unit.
// Everything but the shuffles is the kernel's own code (gx_utf8.hpp).  Compared with utf8_transcode_line, units and unit -> byte
// map, on random lines at every alignment, with poison behind the units and neighbours that would complete the line's sequences.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gx_utf8.hpp"

using namespace gx;

int main() {
    srand(5);
    const uint8_t alpha[] = {0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF,
                             0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF};
    long checked = 0;
    for (int iter = 0; iter < 20000; ++iter) {
        const int pre = 1024 + iter % 16, len = rand() % 600, post = 64;
        std::vector<uint8_t> buf(pre + len + post);
        for (auto& b : buf) b = (rand() % 3) ? alpha[rand() % 24] : static_cast<uint8_t>(0x20 + rand() % 0x5F);
        if (rand() % 4 == 0)   // mostly ASCII: the fast path
            for (int i = pre; i < pre + len; ++i) if (rand() % 5) buf[i] = static_cast<uint8_t>('a' + rand() % 26);
        const uint64_t a0 = pre, a_end = pre + len;
        const auto load = [&](uint64_t a) { return buf[a]; };
        std::vector<uint16_t> want(2 * len + 2), got(2 * len + 40, 0xEEEE);
        std::vector<uint32_t> wat(2 * len + 2), gat(2 * len + 40, 0xEEEEEEEEu);
        const uint64_t n = utf8_transcode_line(buf.data(), static_cast<int64_t>(a0), static_cast<int64_t>(a_end), want.data(), wat.data());
        uint64_t run = 0;
        for (uint64_t c = a0 & ~15ull; c < a_end; c += 256) {
            uint32_t d[16][4], cnt[16];
            bool live[16], ascii[16];
            Utf8Window x[16];
            for (int gl = 0; gl < 16; ++gl) {   // the lanes' loads (bytes outside the line come as they lie in memory: the window masks them)
                const uint64_t ca = c + gl * 16;
                live[gl] = ca < a_end;
                for (int q = 0; q < 4; ++q) {
                    d[gl][q] = 0;
                    if (live[gl]) for (int r = 0; r < 4; ++r) d[gl][q] |= static_cast<uint32_t>(buf[ca + 4 * q + r]) << (8 * r);
                }
            }
            for (int gl = 0; gl < 16; ++gl) {
                const uint64_t ca = c + gl * 16;
                uint32_t prev = gl ? d[gl - 1][3] : 0u, next = gl < 15 ? d[gl + 1][0] : 0u;
                if (gl == 0) prev = utf8_edge_prev(load, ca, a0, a_end);
                if (gl == 15) next = utf8_edge_next(load, ca, a_end);
                const bool whole = ca >= a0 && ca + 16 <= a_end;
                ascii[gl] = whole && ((d[gl][0] | d[gl][1] | d[gl][2] | d[gl][3]) & 0x80808080u) == 0;
                cnt[gl] = 0;
                if (ascii[gl]) cnt[gl] = 16;
                else if (live[gl]) {
                    x[gl] = utf8_make_window(d[gl], prev, next, ca, a0, a_end);
                    cnt[gl] = utf8_chunk_units(x[gl], [](int, uint32_t, uint16_t) {});
                }
            }
            for (int gl = 0; gl < 16; ++gl) {   // (the group scan: the lanes before this one)
                const uint64_t ca = c + gl * 16;
                const uint32_t byte0 = static_cast<uint32_t>(ca - a0);
                uint64_t at = run;
                if (ascii[gl]) {
                    uint32_t pair[8];
                    utf8_widen_ascii(d[gl], pair);
                    for (int q = 0; q < 8; ++q) { got[at + 2 * q] = static_cast<uint16_t>(pair[q]); got[at + 2 * q + 1] = static_cast<uint16_t>(pair[q] >> 16); }
                    for (uint32_t j = 0; j < 16; ++j) gat[at + j] = byte0 + j;
                } else if (live[gl]) {
                    utf8_chunk_units(x[gl], [&](int j, uint32_t, uint16_t unit) { got[at] = unit; gat[at] = byte0 + static_cast<uint32_t>(j); ++at; });
                }
                run += cnt[gl];
            }
        }
        if (run != n || memcmp(want.data(), got.data(), n * 2) || memcmp(wat.data(), gat.data(), n * 4) || got[n] != 0xEEEE) {
            printf("MISMATCH iteration %d: %d bytes at alignment %d, %llu units expected, %llu made\n", iter, len, pre % 16,
                   static_cast<unsigned long long>(n), static_cast<unsigned long long>(run));
            return 1;
        }
        checked += len;
    }
    printf("utf8 lanes checks ok, %ld bytes\n", checked);
    return 0;
}
