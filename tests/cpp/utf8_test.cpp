// utf8_test.cpp -- driver for tests/test_utf8_host.py: the decoding rule of gorp_amd/csrc/gx_utf8.hpp on the CPU, g++ alone.
// stdin:  per string  u32 length, the bytes.
// stdout: per string  u32 number of units, the units (u16), the byte each unit's item starts at (u32).
// Every string is decoded as a line in the MIDDLE of a buffer whose neighbours would complete its sequences if the rule looked
// outside the line: a lead F0 before it, continuation bytes behind it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gx_utf8.hpp"

int main() {
    std::vector<uint8_t> buf;
    std::vector<uint16_t> units;
    std::vector<uint32_t> at;
    uint32_t len = 0;
    while (fread(&len, 4, 1, stdin) == 1) {
        buf.assign(static_cast<size_t>(len) + 8, 0x80);
        buf[0] = buf[1] = buf[2] = 0x41;
        buf[3] = 0xF0;
        if (len && fread(buf.data() + 4, 1, len, stdin) != len) return 2;
        const uint64_t n = gx::utf8_transcode_line(buf.data(), 4, 4 + static_cast<int64_t>(len), nullptr, nullptr);
        units.assign(n + 1, 0);
        at.assign(n + 1, 0);
        if (gx::utf8_transcode_line(buf.data(), 4, 4 + static_cast<int64_t>(len), units.data(), at.data()) != n) return 3;
        const uint32_t n32 = static_cast<uint32_t>(n);
        fwrite(&n32, 4, 1, stdout);
        fwrite(units.data(), 2, n, stdout);
        fwrite(at.data(), 4, n, stdout);
    }
    return 0;
}
