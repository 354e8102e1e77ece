// An 8-bit RGB, non-interlaced PNG file written with the standard library alone (the CLI's -o; tools/asan_sketch_image.cpp): every
// row with filter 0 in front, the zlib stream made of stored (uncompressed) deflate blocks, CRC-32 and Adler-32 computed here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace ezpz {
namespace png {

inline uint32_t crc32(const uint8_t* data, size_t n, uint32_t crc = 0) {
    static uint32_t table[256];
    static bool made = false;
    if (!made) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        made = true;
    }
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ data[i]) & 0xFFu] ^ (crc >> 8);
    return ~crc;
}

inline uint32_t adler32(const uint8_t* data, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n;) {
        const size_t stop = i + 5552 < n ? i + 5552 : n;  // (the longest run whose sums stay below 2^32)
        for (; i < stop; ++i) {
            a += data[i];
            b += a;
        }
        a %= 65521u;
        b %= 65521u;
    }
    return (b << 16) | a;
}

inline void put_be32(std::vector<uint8_t>& out, uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) out.push_back((uint8_t)(v >> s));
}

inline void put_chunk(std::vector<uint8_t>& out, const char tag[4], const std::vector<uint8_t>& body) {
    put_be32(out, (uint32_t)body.size());
    const size_t start = out.size();
    for (int i = 0; i < 4; ++i) out.push_back((uint8_t)tag[i]);
    out.insert(out.end(), body.begin(), body.end());
    put_be32(out, crc32(out.data() + start, out.size() - start));
}

// rgb [height][width][3], the top row first
inline std::vector<uint8_t> encode(const uint8_t* rgb, uint32_t width, uint32_t height) {
    std::vector<uint8_t> raw;
    raw.reserve((size_t)height * (3 * (size_t)width + 1));
    for (uint32_t y = 0; y < height; ++y) {
        raw.push_back(0);
        raw.insert(raw.end(), rgb + (size_t)y * width * 3, rgb + (size_t)(y + 1) * width * 3);
    }
    std::vector<uint8_t> z;
    z.reserve(raw.size() + raw.size() / 65535 * 5 + 16);
    z.push_back(0x78), z.push_back(0x01);
    size_t at = 0;
    do {
        const size_t len = raw.size() - at < 65535 ? raw.size() - at : 65535;
        z.push_back(at + len == raw.size() ? 1 : 0);  // BFINAL, BTYPE 00
        z.push_back((uint8_t)(len & 0xFF)), z.push_back((uint8_t)(len >> 8));
        z.push_back((uint8_t)(~len & 0xFF)), z.push_back((uint8_t)((~len >> 8) & 0xFF));
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + len);
        at += len;
    } while (at < raw.size());
    put_be32(z, adler32(raw.data(), raw.size()));
    static const uint8_t magic[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    std::vector<uint8_t> out(magic, magic + 8);
    std::vector<uint8_t> header;
    put_be32(header, width), put_be32(header, height);
    header.push_back(8), header.push_back(2), header.push_back(0), header.push_back(0), header.push_back(0);
    put_chunk(out, "IHDR", header);
    put_chunk(out, "IDAT", z);
    put_chunk(out, "IEND", std::vector<uint8_t>());
    return out;
}

inline bool write_file(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height) {
    const std::vector<uint8_t> data = encode(rgb, width, height);
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool good = std::fwrite(data.data(), 1, data.size(), f) == data.size();
    return std::fclose(f) == 0 && good;
}

}  // namespace png
}  // namespace ezpz
