// The wave's inflate on one host lane, compiled from csrc/gsr_inflate_core.h ALONE with AddressSanitizer and UBSan
// (tests/test_inflate_sanitized.py builds and runs it): the tests of the library compare outputs, and a byte written behind `dst` or
// read behind lens[] / sorted[] changes no output.  Every buffer here is a heap block of exactly the size the decoder's contract
// names -- the stream rounded up to 4 bytes, dst of the expected length, Shared on its own -- so that one byte outside is a report.
//
//   inflate_sanitized FILE                  per stream one line "index status adler32-of-dst" (dst zero-filled before the call)
//   inflate_sanitized FILE --mutate SEED N  per stream N damaged variants; prints their number.  Nothing is compared: a report
//                                           ends the process with a non-zero status.
//
// FILE: uint32 count, then per stream uint32 stream bytes, uint32 expected bytes, the stream.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gsr_inflate_core.h"

namespace {

struct Stream {
    std::vector<uint8_t> bytes;
    uint32_t expected;
};

uint32_t adler32(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; ++i) {
        a = (a + p[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return (b << 16) | a;
}

// One call, every buffer exact.  *sum: the Adler-32 of dst afterwards.
int run(const uint8_t* bytes, size_t n, size_t expected, uint32_t* sum) {
    const size_t padded = (n + 3) / 4 * 4;
    uint8_t* src = static_cast<uint8_t*>(std::malloc(padded ? padded : 1));
    std::memset(src, 0, padded);
    std::memcpy(src, bytes, n);
    uint8_t* dst = static_cast<uint8_t*>(std::calloc(expected ? expected : 1, 1));
    if (expected == 0) {                     // a block of no bytes at all
        std::free(dst);
        dst = static_cast<uint8_t*>(std::malloc(0));
    }
    gsr::inflate::Shared* sh = static_cast<gsr::inflate::Shared*>(std::malloc(sizeof(gsr::inflate::Shared)));
    const int rc = gsr::inflate::inflate_zlib<1>(src, n, dst, expected, *sh);
    if (sum) *sum = adler32(dst, expected);
    std::free(sh);
    std::free(dst);
    std::free(src);
    return rc;
}

uint64_t g_state;
uint32_t rnd(uint32_t below) {               // xorshift64
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return below ? (uint32_t)((g_state >> 16) % below) : 0u;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2 && !(argc == 5 && std::strcmp(argv[2], "--mutate") == 0)) {
        std::fprintf(stderr, "usage: %s FILE [--mutate SEED N]\n", argv[0]);
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    uint32_t count = 0;
    if (!f || std::fread(&count, 4, 1, f) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<Stream> streams(count);
    for (Stream& s : streams) {
        uint32_t head[2];
        if (std::fread(head, 4, 2, f) != 2) return 2;
        s.bytes.resize(head[0]);
        s.expected = head[1];
        if (head[0] && std::fread(s.bytes.data(), 1, head[0], f) != head[0]) return 2;
    }
    std::fclose(f);

    if (argc == 2) {
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t sum = 0;
            const int rc = run(streams[k].bytes.data(), streams[k].bytes.size(), streams[k].expected, &sum);
            std::printf("%u %d %08x\n", k, rc, sum);
        }
        return 0;
    }

    g_state = std::strtoull(argv[3], nullptr, 0) | 1u;
    const int variants = std::atoi(argv[4]);
    uint64_t done = 0, accepted = 0;
    for (uint32_t k = 0; k < count; ++k) {
        for (int v = 0; v < variants; ++v) {
            std::vector<uint8_t> bytes = streams[k].bytes;
            size_t expected = streams[k].expected;
            const uint32_t n = (uint32_t)bytes.size();
            switch (rnd(5)) {
            case 0:                                                   // one bit flipped
                if (n) bytes[rnd(n)] ^= (uint8_t)(1u << rnd(8));
                break;
            case 1:                                                   // one byte replaced
                if (n) bytes[rnd(n)] = (uint8_t)rnd(256);
                break;
            case 2:                                                   // the tail cut
                bytes.resize(rnd(n + 1));
                break;
            case 3: {                                                 // another output size, 1 ... 300 off
                const uint32_t by = 1 + rnd(300);
                expected = rnd(2) ? expected + by : (expected > by ? expected - by : 0);
                break;
            }
            default: {                                                // the first half, then the second half of another stream
                const std::vector<uint8_t>& other = streams[rnd(count)].bytes;
                bytes.resize(n / 2);
                bytes.insert(bytes.end(), other.begin() + other.size() / 2, other.end());
            }
            }
            accepted += run(bytes.data(), bytes.size(), expected, nullptr) == 0;
            ++done;
        }
    }
    std::printf("mutations %llu accepted %llu\n", (unsigned long long)done, (unsigned long long)accepted);
    return 0;
}
