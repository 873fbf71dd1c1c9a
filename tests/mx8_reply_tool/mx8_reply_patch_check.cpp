// mx8_reply_patch_check.cpp -- TorchArchive::with_mx8_into over a good MX8 receipt and over mutations of it, as a
// stand-alone program that tests/test_mx8_reply_archive_cpu.py builds with -fsanitize=address,undefined and runs on
// the CPU.
//
//   mx8_reply_patch_check GOOD.pt Q.bin E.bin OUT.pt [BAD.pt ...]
//
// GOOD.pt, an MX8 receipt of n codes, is the template; Q.bin (n bytes) and E.bin (ceil(n / 32) bytes) are patched into
// a copy of it, which is written to OUT.pt.  The copy must parse again, hand out exactly Q and E, and every record's
// stored CRC-32 must be zlib's over the record's bytes.  Then the patcher must refuse -- and leave the destination
// untouched: another n, null codes, every truncation of GOOD.pt that still parses, and every BAD.pt.  Templates and
// destinations lie in heap blocks of exactly their length, so an access past either end is the sanitizer's to report.
// One JSON line; exit 0 if all of that held, 1 otherwise.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "archive.h"

using namespace fahost;

static std::string slurp(const char* p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// Patches (q, e, n) into bytes[0, size), parsed from a block of its own, into a destination of its own filled with
// 0xA5.  1: patched (*out the copy); 0: refused with the destination untouched; -1: refused, but the destination was
// written.
static int patch(const std::string& bytes, size_t size, const int8_t* q, const uint8_t* e, int64_t n, std::string* out) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[size ? size : 1]);
    std::memcpy(block.get(), bytes.data(), size);
    TorchArchive ar;
    std::string err;
    if (!ar.parse(block.get(), size, &err)) return 0;
    std::unique_ptr<uint8_t[]> dst(new uint8_t[size ? size : 1]);
    std::memset(dst.get(), 0xA5, size);
    if (ar.with_mx8_into(q, e, n, dst.get(), &err)) {
        if (out) out->assign((const char*)dst.get(), size);
        return 1;
    }
    for (size_t i = 0; i < size; ++i)
        if (dst[i] != 0xA5) return -1;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) return std::cerr << "usage: mx8_reply_patch_check GOOD.pt Q.bin E.bin OUT.pt [BAD.pt ...]\n", 2;
    const std::string good = slurp(argv[1]), qs = slurp(argv[2]), es = slurp(argv[3]);
    const int64_t n = (int64_t)qs.size();
    if (good.empty() || (int64_t)es.size() != (n + 31) / 32) return std::cerr << "bad inputs\n", 2;
    const int8_t* q = (const int8_t*)qs.data();
    const uint8_t* e = (const uint8_t*)es.data();
    std::string out;
    int good_ok = patch(good, good.size(), q, e, n, &out) == 1;
    int crc_ok = 0, records = 0, same = 0;
    if (good_ok) {
        std::ofstream(argv[4], std::ios::binary).write(out.data(), (std::streamsize)out.size());
        TorchArchive ar;
        std::string err;
        const int8_t* pq = nullptr;
        const uint8_t* pe = nullptr;
        int64_t pn = 0;
        if (ar.parse((const uint8_t*)out.data(), out.size(), &err) && ar.mx8_view(&pq, &pe, &pn) && pn == n)
            same = std::memcmp(pq, q, (size_t)n) == 0 && std::memcmp(pe, e, es.size()) == 0;
        for (const ZipEntry& z : ar.entries()) {
            if (z.method != 0) continue;  // a deflated record (never a tensor's): the test reads it with zlib
            ++records;
            const uint32_t c = (uint32_t)::crc32(0L, (const Bytef*)out.data() + z.data_offset, (uInt)z.size);
            crc_ok += c == z.crc;
        }
    }
    int refused_wrong = 0, dirty = 0;
    for (int r : {patch(good, good.size(), q, e, n + 1, nullptr), patch(good, good.size(), q, e, n - 1, nullptr),
                  patch(good, good.size(), q, e, n + 32, nullptr), patch(good, good.size(), q, e, 0, nullptr),
                  patch(good, good.size(), nullptr, e, n, nullptr), patch(good, good.size(), q, nullptr, n, nullptr)}) {
        refused_wrong += r == 0;
        dirty += r < 0;
    }
    int truncations_patched = 0;
    for (size_t len = 0; len < good.size(); ++len) {
        const int r = patch(good, len, q, e, n, nullptr);
        truncations_patched += r == 1;
        dirty += r < 0;
    }
    int bad_patched = 0;
    for (int i = 5; i < argc; ++i) {
        const std::string bad = slurp(argv[i]);
        if (bad.empty()) return std::cerr << "cannot read " << argv[i] << "\n", 2;
        const int r = patch(bad, bad.size(), q, e, n, nullptr);
        if (r == 1) std::cerr << "patched as an MX8 reply: " << argv[i] << "\n";
        bad_patched += r == 1;
        dirty += r < 0;
    }
    printf("{\"good\":%d,\"n\":%lld,\"same\":%d,\"records\":%d,\"crc_ok\":%d,\"refused_wrong\":%d,\"truncations\":%zu,"
           "\"truncations_patched\":%d,\"bad\":%d,\"bad_patched\":%d,\"dirty\":%d}\n",
           good_ok, (long long)n, same, records, crc_ok, refused_wrong, good.size(), truncations_patched, argc - 5,
           bad_patched, dirty);
    return good_ok && same && records > 0 && crc_ok == records && refused_wrong == 6 && truncations_patched == 0 &&
                   bad_patched == 0 && dirty == 0
               ? 0
               : 1;
}
