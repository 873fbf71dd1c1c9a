// mx8_archive_check.cpp -- TorchArchive::parse and mx8_view over a good MX8 receipt and over mutations of it, as a
// stand-alone program that tests/test_mx8_archive_cpu.py builds with -fsanitize=address,undefined and runs on the CPU.
//
//   mx8_archive_check GOOD.pt [BAD.pt ...]
//
// GOOD.pt must be accepted, and every byte of the two views it hands out is read.  Then every truncation of it
// (each in a heap block of exactly its length, so a read past the end is the sanitizer's to report) is parsed and, if
// it parses, viewed and read the same way: none may be accepted as a receipt.  Every BAD.pt may parse but must not be
// accepted.  One JSON line; exit 0 if all of that held, 1 otherwise.
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

// Parses bytes[0, size) from a block of its own; 1 if it is an MX8 receipt (*n its elements; every byte of q and e
// read into *sum), 0 if not.
static int view(const std::string& bytes, size_t size, int64_t* n, unsigned long long* sum) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[size ? size : 1]);
    std::memcpy(block.get(), bytes.data(), size);
    TorchArchive ar;
    std::string err;
    if (!ar.parse(block.get(), size, &err)) return 0;
    const int8_t* q = nullptr;
    const uint8_t* e = nullptr;
    if (!ar.mx8_view(&q, &e, n)) return 0;
    for (int64_t i = 0; i < *n; ++i) *sum += (uint8_t)q[i];
    for (int64_t b = 0; b < (*n + 31) / 32; ++b) *sum += e[b];
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return std::cerr << "usage: mx8_archive_check GOOD.pt [BAD.pt ...]\n", 2;
    const std::string good = slurp(argv[1]);
    int64_t n = 0, tn = 0;
    unsigned long long sum = 0, tsum = 0;
    const int good_ok = view(good, good.size(), &n, &sum);
    int truncations_accepted = 0;
    for (size_t len = 0; len < good.size(); ++len) truncations_accepted += view(good, len, &tn, &tsum);
    int bad_accepted = 0;
    for (int i = 2; i < argc; ++i) {
        const std::string bad = slurp(argv[i]);
        if (bad.empty()) return std::cerr << "cannot read " << argv[i] << "\n", 2;
        if (view(bad, bad.size(), &tn, &tsum)) {
            std::cerr << "accepted as an MX8 receipt: " << argv[i] << "\n";
            ++bad_accepted;
        }
    }
    printf("{\"good\":%d,\"n\":%lld,\"sum\":%llu,\"truncations\":%zu,\"truncations_accepted\":%d,\"bad\":%d,"
           "\"bad_accepted\":%d}\n",
           good_ok, (long long)n, sum, good.size(), truncations_accepted, argc - 2, bad_accepted);
    return good_ok == 1 && truncations_accepted == 0 && bad_accepted == 0 ? 0 : 1;
}
