// jpeg_host_check.cpp — a stand-alone program (its own main, no HIP, no Python) that runs the shared decoder csrc/jpeg.h on the host over damaged
// input, meant to be built with the address and undefined-behaviour sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I yolo2-pytorch_amd/csrc tools/jpeg_host_check.cpp -o jpeg_host_check
//   ./jpeg_host_check tests/golden/jpeg
//
// Every buffer (file, scratch, destination) is a heap block of exactly the size handed to the decoder, so a read or write one byte outside is reported.
// Input: every *.jpg of the directory; for each file every truncation inside its scan (probed again), every single-byte flip inside its scan (the intact
// file's descriptor), a few thousand seeded random mutations of the whole file (probed again: the parser is under test too) and of the DESCRIPTOR (any
// contents must be safe: the decoder runs whenever jp_extents_ok accepts the record against the buffers of the intact image).
#define Y2_HD inline
#include "jpeg.h"

#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

namespace {

long long decoded = 0, refused = 0, damaged = 0;

// decode `file` with `desc` into exact-size buffers; returns the status (-1: the record does not fit)
int decode(const std::vector<uint8_t>& file, const JpDesc& desc, long long ws_cap = -1, int dst_h = -1, int dst_w = -1) {
    const JpLayout L = jp_layout(&desc);
    const int h = dst_h < 0 ? L.h : dst_h, w = dst_w < 0 ? L.w : dst_w;
    const long long ws_bytes = ws_cap < 0 ? L.bytes : ws_cap, stride = 3LL * w + 5, dst_bytes = (h - 1) * stride + 3LL * w;
    if (ws_bytes > (8LL << 20) || dst_bytes > (8LL << 20)) return -1;
    const int32_t geom[8] = {(int32_t)stride, h, w, 0, 0, h, w, 0};
    if (!jp_extents_ok(L, (long long)file.size(), 0, dst_bytes, 0, geom, ws_bytes)) { ++refused; return -1; }
    uint8_t* src = (uint8_t*)malloc(file.size() ? file.size() : 1);          // exact blocks, not vectors: capacity would hide an overrun
    uint8_t* ws = (uint8_t*)malloc((size_t)ws_bytes);
    uint8_t* dst = (uint8_t*)malloc((size_t)dst_bytes);
    memcpy(src, file.data(), file.size());
    const int status = jp_decode_image_host(&desc, L, src + L.scan_offset, ws, dst, stride);
    free(src); free(ws); free(dst);
    ++decoded;
    if (status) ++damaged;
    return status;
}

std::vector<uint8_t> read_file(const std::string& path) {
    std::vector<uint8_t> data;
    if (FILE* f = fopen(path.c_str(), "rb")) {
        uint8_t buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + n);
        fclose(f);
    }
    return data;
}

int probe(const std::vector<uint8_t>& file, JpDesc& d) {
    uint8_t* p = (uint8_t*)malloc(file.size() ? file.size() : 1);
    memcpy(p, file.data(), file.size());
    const int rc = jp_probe(p, (long long)file.size(), &d);
    free(p);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <directory of .jpg files> [random mutations per file]\n", argv[0]); return 2; }
    const int rounds = argc > 2 ? atoi(argv[2]) : 3000;
    std::vector<std::string> names;
    if (DIR* dir = opendir(argv[1])) {
        while (dirent* e = readdir(dir)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".jpg") names.push_back(n);
        }
        closedir(dir);
    }
    if (names.empty()) { fprintf(stderr, "no .jpg files in %s\n", argv[1]); return 2; }
    std::mt19937 rng(20);
    int supported = 0;
    for (const std::string& name : names) {
        const std::vector<uint8_t> file = read_file(std::string(argv[1]) + "/" + name);
        JpDesc desc;
        const int rc = probe(file, desc);
        if (rc == 0) {
            ++supported;
            if (decode(file, desc) != 0) { fprintf(stderr, "%s: the intact file decodes with a nonzero status\n", name.c_str()); return 1; }
            const JpLayout L = jp_layout(&desc);
            for (int k = 0; k < L.scan_bytes; ++k) {
                std::vector<uint8_t> cut(file.begin(), file.begin() + L.scan_offset + k);
                JpDesc d;
                if (probe(cut, d) == 0 && decode(cut, d) == 0) { fprintf(stderr, "%s: cut at scan byte %d decodes with status 0\n", name.c_str(), k); return 1; }
                std::vector<uint8_t> flip = file;
                flip[(size_t)L.scan_offset + k] ^= 0xFF;
                decode(flip, desc);
            }
            for (int r = 0; r < rounds; ++r) {          // the descriptor: any contents, against the buffers of the intact image
                JpDesc d = desc;
                uint8_t* bytes = reinterpret_cast<uint8_t*>(&d);
                const int n = 1 + (int)(rng() % 4);
                for (int i = 0; i < n; ++i) {
                    const size_t at = (r % 2) ? rng() % 96 : rng() % sizeof(JpDesc);          // half of them in the header fields
                    bytes[at] = (r % 3) ? (uint8_t)rng() : (uint8_t)(bytes[at] ^ (1u << (rng() % 8)));
                }
                decode(file, d, L.bytes, L.h, L.w);
            }
        }
        for (int r = 0; r < rounds; ++r) {              // the file: headers and scan alike, probed again
            std::vector<uint8_t> m = file;
            const int n = 1 + (int)(rng() % 4);
            for (int i = 0; i < n; ++i) m[rng() % m.size()] = (r % 3) ? (uint8_t)rng() : (uint8_t)(m[rng() % m.size()] ^ (1u << (rng() % 8)));
            if (r % 7 == 0) m.resize(rng() % (m.size() + 1));
            JpDesc d;
            if (probe(m, d) == 0) decode(m, d);
        }
    }
    printf("%d files (%d supported): %lld decodes, %lld with a nonzero status, %lld records refused by the extent check\n", (int)names.size(), supported,
           decoded, damaged, refused);
    return 0;
}
