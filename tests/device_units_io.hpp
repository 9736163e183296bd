// device_units_io.hpp -- the cases file and results file of the device-unit driver
// (tests/device_units.hip) and of its host-only companion (tests/round_decide_host.cpp); written and
// read by tests/device_units_common.py.  Plain C++, little-endian, every field 8-byte aligned.
//
//   cases:   "RHDUC001", u64 nbuf, nbuf x { u64 bytes, data padded to 8 },
//            u64 ncase, ncase x Case
//   results: "RHDUR001", then per output { char name[64], u64 bytes, data padded to 8 }
//
// A case names its input buffers by index (-1: none), so several cases share one array.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace du {

enum Op : uint32_t {
    OP_ROUND = 1,       // buf0: cnt x 15 u64 (l, h, L[5], R[5], n, sqrt_policy, b)
    OP_ROUND_SPANS = 2, // buf0: cnt x u64 spans; arg1 sqrt_policy, arg2 b (l = 0, h = n = span, rem.size = 1)
    OP_FP_ADDSUB = 3,   // buf0, buf1: cnt x 32 B operands
    OP_ACC_SEQ = 4,     // buf0: (cnt + 1) x u64 offsets, buf1: fingerprints; one thread per sequence
    OP_ACC_WAVE = 5,    // buf0: cnt x 64 x arg1 fingerprints; one wave per case
    OP_ACC_BLOCK = 6,   // buf0: cnt x arg2 x arg1 fingerprints; arg2 = NT, one workgroup per case
    OP_BLOCK_SUM = 7,   // buf0: cnt x 256 fingerprints; one workgroup per case
    OP_REDUCE = 8,      // arg0 n, arg1 stride; buf0 records
    OP_TOTAL = 9,       // arg0 n; buf0 entries (32 B)
    OP_RANGE = 10,      // arg0 n, arg1 stride, arg2 r, arg3 records; buf0 records, buf1 slots, buf2 bsums, buf3 ssums, buf4 lo, buf5 hi
    OP_PREFIX = 11,     // arg0 n, arg1 max_wgs, arg2 also launch_row_prefix; buf0 fps, buf1 bsums, buf2 ssums
    OP_BLOCK_PREFIX = 12 // arg0 n; buf0 bsums, buf1 ssums
};

struct Case {
    char name[40];
    uint32_t op, pad;
    uint64_t arg[4];
    int64_t buf[6];
};

struct Cases {
    std::vector<std::vector<uint8_t>> bufs;
    std::vector<Case> cases;
};

inline bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

inline bool load_cases(const char *path, Cases &c, std::string &why) {
    FILE *f = fopen(path, "rb");
    if (!f) return why = "cannot open the cases file", false;
    char magic[8];
    uint64_t nbuf = 0, ncase = 0;
    bool ok = read_exact(f, magic, 8) && !memcmp(magic, "RHDUC001", 8) && read_exact(f, &nbuf, 8) && nbuf < (1u << 20);
    for (uint64_t i = 0; ok && i < nbuf; i++) {
        uint64_t bytes = 0;
        ok = read_exact(f, &bytes, 8) && bytes < (1ull << 32);
        if (!ok) break;
        c.bufs.emplace_back((bytes + 7) & ~7ull);
        ok = read_exact(f, c.bufs.back().data(), c.bufs.back().size());
        c.bufs.back().resize(bytes);
    }
    ok = ok && read_exact(f, &ncase, 8) && ncase < (1u << 20);
    if (ok) {
        c.cases.resize(ncase);
        ok = read_exact(f, c.cases.data(), ncase * sizeof(Case));
    }
    fclose(f);
    if (!ok) return why = "malformed cases file", false;
    for (auto &k : c.cases) {
        k.name[sizeof k.name - 1] = 0;
        for (int64_t b : k.buf)
            if (b < -1 || b >= (int64_t)nbuf) return why = std::string("case ") + k.name + ": no such buffer", false;
    }
    return true;
}

struct Results {
    FILE *f = nullptr;
    bool open(const char *path) {
        f = fopen(path, "wb");
        return f && fwrite("RHDUR001", 1, 8, f) == 8;
    }
    bool put(const char *case_name, const char *what, const void *data, uint64_t bytes) {
        char name[64] = {0};
        snprintf(name, sizeof name, "%s/%s", case_name, what);
        const uint64_t pad = (8 - bytes % 8) % 8, zero = 0;
        return fwrite(name, 1, 64, f) == 64 && fwrite(&bytes, 8, 1, f) == 1 &&
               (bytes == 0 || fwrite(data, 1, bytes, f) == bytes) && (pad == 0 || fwrite(&zero, 1, pad, f) == pad);
    }
    bool close() {
        const bool ok = f && fclose(f) == 0;
        f = nullptr;
        return ok;
    }
};

}  // namespace du
