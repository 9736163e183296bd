// snap_ragged.hpp -- byte-granular locate and decode of an RCNL v1 snapshot whose entries carry
// their own lengths: String / Vec<u8> keys (RH_KEY_STR) and Vec<u8> / String values
// (RH_VAL_VARBYTES).  The RH_FORM_RAGGED route of rh_store_load_snapshot and
// rh_snapshot_decode_device (snap_ragged.hip; DESIGN.md "Ragged snapshot reload").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "store_kernels.hpp"

namespace rh {

// One bincode (fixint, LE) entry (K, Entry<Timestamp, V>):
//   [u64 L][key bytes]  phys u64 | logical u32 | node u64   variant u32   [u64 M][value bytes]
// variant 0 = State::Present (the value follows), 1 = State::Tombstone (the entry ends).
struct RagFmt {
    enum : uint32_t { KEY_RAW = 0, KEY_VEC = 1, KEY_STR = 2 };  // raw bytes | L == key_len | L <= key_len - 1
    enum : uint32_t { VAL_RAW = 0, VAL_VEC = 1, VAL_VAR = 2 };  // raw bytes | M == val_len | any M
    uint64_t len = 0;       // bytes in the file
    uint32_t key_mode = 0;
    uint32_t key_len = 0;   // bytes per row of the key column (STR: the row width W)
    uint32_t val_mode = 0;
    uint32_t val_len = 0;   // bytes per row of the value column (VAL_VAR: 0)
    uint32_t hdr = 0;       // most bytes of an entry the parser reads (everything but the value's bytes)
    uint32_t min_entry = 0; // shortest entry (an empty-key tombstone)
    uint32_t seg = 0;       // segment bytes S (a multiple of 16)
};
// segment bytes: RSOS_HIP_RAGGED_SEG (a multiple of 16 in [256, 32768]) or the measured default
uint32_t ragged_segment_bytes();

enum : uint32_t { RAG_OK = 0, RAG_EOF = 1, RAG_KEY_LEN = 2, RAG_VARIANT = 3, RAG_VAL_LEN = 4 };

// what the locate found (host copy of its result words)
struct RagResult {
    uint64_t parsed = 0;       // entries on the chain from offset 16 before it ends or breaks
    uint64_t last_seg = 0;     // segment holding entry n - 1 (parsed >= n)
    uint64_t bad_pos = 0;      // where the chain broke (parsed < n)
    uint64_t bad_len = 0;      // the u64 length read there (RAG_KEY_LEN / RAG_VAL_LEN)
    uint32_t why = RAG_OK;     // why it broke
    uint64_t segments = 0, rounds = 0, rewalked = 0;
};

struct RagTables {
    const uint64_t *first = nullptr;  // per segment: where its first entry starts
    const uint64_t *cnt = nullptr;    // per segment: entries starting in it
    const uint64_t *basev = nullptr;  // per segment: index of its first entry
    uint64_t *tomb = nullptr;         // per segment: tombstones among its decoded entries (the decode writes it)
    unsigned long long *words = nullptr;
};
// words written by the decode: tombstones among entries [0, n), end of entry n - 1
enum : int { RAGW_FI = 0, RAGW_LAST = 1, RAGW_PARSED = 2, RAGW_BAD = 3, RAGW_WHY = 4, RAGW_BADLEN = 5,
             RAGW_TOMB = 6, RAGW_END = 7, RAGW_N = 8 };

// The chain of entries from offset 16: guess per segment, fix-up rounds until a round changes
// nothing, scan of the counts.  Needs n >= 1.  Synchronises st (a read-back per round).
hipError_t ragged_locate(const RagFmt &f, const uint8_t *blob, uint64_t n, Scratch &s, hipStream_t st, RagTables *t,
                         RagResult *res);

// Columns of entries [0, n) (res.parsed >= n).  VAL_VAR: vlen gets the n value lengths and a
// trailing 0, vsrc the values' file offsets; ragged_copy_values then packs them behind their
// scanned offsets.  Otherwise values gets the rows (a tombstone's zero-filled).
struct RagCols {
    uint8_t *keys = nullptr;
    uint64_t *phys = nullptr;
    uint32_t *logical = nullptr;
    uint64_t *node = nullptr;
    uint8_t *tags = nullptr;
    uint8_t *values = nullptr;   // fixed-width rows, or the VAL_VAR heap
    uint64_t *voffs = nullptr;   // VAL_VAR: n + 1 offsets (out)
    uint64_t heap_cap = 0;       // VAL_VAR: bytes writable at values
};
// lists and decodes; VAL_VAR: leaves the scanned offsets in c.voffs (voffs[n] = the values' bytes)
hipError_t ragged_decode(const RagFmt &f, const uint8_t *blob, uint64_t n, const RagTables &t, const RagResult &res,
                         const RagCols &c, Scratch &s, hipStream_t st);
// the value bytes into place (VAL_VAR: the heap, never past heap_cap; fixed rows wider than 16 B)
hipError_t ragged_copy_values(const RagFmt &f, const uint8_t *blob, uint64_t n, const RagCols &c, Scratch &s,
                              hipStream_t st);

}  // namespace rh
