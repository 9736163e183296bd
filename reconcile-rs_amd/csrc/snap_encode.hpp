// snap_encode.hpp -- device columns into the head of an RCNL v1 snapshot: the inverse of the
// ragged decode (snap_ragged.hpp), behind rh_snapshot_encode_device (snap_encode.hip; DESIGN.md
// "Snapshot save").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "snap_ragged.hpp"
#include "store_kernels.hpp"

namespace rh {

// The columns read.  Of RagFmt the encoder uses key_mode / key_len / val_mode / val_len only.
struct EncCols {
    const uint8_t *keys = nullptr;      // n rows of key_len bytes (16-byte aligned)
    const uint64_t *phys = nullptr;
    const uint32_t *logical = nullptr;
    const uint64_t *node = nullptr;
    const uint8_t *tags = nullptr;      // nullable: all present
    const uint8_t *values = nullptr;    // fixed-width rows, or the VAL_VAR heap (4-byte aligned)
    const uint64_t *voffs = nullptr;    // VAL_VAR: n + 1 offsets
    uint64_t vlimit = 0;                // bytes readable at values (VAL_VAR: bytes_len)
};

struct EncSizes {
    uint64_t entry_bytes = 0;  // the n entries' bytes (the file's length is 16 more)
    uint64_t tombstones = 0;   // rows whose tag is not 0
};

// Every entry's length from its own row, the exclusive scan of the lengths (entry starts relative
// to offset 16, kept in the scratch for encode_write) and the tombstone count.  n >= 1.
// Synchronises st (one read-back).
hipError_t encode_measure(const RagFmt &f, const EncCols &c, uint64_t n, Scratch &s, hipStream_t st, EncSizes *sz);

// The 16-byte header and the n entries to out[0 .. 16 + entry_bytes) (out 16-byte aligned); after
// encode_measure of the same columns on the same scratch, or with n == 0 (the header alone).
// Enqueues on st and returns.
hipError_t encode_write(const RagFmt &f, const EncCols &c, uint64_t n, uint8_t *out, Scratch &s, hipStream_t st);

}  // namespace rh
