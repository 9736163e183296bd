// shard_route.hpp -- record columns partitioned by the sharded store's splitters, on the device
// (rh_route_columns_device, include/rsos_hip.h; the kernels: shard_route.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "store_kernels.hpp"

namespace rh {

constexpr int ROUTE_MAX_SHARDS = 64;    // rh_sstore_create's limit
constexpr uint32_t ROUTE_TILE = 2048;   // rows per workgroup: 256 threads, 8 steps of one row each
constexpr uint64_t ROUTE_ALIGN = 16;    // every shard's segment starts at a multiple of this many rows
constexpr int ROUTE_MAX_COLS = 7;       // keys, phys, logical, node, tags, values, ops

// One column to move: rows of `units` elements of `unit` bytes (16, 8, 4 or 1: the widest of them
// that divides the row; a segment start being a multiple of 16 rows keeps every unit aligned)
struct RouteCol {
    const uint8_t *src;
    uint8_t *dst;
    uint32_t unit;
    uint32_t units;
    int32_t shift;  // log2(units) when units is a power of two, else -1
};
RouteCol route_col(const void *src, void *dst, uint32_t row_bytes);

// The key order of the store kernels: key_bytes 4 or 8 with numeric = true (u32 / u64 keys, LE in
// memory), 8, 16, 32 or 64 with numeric = false (byte rows in memcmp order)
bool route_key_supported(uint32_t key_bytes, bool numeric);

struct RouteJob {
    const uint8_t *keys;  // the input key column (also one of cols)
    uint32_t key_bytes;
    bool numeric;
    uint64_t n;
    int shards;
    RouteCol cols[ROUTE_MAX_COLS];
    int ncols;
};

// A VARBYTES value column routed beside the job's fixed-width columns (rh_route_columns_var_device):
// value i of the input = bytes_in[offs_in[i] .. offs_in[i + 1]) clipped to limit_in (route_span), into
// a heap packed in output-row order.  Nothing is written at or past bytes_out + cap_out, nor past
// offs_out[R], R = the routed rows with their gaps; when the values (rounded up to 4) do not fit in
// cap_out no heap byte is written at all.
struct RouteVar {
    const uint8_t *bytes_in;
    const uint64_t *offs_in;
    uint64_t limit_in;
    uint8_t *bytes_out;
    uint64_t *offs_out;
    uint64_t cap_out;
};

// Partition the job's columns (n >= 1).  split: the shards - 1 splitter rows on the device.  meta
// (device, 2 * shards + 1 u64) receives the per-shard counts, then the segment starts (rows), then --
// with var -- the routed heap's bytes.  Scratch slots 120-121 hold the (shard, workgroup) counts and
// their scan, 124-126 each output row's value length, source offset and heap offset.  Asynchronous on st.
hipError_t launch_route(const RouteJob &job, const uint8_t *split, uint64_t *meta, Scratch &s, hipStream_t st,
                        const RouteVar *var = nullptr);

// *first (device) = the least i in [1, n) with key[i - 1] >= key[i] in that key order, or ~0 when
// the keys are strictly increasing (the word is preset on st by this call)
hipError_t launch_first_unsorted(const uint8_t *keys, uint32_t key_bytes, bool numeric, uint64_t n,
                                 unsigned long long *first, hipStream_t st);

}  // namespace rh
