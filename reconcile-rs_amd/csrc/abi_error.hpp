// abi_error.hpp -- what the library's other sources (sharded_store.hip, shard_route.hip, wire_codec.cpp)
// call in rsos_hip_abi.hip, which defines it all: the thread's error string, the fail points, the argument
// checks and the two halves of a store's protocol round.  One set of declarations for every caller, seen
// by the definitions too.  No HIP here: wire_codec.cpp is built by the host compiler.
#pragma once
#include <cstddef>
#include <string>

#include "../../include/rsos_hip.h"

namespace rh {
int set_error(int code, const std::string &msg);  // the calling thread's rh_last_error; returns code
bool debug_fail_point(const char *name);          // rh_debug_fail_point, armed on the calling thread
int check_schema_arg(const rh_schema *s);         // check_schema: RH_ERR_ARG naming the bad field
// host key rows of a RH_KEY_STR schema (length byte, zero padding), RH_ERR_ARG naming the first bad
// row; RH_OK for every other key kind.  Checked here for the whole batch before any shard changes
int check_str_rows(const rh_schema &s, const void *keys, size_t n);
// rh_store_protocol_round in two halves (rsos_hip_abi.hip round_entry): a device round issued
// (*pending: the store stays locked) and completed later on the same thread.  threshold != 0: the
// round of rh_store_protocol_round_threshold (policy is then RH_POLICY_FIXED_FAN_OUT)
int store_round_issue(rh_store *s, int policy, uint64_t fan_out, const rh_segments *active, rh_segments *children,
                      rh_segments *enumerations, rh_round_outcome *outcome, bool *pending, uint64_t threshold = 0);
int store_round_complete(rh_store *s, rh_segments *children, rh_segments *enumerations, rh_round_outcome *outcome);
// what both enumerate entry points check before any device call: NULL arguments, the bound kinds and
// key arrays (rh_store_resolve_segments' rule), max_rows (0 becomes 2^22, more is RH_ERR_ARG); *out zeroed
int check_enumerate_args(const void *store, const rh_segments *ranges, uint64_t *max_rows, rh_enumerated *out);
// rh_store_enumerate_segments for a shard: ranges that hold more than max_rows rows are no error
// here -- *over = true, `out` filled without rows -- since the map weighs the shards' totals together
int store_enumerate(rh_store *s, const rh_segments *ranges, uint64_t max_rows, rh_enumerated *out, bool *over);
}  // namespace rh
