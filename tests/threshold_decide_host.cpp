// threshold_decide_host.cpp -- the host tier's decide_segment (csrc/round_decide.hpp) with
// EnumerateBelowThreshold's threshold, on records a test writes as text.  Host-only, no HIP.
//
//   threshold_decide_host <records-file> <results-file>
//
// A record is one line of 15 decimal u64: lo hi, the local aggregate (4 limbs, size), the remote
// aggregate (4 limbs, size), sqrt_policy, fan-out, threshold.  A result is one line: kind stride
// children enums, from the seven-argument call; a record whose threshold is 0 is also decided by
// the six-argument call (the parent's), and the two must be the same decision.
#include <cinttypes>
#include <cstdio>

#include "../reconcile-rs_amd/csrc/round_decide.hpp"

static rh_aggregate agg_of(const uint64_t *a) { return rh_aggregate{{a[0], a[1], a[2], a[3]}, a[4]}; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: threshold_decide_host <records-file> <results-file>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    uint64_t r[15];
    for (;;) {
        int got = 0;
        for (int i = 0; i < 15; i++) got += fscanf(in, "%" SCNu64, &r[i]) == 1;
        if (got == 0) break;
        if (got != 15) return 3;
        const rh::SegDecision d = rh::decide_segment(r[0], r[1], agg_of(r + 2), agg_of(r + 7), (int)r[12], r[13], r[14]);
        if (r[14] == 0) {
            const rh::SegDecision p = rh::decide_segment(r[0], r[1], agg_of(r + 2), agg_of(r + 7), (int)r[12], r[13]);
            if (p.kind != d.kind || p.stride != d.stride || p.children != d.children || p.enums != d.enums) return 4;
        }
        fprintf(out, "%d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", d.kind, d.stride, d.children, d.enums);
    }
    return fclose(out) == 0 ? 0 : 5;
}
