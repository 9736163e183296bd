// round_decide_host.cpp -- the host tier's decide_segment (csrc/round_decide.hpp) on the round cases
// of a device-unit cases file (device_units_io.hpp): the same inputs tests/device_units.hip gives
// the device's round_decide, so the two tiers and the reference are compared on one set.  Host-only,
// no HIP; every other case of the file is skipped.
//
//   round_decide_host <cases-file> <results-file>
#include "../reconcile-rs_amd/csrc/round_decide.hpp"
#include "device_units_io.hpp"

static rh_aggregate agg_of(const uint64_t *a) { return rh_aggregate{{a[0], a[1], a[2], a[3]}, a[4]}; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: round_decide_host <cases-file> <results-file>\n");
        return 2;
    }
    du::Cases cs;
    std::string why;
    if (!du::load_cases(argv[1], cs, why)) {
        fprintf(stderr, "round_decide_host: %s\n", why.c_str());
        return 2;
    }
    du::Results res;
    if (!res.open(argv[2])) return 2;
    bool ok = true;
    for (const du::Case &c : cs.cases) {
        const uint64_t cnt = c.arg[0];
        if (c.op == du::OP_ROUND) {
            const std::vector<uint8_t> &b = cs.bufs.at((size_t)c.buf[0]);
            if (b.size() != cnt * 15 * 8) return 2;
            const uint64_t *rec = (const uint64_t *)b.data();
            std::vector<uint64_t> out(cnt * 4);
            for (uint64_t i = 0; i < cnt; i++) {
                const uint64_t *r = rec + 15 * i;
                const rh::SegDecision d = rh::decide_segment(r[0], r[1], agg_of(r + 2), agg_of(r + 7), (int)r[13], r[14]);
                out[4 * i] = (uint64_t)d.kind, out[4 * i + 1] = d.stride, out[4 * i + 2] = d.children, out[4 * i + 3] = d.enums;
            }
            ok = ok && res.put(c.name, "out", out.data(), out.size() * 8);
        } else if (c.op == du::OP_ROUND_SPANS) {
            const std::vector<uint8_t> &b = cs.bufs.at((size_t)c.buf[0]);
            if (b.size() != cnt * 8) return 2;
            const uint64_t *spans = (const uint64_t *)b.data();
            std::vector<uint64_t> stride(cnt), children(cnt);
            std::vector<uint8_t> kind(cnt);
            for (uint64_t i = 0; i < cnt; i++) {
                const uint64_t L[5] = {1, 0, 0, 0, spans[i]}, R[5] = {0, 0, 0, 0, 1};
                const rh::SegDecision d = rh::decide_segment(0, spans[i], agg_of(L), agg_of(R), (int)c.arg[1], c.arg[2]);
                stride[i] = d.stride, children[i] = d.children, kind[i] = (uint8_t)d.kind;
            }
            ok = ok && res.put(c.name, "stride", stride.data(), cnt * 8) && res.put(c.name, "children", children.data(), cnt * 8) &&
                 res.put(c.name, "kind", kind.data(), cnt);
        }
    }
    return ok && res.close() ? 0 : 5;
}
