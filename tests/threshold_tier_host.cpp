// threshold_tier_host.cpp -- HostTier::round (csrc/host_tier.hpp) under EnumerateBelowThreshold, on a
// map and rounds a test writes as text; the test compares every round with oracle/rbsr.py.  Host-only.
//
//   threshold_tier_host <input-file> <results-file>
//
// Input, one item a line (keys as 2 * kl hex digits, a fingerprint as four decimal u64 limbs):
//   K <kl>                                    16-byte keys in bytes order (RH_KEY_BYTES)
//   B <key> <fp>                              a base row, in key order
//   D <key> <live 0|1> <fp>                   a later batch's row (sorted, distinct): upsert or delete,
//                                             folded into the tier's delta tree
//   R <threshold> <fan-out> <segments>        a round, followed by its segments:
//   S <sk> <start key> <ek> <end key> <fp> <size>
// Results: per round "R skipped enumerated split children dropped", then its children
// "C <sk> <start key> <ek> <end key> <fp> <size>" and enumerations "E <sk> <start key> <ek> <end key>".
// Each round is run with the batched searches and key by key; the two must agree byte for byte.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../reconcile-rs_amd/csrc/host_tier.hpp"

static bool unhex(const char *s, uint8_t *out, uint32_t kl) {
    if (strlen(s) != 2 * kl) return false;
    for (uint32_t i = 0; i < kl; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static void hex(FILE *f, const uint8_t *k, uint32_t kl) {
    for (uint32_t i = 0; i < kl; i++) fprintf(f, "%02x", k[i]);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: threshold_tier_host <input-file> <results-file>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 2;
    uint32_t kl = 0;
    std::vector<uint8_t> bkeys, dkeys, dlive;
    std::vector<uint64_t> prefix(4, 0), dfps;
    rh::HostTier T;
    bool built = false;
    // the base copy, then the batch folded into the delta tree, before the first round
    auto build = [&]() {
        const uint64_t nb = bkeys.size() / kl, nd = dlive.size();
        bkeys.resize(bkeys.size() + 64);
        dkeys.resize(dkeys.size() + 64);
        T.build(kl, RH_KEY_BYTES, nb, bkeys.data(), prefix.data());
        std::vector<rh::DeltaTree::Rec> rows(nd);
        std::vector<uint8_t> drop(nd);
        for (uint64_t j = 0; j < nd; j++)
            drop[j] = T.entry_vs_base(dkeys.data() + j * kl, dlive[j] ? &dfps[4 * j] : nullptr, &rows[j]);
        T.fold(rows.data(), drop.data(), nd);
        built = true;
    };
    char tag[8], a[160], b[160];
    while (fscanf(in, "%7s", tag) == 1) {
        if (tag[0] == 'K') {
            if (fscanf(in, "%u", &kl) != 1 || kl == 0 || kl > 64) return 3;
        } else if (tag[0] == 'B') {
            uint64_t f[4];
            if (fscanf(in, "%159s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, a, &f[0], &f[1], &f[2], &f[3]) != 5) return 3;
            bkeys.resize(bkeys.size() + kl);
            if (!unhex(a, bkeys.data() + bkeys.size() - kl, kl)) return 3;
            uint64_t acc[4];
            memcpy(acc, &prefix[prefix.size() - 4], 32);
            rh::fp4_add(acc, f);
            prefix.insert(prefix.end(), acc, acc + 4);
        } else if (tag[0] == 'D') {
            uint64_t f[4];
            unsigned live;
            if (fscanf(in, "%159s %u %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, a, &live, &f[0], &f[1], &f[2], &f[3]) != 6)
                return 3;
            dkeys.resize(dkeys.size() + kl);
            if (!unhex(a, dkeys.data() + dkeys.size() - kl, kl)) return 3;
            dlive.push_back((uint8_t)live);
            dfps.insert(dfps.end(), f, f + 4);
        } else if (tag[0] == 'R') {
            uint64_t thr, fan, r;
            if (fscanf(in, "%" SCNu64 " %" SCNu64 " %" SCNu64, &thr, &fan, &r) != 3) return 3;
            if (!built) build();
            std::vector<uint8_t> sk(r + 1), ek(r + 1), skeys(r * kl + 1), ekeys(r * kl + 1);
            std::vector<rh_aggregate> rem(r + 1);
            for (uint64_t j = 0; j < r; j++) {
                unsigned s, e;
                uint64_t *f = rem[j].fingerprint;
                if (fscanf(in, "%7s %u %159s %u %159s %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, tag, &s, a, &e,
                           b, &f[0], &f[1], &f[2], &f[3], &rem[j].size) != 10 || tag[0] != 'S')
                    return 3;
                sk[j] = (uint8_t)s, ek[j] = (uint8_t)e;
                if (!unhex(a, &skeys[j * kl], kl) || !unhex(b, &ekeys[j * kl], kl)) return 3;
            }
            rh_segments seg{sk.data(), skeys.data(), ek.data(), ekeys.data(), rem.data(), (size_t)r, (size_t)r};
            std::vector<uint8_t> o, o2;
            uint64_t h[5], h2[5];
            T.batch = true;
            T.round(0, fan < 2 ? 2 : fan, seg, o, h, thr);
            T.batch = false;
            T.round(0, fan < 2 ? 2 : fan, seg, o2, h2, thr);
            T.batch = true;
            if (o != o2 || memcmp(h, h2, sizeof h)) return 4;
            const uint64_t nc = h[3], ne = h[1];
            const rh::RoundLayout L = rh::round_layout(nc, ne, kl);
            fprintf(out, "R %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", h[0], h[1], h[2], h[3], h[4]);
            for (uint64_t c = 0; c < nc; c++) {
                const uint64_t *g = reinterpret_cast<const uint64_t *>(o.data() + L.caggs) + 5 * c;
                fprintf(out, "C %u ", o[L.csk + c]);
                hex(out, o.data() + L.cskeys + c * kl, kl);
                fprintf(out, " %u ", o[L.cek + c]);
                hex(out, o.data() + L.cekeys + c * kl, kl);
                fprintf(out, " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", g[0], g[1], g[2], g[3], g[4]);
            }
            for (uint64_t e = 0; e < ne; e++) {
                fprintf(out, "E %u ", o[L.esk + e]);
                hex(out, o.data() + L.eskeys + e * kl, kl);
                fprintf(out, " %u ", o[L.eek + e]);
                hex(out, o.data() + L.eekeys + e * kl, kl);
                fprintf(out, "\n");
            }
        } else {
            return 3;
        }
    }
    return fclose(out) == 0 ? 0 : 5;
}
