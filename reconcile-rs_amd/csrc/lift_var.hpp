// lift_var.hpp -- the lift of records whose value is a run of bytes of per-record length
// (RH_VAL_VARBYTES: Vec<u8> / String / &str, rsos/src/encoding/serializer.rs:105-113): a
// fixed-width key column, stamp and tag columns as for the schema kernels, and the values packed
// back to back in a heap with n + 1 offsets.
//
// The message of a present record is the prefix -- key words (with the u64 length of a byte key),
// the 5 stamp words (DATED), the State variant word (DATED / PROJECTION) and the value's u64
// length -- followed by the value's bytes; a tombstone's is the prefix up to the variant word
// (LEN_TOMB bytes, one block for every key shape here).  The prefix is built in registers from the
// columns, as build_prefix does for the fixed-width kernels: no framing byte exists in HBM.  P
// is a multiple of 4, so the prefix words are whole words of the message; the value starts
// anywhere in the heap and comes through the byte-granular loaders of msg_reader.hpp.
//
// Read per record: key + stamp + tag + one 8 B offset + the value bytes; written: 32 B.
//
// Two kernels, the encoded path's split: messages of one chunk (<= 1,024 B) go through a
// lane-refill loop (a wave owns 256 consecutive records, every iteration compresses one block
// per lane, a finished lane claims the wave's next record), so a wave is not held to its longest
// record; longer ones take one lane each through hash_message (CV stack, parent nodes).
#pragma once
#include "lift_kernels.hpp"
#include "msg_reader.hpp"

namespace rh {

constexpr int VAR_PER_WAVE = 64 * 4;

// The message of one record as a reader: prefix words from the columns, then the value span.
// The column pointers are rebased (in scalar registers) to the first row of the wave's or
// workgroup's range and the record is a 32-bit row within it, so every per-lane column address is
// a 32-bit offset from a scalar base, as in k_lift: no 64-bit VALU address arithmetic.
template <int KK, int KL, int RK>
struct VarReader {
    using L = Layout<KK, KL, VAL_BYTES, 0, RK>;  // a byte value's framing: P ends with its u64 length
    static constexpr int P = L::P, PW = L::PW, LEN_TOMB = L::LEN_TOMB;
    static constexpr int NPB = (P + 63) / 64;  // blocks holding prefix words
    static_assert(P % 4 == 0 && L::KEY_ROW % 4 == 0, "prefix words are whole message words");
    static_assert(NPB <= 2 && PW - 16 <= 2, "past block 0 the prefix is the value's length alone");
    static_assert(RK == REC_PLAIN || LEN_TOMB <= 64, "a tombstone is one block");

    VarCols c;            // keys, stamps, tags, voffs and dst rebased to row `base`; values the whole heap
    uint64_t base;
    uint32_t t = 0;       // the record's row, from base
    bool tomb = false;    // State::Tombstone: the message ends with the variant word
    uint64_t vstart = 0;  // the value's span in the heap, clipped to it (0 bytes for a tombstone)
    uint64_t vlen = 0;

    __device__ __forceinline__ VarReader(const VarCols &cols, uint64_t first) : c(cols), base(first) {
        c.keys = cols.keys + first * L::KEY_ROW;
        c.phys = cols.phys + first;
        c.logical = cols.logical + first;
        c.node = cols.node + first;
        c.tags = cols.tags + first;
        c.voffs = cols.voffs + first;
        if (cols.dst) c.dst = cols.dst + first;
    }

    // take row `row` of the range; returns its message length
    template <bool TAGS>
    __device__ __forceinline__ uint64_t take(uint32_t row) {
        t = row;
        tomb = (TAGS && RK != REC_PLAIN) ? c.tags[row] != 0 : false;
        const uint2 *o = reinterpret_cast<const uint2 *>(c.voffs) + row;  // offsets[row], offsets[row + 1]
        const uint2 a2 = o[0], b2 = o[1];
        uint64_t a = ((uint64_t)a2.y << 32) | a2.x, b = ((uint64_t)b2.y << 32) | b2.x;
        // clipped to the heap: offsets that decrease or run past it give a wrong fingerprint, never
        // an out-of-range read or a loop over a wrapped-around length (record_span's rule)
        if (a > c.vlimit) a = c.vlimit;
        if (b > c.vlimit) b = c.vlimit;
        vstart = a;
        vlen = (b > a && !tomb) ? b - a : 0;  // a tombstone's span is ignored, whatever its length
        return tomb ? (uint64_t)LEN_TOMB : (uint64_t)P + vlen;
    }

    // the key and stamp words (block 0's loads, issued before the value's so both are in flight)
    struct Head {
        uint32_t kw[L::KEY_ENC / 4 > 0 ? L::KEY_ENC / 4 : 1];
        uint32_t sw[5];
    };
    __device__ __forceinline__ void load_head(Head &h) const {
        load_key<KK, KL, uint32_t>(c.keys, t, h.kw);
        if constexpr (RK == REC_DATED) load_stamp<uint32_t>(c, t, h.sw);
    }

    // the prefix words of block B (B < NPB) over the value words `v` that follow them
    template <int B>
    __device__ __forceinline__ void prefix_block(const Head &h, const uint32_t v[16], uint32_t m[16]) const {
        constexpr int G0 = 16 * B;                        // the block's first message word
        constexpr int NPW = PW - G0 < 16 ? PW - G0 : 16;  // prefix words in it
        uint32_t pw[PW];
        if constexpr (B == 0) {
            build_prefix<L, KK, RK>(h.kw, h.sw, false, pw);  // variant 0, length 0
            if constexpr (RK != REC_PLAIN) pw[PW - 3] = tomb ? 1u : 0u;
        }
        pw[PW - 2] = (uint32_t)vlen;  // 0 for a tombstone: past its last byte
        pw[PW - 1] = (uint32_t)(vlen >> 32);
#pragma unroll
        for (int j = 0; j < 16; j++) m[j] = j < NPW ? pw[G0 + j] : v[j - NPW];
    }

    // Every block takes its value bytes through one load_block -- from the value's start behind
    // the prefix words, from (boff - P) past them -- so lanes of a wave at different blocks share
    // the loads and the funnel shift, and only the prefix words' loads are a branch of their own.
    __device__ __forceinline__ void block(uint64_t boff, uint32_t blen, uint32_t m[16]) const {
        const bool b0 = boff == 0, b1 = NPB == 2 && boff == 64;
        const uint32_t pbytes = b0 ? (uint32_t)(P < 64 ? P : 64) : b1 ? (uint32_t)(P - 64) : 0u;  // prefix bytes here
        const uint64_t voff = (b0 || b1) ? 0ull : boff - (uint64_t)P;
        const uint32_t vb = blen > pbytes ? blen - pbytes : 0u;
        Head h;
        if (b0) load_head(h);
        uint32_t v[16];
        if (vb) {
            // (a full block behind prefix words uses only its vb value bytes: no mask needed)
            load_block(c.values, vstart + voff, vb, c.vlimit, v, blen < 64);
        } else {  // an empty value or a tombstone: nothing is read
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = 0u;
        }
        if (b0) {
            prefix_block<0>(h, v, m);
        } else if (b1) {
            prefix_block<NPB - 1>(h, v, m);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) m[j] = v[j];
        }
    }

    // the record's fingerprint to its row: the row itself, or the batch path's sorted slot (DevCols::dst)
    __device__ __forceinline__ void store(uint64_t n, uint8_t *fps, const uint32_t h[8]) const {
        if (c.dst) {
            const uint32_t r = c.dst2 ? c.dst2[c.dst[t]] : c.dst[t];
            if (r < n) store_fp<uint64_t>(fps, r, h);  // bounded, as in k_lift
        } else {
            store_fp<uint32_t>(fps + base * 32, t, h);
        }
    }
};

// one-chunk messages: the lane-refill loop.  bsums (in-order path only, no DevCols::dst): the
// wave's 256 records are one 256-row block, summed at the end from the fingerprints just written
template <int KK, int KL, int RK, bool TAGS>
__global__ __launch_bounds__(256) void k_lift_var_short(VarCols c, uint64_t n, uint8_t *fps, uint8_t *bsums) {
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint64_t w0 = wave * VAR_PER_WAVE;
    if (w0 >= n) return;  // uniform per wave
    const uint32_t rows = (uint32_t)(n - w0 < (uint64_t)VAR_PER_WAVE ? n - w0 : (uint64_t)VAR_PER_WAVE);
    uint32_t next = 0;  // first unclaimed row of the wave's range (same in every lane)
    VarReader<KK, KL, RK> rd(c, w0);
    uint64_t len = 0;
    uint32_t b = 0, nb = 0, cv[8];
    bool active = false;
    for (;;) {
        // lanes without a record claim the next ones, in order; a multi-chunk message is skipped
        // (k_lift_var_long hashes it) and the lane claims again
        bool need = !active;
        for (;;) {
            const uint64_t mask = __ballot(need && next < rows);
            if (!mask) break;
            const uint32_t cand = next + lanes_below(mask);
            next += (uint32_t)__popcll(mask);
            if (need && cand < rows) {
                VarReader<KK, KL, RK> cnd = rd;
                const uint64_t l0 = cnd.template take<TAGS>(cand);
                if (l0 <= (uint64_t)CHUNK_LEN) {
                    rd.t = cnd.t, rd.tomb = cnd.tomb, rd.vstart = cnd.vstart, rd.vlen = cnd.vlen;
                    len = l0;
                    b = 0;
                    nb = (uint32_t)((l0 + 63) / 64);  // l0 >= 8: at least the value's length, or a variant word
                    cv_iv(cv);
                    active = true;
                    need = false;
                }
            } else {
                need = false;
            }
        }
        if (!__ballot(active)) break;
        if (active) {
            const uint32_t boff = 64u * b;
            const uint32_t blen = (uint32_t)len - boff < 64u ? (uint32_t)len - boff : 64u;
            uint32_t m[16];
            rd.block(boff, blen, m);
            const uint32_t flags = (b == 0 ? CHUNK_START : 0u) | (b + 1 == nb ? (CHUNK_END | ROOT) : 0u);
            compress(cv, m, 0u, 0u, blen, flags);
            if (++b == nb) {
                rd.store(n, fps, cv);
                active = false;
            }
        }
    }
    if (bsums) wave_block_sums<VAR_PER_WAVE>(fps, w0, n, bsums);
}

// messages longer than one chunk: one per lane (shorter ones return at once)
template <int KK, int KL, int RK, bool TAGS>
__global__ __launch_bounds__(256) void k_lift_var_long(VarCols c, uint64_t n, uint8_t *fps) {
    const uint64_t b0 = (uint64_t)blockIdx.x * 256;
    if (b0 + threadIdx.x >= n) return;
    VarReader<KK, KL, RK> rd(c, b0);
    const uint64_t len = rd.template take<TAGS>(threadIdx.x);
    if (len <= (uint64_t)CHUNK_LEN) return;
    uint32_t cv[8];
    hash_message(rd, len, cv);
    rd.store(n, fps, cv);
}

}  // namespace rh
