// lift_strfix.hpp -- the lift of records whose key is a short string held in a fixed-width row
// (RH_KEY_STR, lift_str.hpp) and whose value is fixed-width: (), u32 or u64 -- FingerprintTreeMap<String, u32>,
// ReplicatedSet<String>, String -> u64 counters.
//
// The message of a present record:
//   u64 L | L key bytes | DATED: phys u64, logical u32, node u64 | DATED/PROJECTION: u32 variant |
//   value 0 / 4 / 8 bytes
// and a tombstone's ends after the variant word.  At most 8 + 63 + 24 + 8 = 103 bytes: one or two
// blocks, always one chunk.  So there is no heap, no offsets column, no multi-chunk kernel and no
// refill over long values: one kernel.
//
// The composition is StrReader's (lift_str.hpp), used as it stands.  Its stream behind the key is
// the tail words, the u64 length of the value, and the value's bytes; here the value's *words* take
// the place of that u64 (a u32 leaves its high word zero, () both, and so does a tombstone, whose
// value row is not looked at), and no value bytes follow: the words behind are compile-time zeros,
// so their selects and shifts fold away, and the W = 64 column in LDS holds the tail words alone
// (compose64<0>).  The message is then 8 - 4 VW bytes shorter than the stream: what lies past its
// end is zero, as a block's padding has to be.
//
// Blocks: 8 + (W - 1) + 4 NS bytes at most, NS the stamp, variant and value words.  W = 16: 55,
// one block, and no second-block code in any instantiation (ONE_BLOCK).  W = 32: one block but for
// DATED u32 (L >= 29) and DATED u64 (L >= 25).  W = 64: two blocks from L = 57 - 4 NS, for every
// shape.  Where two blocks can occur the lanes of a wave differ in block count and the kernel runs
// a lane-refill loop (a lane that has finished claims the wave's next record); where they cannot,
// each lane takes the wave's rows in turn.
//
// A length byte above W - 1 is clipped and row bytes at and past L are masked (StrReader): a wrong
// fingerprint for a malformed device row, never an access out of range.
//
// Read per record: the W-byte row + stamp + tag + value row; written: 32 B.
#pragma once
#include "lift_str.hpp"

namespace rh {

template <int W, int VK, int RK>
struct StrFixReader {
    static_assert(VK == VAL_UNIT || VK == VAL_U32 || VK == VAL_U64, "a fixed-width value: (), u32 or u64");
    using S = StrReader<W, RK>;
    static constexpr int VW = VK == VAL_U32 ? 1 : VK == VAL_U64 ? 2 : 0;  // value words
    static constexpr int NS = S::TLW - 2 + VW;                            // stamp, variant, value
    static constexpr int LMAX = 8 + (W - 1) + 4 * NS;                     // the longest message
    static constexpr bool ONE_BLOCK = LMAX <= 64;
    static_assert(LMAX <= 128, "at most two blocks");

    S s;                    // the row, L, the tombstone flag; S::vlen holds the value's words
    const uint8_t *values;  // the value column, rebased as s.c's columns are

    static __device__ __forceinline__ VarCols as_var(const DevCols &cols) {
        VarCols v;
        static_cast<DevCols &>(v) = cols;
        return v;  // no heap, no offsets: StrReader::take and ::block are not used
    }
    __device__ __forceinline__ StrFixReader(const DevCols &cols, uint64_t first)
        : s(as_var(cols), first), values(cols.values + first * (uint64_t)(4 * VW)) {}

    // take row `row` of the range; returns its message length
    template <bool TAGS>
    __device__ __forceinline__ uint32_t take(uint32_t row) {
        s.t = row;
        s.tomb = (TAGS && RK != REC_PLAIN) ? s.c.tags[row] != 0 : false;
        const uint32_t lb = s.c.keys[row * (uint32_t)W + (uint32_t)(W - 1)];
        s.klen = lb < (uint32_t)(W - 1) ? lb : (uint32_t)(W - 1);
        uint64_t v = 0;
        if constexpr (VW > 0) {
            uint32_t vw[2] = {0u, 0u};
            ldw<VW, 4 * VW>(values + row * (uint32_t)(4 * VW), vw);  // the row exists whatever the tag says
            v = ((uint64_t)vw[1] << 32) | vw[0];
        }
        s.vlen = s.tomb ? 0 : v;
        return 8u + s.klen + (uint32_t)(4 * (S::TLW - 2)) + (s.tomb ? 0u : (uint32_t)(4 * VW));
    }

    // the 16 words of block 0 (hi = false) or block 1, zero past the message's last byte
    __device__ __forceinline__ void block(bool hi, uint32_t m[16]) const {
        typename S::Head h;
        if constexpr (W == 64) {
            if (hi) s.load_head_hi(h);
            else s.load_head(h);
            s.template compose64<0>(hi, h, nullptr, m);
        } else {
            uint32_t v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = 0u;
            if (ONE_BLOCK || !hi) {
                s.load_head(h);
                s.compose(h, v, m);
            } else if constexpr (!ONE_BLOCK) {
                s.compose_hi(v, m);
            }
        }
    }

    __device__ __forceinline__ void store(uint64_t n, uint8_t *fps, const uint32_t h[8]) const { s.store(n, fps, h); }
};

// A wave lifts STR_PER_WAVE consecutive records.  bsums (in-order path only, no DevCols::dst): they
// are one 256-row block, summed at the end from the fingerprints just written.
template <int W, int VK, int RK, bool TAGS>
__global__ __launch_bounds__(256) void k_lift_strfix(DevCols c, uint64_t n, uint8_t *fps, uint8_t *bsums) {
    using R = StrFixReader<W, VK, RK>;
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint64_t w0 = wave * STR_PER_WAVE;
    if (w0 >= n) return;  // uniform per wave
    const uint32_t rows = (uint32_t)(n - w0 < (uint64_t)STR_PER_WAVE ? n - w0 : (uint64_t)STR_PER_WAVE);
    R rd(c, w0);
    uint32_t cv[8];
    if constexpr (R::ONE_BLOCK) {
        for (uint32_t r = threadIdx.x & 63u; r < rows; r += 64u) {
            const uint32_t len = rd.template take<TAGS>(r);
            uint32_t m[16];
            rd.block(false, m);
            cv_iv(cv);
            compress(cv, m, 0u, 0u, len, CHUNK_START | CHUNK_END | ROOT);
            rd.store(n, fps, cv);
        }
    } else {
        uint32_t next = 0;  // first unclaimed row of the wave's range (same in every lane)
        uint32_t len = 0;
        bool active = false, hi = false;
        for (;;) {
            // lanes without a record claim the next ones, in order
            const uint64_t mask = __ballot(!active && next < rows);
            if (mask) {
                const uint32_t cand = next + lanes_below(mask);
                next += (uint32_t)__popcll(mask);
                if (!active && cand < rows) {
                    len = rd.template take<TAGS>(cand);
                    hi = false;
                    cv_iv(cv);
                    active = true;
                }
            }
            if (!__ballot(active)) break;
            if (active) {
                uint32_t m[16];
                rd.block(hi, m);
                const uint32_t left = hi ? len - 64u : len;
                const bool last = left <= 64u;
                compress(cv, m, 0u, 0u, last ? left : 64u, (hi ? 0u : CHUNK_START) | (last ? (CHUNK_END | ROOT) : 0u));
                if (last) {
                    rd.store(n, fps, cv);
                    active = false;
                } else {
                    hi = true;
                }
            }
        }
    }
    if (bsums) wave_block_sums<STR_PER_WAVE>(fps, w0, n, bsums);
}

// ---- host side: one row width's instantiations (a translation unit each: lift_strfix{16,32,64}.hip) ----
template <int W, int VK, int RK, bool TAGS>
hipError_t launch_strfix(const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums, hipStream_t st) {
    const uint64_t waves = (n + STR_PER_WAVE - 1) / STR_PER_WAVE;
    hipLaunchKernelGGL((k_lift_strfix<W, VK, RK, TAGS>), dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, st, c, n, fps,
                       c.dst ? nullptr : bsums);
    return hipGetLastError();
}

template <int W, int VK>
hipError_t launch_strfix_kind(int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                              hipStream_t st) {
    switch (rk) {
    case REC_PLAIN: return launch_strfix<W, VK, REC_PLAIN, false>(c, n, fps, bsums, st);
    case REC_DATED:
        return tags ? launch_strfix<W, VK, REC_DATED, true>(c, n, fps, bsums, st)
                    : launch_strfix<W, VK, REC_DATED, false>(c, n, fps, bsums, st);
    case REC_PROJECTION:
        return tags ? launch_strfix<W, VK, REC_PROJECTION, true>(c, n, fps, bsums, st)
                    : launch_strfix<W, VK, REC_PROJECTION, false>(c, n, fps, bsums, st);
    default: return hipErrorInvalidValue;
    }
}

template <int W>
hipError_t launch_strfix_width(int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                               hipStream_t st) {
    switch (vk) {
    case VAL_UNIT: return launch_strfix_kind<W, VAL_UNIT>(rk, tags, c, n, fps, bsums, st);
    case VAL_U32: return launch_strfix_kind<W, VAL_U32>(rk, tags, c, n, fps, bsums, st);
    case VAL_U64: return launch_strfix_kind<W, VAL_U64>(rk, tags, c, n, fps, bsums, st);
    default: return hipErrorInvalidValue;
    }
}

// defined in lift_strfix16.hip / 32 / 64
hipError_t launch_lift_strfix_w16(int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                                  hipStream_t st);
hipError_t launch_lift_strfix_w32(int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                                  hipStream_t st);
hipError_t launch_lift_strfix_w64(int vk, int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                                  hipStream_t st);

}  // namespace rh
