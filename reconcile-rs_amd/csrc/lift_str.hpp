// lift_str.hpp -- the lift of records whose key is a short string held in a fixed-width row
// (RH_KEY_STR: String / Vec<u8> / &str of at most W - 1 bytes, W = 16, 32 or 64) and whose value is a
// run of bytes of per-record length (RH_VAL_VARBYTES).  The key row is the string's L bytes, zero
// bytes up to offset W - 2, and L in byte W - 1 (include/rsos_hip.h): to every sort, search and
// merge it is a RH_KEY_BYTES row of width W; only this lift knows that the *string* is hashed --
// u64 L, then L bytes (rsos/src/encoding/serializer.rs:105-113) -- and not the row.
//
// The message of a present record:
//   u64 L | L key bytes | DATED: phys u64, logical u32, node u64 | DATED/PROJECTION: u32 variant |
//   u64 vlen | value bytes
// and a tombstone's ends after the variant word (12..63 bytes, one block, for W <= 32; up to 95
// bytes, two blocks, for W = 64).  The prefix is P = 8 + L + TL bytes (TL = stamp + variant + 8: 8,
// 12 or 32), 16..71 for W <= 32 and up to 103 for W = 64, in general no multiple of 4: everything
// behind the key starts at a per-record byte offset.  So the fields behind the
// key -- the TL/4 tail words, and the value words of the block in which the prefix ends -- are one
// stream of words that is moved up by L bytes: (L & 3) bytes with a funnel shift, (L >> 2) words
// with a select per bit of it in registers (W <= 32) or through LDS (W = 64, below), every
// register index a compile-time constant.  The
// value's bytes of that block are loaded from the value's start (never from an address below it)
// and take part in the same shift; every later block is value bytes alone, from
// vstart + boff - P >= vstart.
//
// W = 64: the key itself can end in block 1 (8 + L > 64 from L = 57), and the tail words and the
// first value words can lie on either side of the block edge.  Both prefix blocks are windows of
// the same stream: message word K is stream word K - 2 - (L >> 2), moved up by (L & 3) bytes.
// Here the word offset is taken through LDS (compose64): each lane writes its stream to a column
// of its own and reads 17 words back from a run-time slot -- select passes for 16 word offsets
// over two blocks measured x1.30-1.34 of the encoded route, this form x1.21-1.26 (DESIGN.md
// section 6).  Still no scratch and no register indexed at run time.
//
// Read per record: the W-byte row + stamp + tag + one 8 B offset + the value bytes; written: 32 B.
//
// Two kernels, lift_var.hpp's split: messages of one chunk go through the lane-refill loop
// (k_lift_str_short, which also forms the block sums on the in-order path), longer ones take one
// lane each through hash_message (k_lift_str_long).
#pragma once
#include "lift_kernels.hpp"
#include "msg_reader.hpp"

namespace rh {

enum { KEY_STR = 4 };

constexpr int STR_PER_WAVE = 64 * 4;

template <int W, int RK>
struct StrReader {
    static_assert(W == 16 || W == 32 || W == 64, "a key row is 16, 32 or 64 bytes");
    static constexpr int STAMP = RK == REC_DATED ? 20 : 0, TAG = RK == REC_PLAIN ? 0 : 4;
    static constexpr int TL = STAMP + TAG + 8, TLW = TL / 4;  // the fields behind the key, up to the value's length
    static constexpr int KW = W / 4;                          // words of a key row
    static constexpr int PMAX = 8 + (W - 1) + TL;             // the longest prefix
    static constexpr int QBITS = W == 32 ? 3 : 2;             // L >> 2 is below 1 << QBITS
    static_assert(W == 64 ? PMAX <= 103 : PMAX <= 71, "the prefix ends in block 0 or 1");

    VarCols c;            // keys, stamps, tags, voffs and dst rebased to row `base`; values the whole heap
    uint64_t base;
    uint32_t t = 0;       // the record's row, from base
    uint32_t klen = 0;    // L: the row's length byte, clipped to W - 1
    bool tomb = false;    // State::Tombstone: the message ends with the variant word
    uint64_t vstart = 0;  // the value's span in the heap, clipped to it (0 bytes for a tombstone)
    uint64_t vlen = 0;

    __device__ __forceinline__ StrReader(const VarCols &cols, uint64_t first) : c(cols), base(first) {
        c.keys = cols.keys + first * W;
        c.phys = cols.phys + first;
        c.logical = cols.logical + first;
        c.node = cols.node + first;
        c.tags = cols.tags + first;
        c.voffs = cols.voffs + first;
        if (cols.dst) c.dst = cols.dst + first;
    }

    // the prefix length of a present record with this key
    __device__ __forceinline__ uint32_t plen() const { return 8u + klen + (uint32_t)TL; }

    // take row `row` of the range; returns its message length
    template <bool TAGS>
    __device__ __forceinline__ uint64_t take(uint32_t row) {
        t = row;
        tomb = (TAGS && RK != REC_PLAIN) ? c.tags[row] != 0 : false;
        // a length byte above W - 1 (a caller error in a device column) is clipped: a wrong
        // fingerprint, and a prefix of at most PMAX bytes
        const uint32_t lb = c.keys[row * (uint32_t)W + (uint32_t)(W - 1)];
        klen = lb < (uint32_t)(W - 1) ? lb : (uint32_t)(W - 1);
        const uint2 *o = reinterpret_cast<const uint2 *>(c.voffs) + row;  // offsets[row], offsets[row + 1]
        const uint2 a2 = o[0], b2 = o[1];
        uint64_t a = ((uint64_t)a2.y << 32) | a2.x, b = ((uint64_t)b2.y << 32) | b2.x;
        // clipped to the heap, as VarReader::take does (record_span's rule)
        if (a > c.vlimit) a = c.vlimit;
        if (b > c.vlimit) b = c.vlimit;
        vstart = a;
        vlen = (b > a && !tomb) ? b - a : 0;  // a tombstone's span is ignored, whatever its length
        return tomb ? (uint64_t)(plen() - 8u) : (uint64_t)plen() + vlen;
    }

    // the key row and the stamp words (issued before the value's loads so both are in flight)
    struct Head {
        uint32_t kw[KW];
        uint32_t sw[5];
    };
    __device__ __forceinline__ void load_head(Head &h) const {
        ldw<KW, 16>(c.keys + t * (uint32_t)W, h.kw);  // the whole row, W-byte aligned
        if constexpr (RK == REC_DATED) load_stamp<uint32_t>(c, t, h.sw);
    }
    // W = 64, block 1: the row's last two words (the key bytes from offset 56) and the stamp
    __device__ __forceinline__ void load_head_hi(Head &h) const {
        static_assert(W == 64, "only a 64-byte row reaches block 1");
        ldw<2, 8>(c.keys + t * (uint32_t)W + 56u, h.kw + 14);
        if constexpr (RK == REC_DATED) load_stamp<uint32_t>(c, t, h.sw);
    }

    // The fields behind the key as words: stamp, State variant, the value's u64 length
    __device__ __forceinline__ void tail_words(const Head &h, uint32_t tw[TLW]) const {
        int o = 0;
        if constexpr (RK == REC_DATED) {
#pragma unroll
            for (int j = 0; j < 5; j++) tw[o++] = h.sw[j];
        }
        if constexpr (RK != REC_PLAIN) tw[o++] = tomb ? 1u : 0u;  // State variant index
        tw[o++] = (uint32_t)vlen;  // 0 for a tombstone: past its last byte
        tw[o++] = (uint32_t)(vlen >> 32);
    }

    // word `hi` moved up by (L & 3) bytes, its low bytes filled from the word before it:
    // (hi:lo) >> (32 - s8), which alignbit cannot express at s8 == 0 (a shift by 32)
    static __device__ __forceinline__ uint32_t up_bytes(uint32_t hi, uint32_t lo, uint32_t s8) {
        return s8 ? __builtin_amdgcn_alignbit(hi, lo, 32u - s8) : hi;
    }

    // Block 0 of a record whose first value words are v: u64 L and the key bytes below L in
    // place; behind them the stream of tail words and value words, moved up by L bytes -- (L & 3)
    // bytes by a funnel shift, (L >> 2) words by one select pass per bit of it.  Bytes of the row
    // at and past L (padding, the length byte) are masked to zero before they enter the message.
    __device__ __forceinline__ void compose(const Head &h, const uint32_t v[16], uint32_t m[16]) const {
        static_assert(W != 64, "a 64-byte row's prefix blocks: compose64");
        constexpr int NST = 14;  // stream words that can reach block 0: its word 0 is message word 2 at least
        uint32_t st[NST];
        uint32_t tw[TLW];
        tail_words(h, tw);
#pragma unroll
        for (int i = 0; i < NST; i++) st[i] = i < TLW ? tw[i] : v[i - TLW];
        const uint32_t s8 = (klen & 3u) * 8u, q = klen >> 2;
        uint32_t e[16];
        e[0] = klen;
        e[1] = 0u;
#pragma unroll
        for (int i = 0; i < NST; i++) e[2 + i] = up_bytes(st[i], i > 0 ? st[i - 1] : 0u, s8);
        // up by (L >> 2) words: one pass per bit, highest word first so each reads unshifted ones
        // (words 0 and 1 stay: the stream starts at word 2)
#pragma unroll
        for (int bit = 0; bit < QBITS; bit++) {
            const bool on = (q >> bit) & 1u;
#pragma unroll
            for (int k = 15; k >= 2; k--) {
                const int src = k - (1 << bit);
                const uint32_t from = src >= 2 ? e[src >= 2 ? src : 2] : 0u;
                e[k] = on ? from : e[k];
            }
        }
        // the key: words below the boundary whole, the boundary word's bytes below L, nothing past it
        const uint32_t bm = (1u << s8) - 1u;
#pragma unroll
        for (int j = 0; j < KW; j++) e[2 + j] |= (uint32_t)j < q ? h.kw[j] : ((uint32_t)j == q ? (h.kw[j] & bm) : 0u);
#pragma unroll
        for (int j = 0; j < 16; j++) m[j] = e[j];
    }

    // W = 64, both prefix blocks at once, the word shift through LDS.  The lane writes its stream
    // (tail words, 16 value words) to a column of its own -- slot s of lane t at word 256 s + t, so
    // whatever slots a wave's lanes address, each lane stays in its own bank -- and reads back the 17
    // words t[k] = stream[base + k], base = 16 blk - 3 - (L >> 2): a run-time word offset with no
    // select pass and no register indexed at run time.  Indices below 0 (the key's place, and
    // words 0 and 1 of block 0) read slot 0, which holds zero.  The highest index is 13 in block 0
    // and 29 - (L >> 2) in block 1, where P > 64 means L >= 57 - TL: at most TLW + 15, the last
    // stream word (dated 23, projection 18, plain 17); it is clamped all the same.  A lane reads only what
    // it wrote itself, in program order: no barrier.  Then the byte shift and the key mask as in
    // compose: message word 2 + j holds key word j, so block 0 takes words 0..13 and block 1 words
    // 14 and 15 (word 15's last byte, the length, is always at or past L).  A tombstone's stream is
    // zero behind its variant word, so its blocks are zero past its last byte.  A wave whose lanes
    // are at block 0 and at block 1 runs this once.
    // NV: the value words behind the tail (16 here; lift_strfix.hpp's stream ends with the tail words,
    // NV = 0, and whatever a block holds past them is read from slot 0 as zero).
    template <int NV = 16>
    __device__ __forceinline__ void compose64(bool hi, const Head &h, const uint32_t *v, uint32_t m[16]) const {
        static_assert(W == 64, "the LDS composition is the 64-byte row's");
        constexpr int NSTR = TLW + NV;
        __shared__ uint32_t lds[(NSTR + 1) * 256];  // (both kernels launch 256 lanes a workgroup)
        uint32_t *col = lds + threadIdx.x;
        uint32_t tw[TLW];
        tail_words(h, tw);
        col[0] = 0u;
#pragma unroll
        for (int i = 0; i < TLW; i++) col[(1 + i) * 256] = tw[i];
#pragma unroll
        for (int i = 0; i < NV; i++) col[(1 + TLW + i) * 256] = v[i];
        const uint32_t s8 = (klen & 3u) * 8u, q = klen >> 2;
        const int base = (hi ? 13 : -3) - (int)q;
        uint32_t t[17];
#pragma unroll
        for (int k = 0; k < 17; k++) {
            int i = base + k;
            i = i < -1 ? -1 : i;
            i = i > NSTR - 1 ? (NV < 16 ? -1 : NSTR - 1) : i;
            t[k] = col[(i + 1) * 256];
        }
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = up_bytes(t[k + 1], t[k], s8);
        const uint32_t bm = (1u << s8) - 1u;
        if (hi) {
#pragma unroll
            for (int j = 14; j < 16; j++) m[j - 14] |= (uint32_t)j < q ? h.kw[j] : ((uint32_t)j == q ? (h.kw[j] & bm) : 0u);
        } else {
            m[0] = klen;
#pragma unroll
            for (int j = 0; j < 14; j++) m[2 + j] |= (uint32_t)j < q ? h.kw[j] : ((uint32_t)j == q ? (h.kw[j] & bm) : 0u);
        }
    }

    // Block 1 of a record whose prefix ends there (P = 65..71: W = 32, DATED, L = 25..31): the last
    // bytes of the value's length, then the value from its start.  Message word 16 + k is stream
    // word 14 + k - (L >> 2), and L >> 2 is 6 or 7 here: one select, then the byte shift.
    __device__ __forceinline__ void compose_hi(const uint32_t v[16], uint32_t m[16]) const {
        static_assert(W != 64, "a 64-byte row's prefix blocks: compose64");
        static_assert(PMAX <= 64 || TLW == 8, "block 1 holds prefix bytes for W = 32 DATED alone");
        const uint32_t s8 = (klen & 3u) * 8u;
        const bool q7 = (klen >> 2) == 7u;
        // stream words 6 .. 23: the value's length, the 16 value words
        uint32_t st[18];
        st[0] = (uint32_t)vlen;
        st[1] = (uint32_t)(vlen >> 32);
#pragma unroll
        for (int j = 0; j < 16; j++) st[2 + j] = v[j];
        uint32_t t[17];  // stream words 14 + k - (L >> 2), k = -1 .. 15
#pragma unroll
        for (int k = 0; k < 17; k++) t[k] = q7 ? st[k] : st[k + 1];
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = up_bytes(t[k + 1], t[k], s8);
    }

    // msg_reader.hpp's contract: the 16 words of the block at message byte boff, blen valid bytes,
    // zero past them.  Every block takes its value bytes through one load_block, as in VarReader,
    // so lanes of a wave at different blocks share the loads and the funnel shift.  The blocks that
    // hold prefix bytes (block 0; block 1 when P > 64) load the value from its start and shift it
    // in registers -- the address vstart + boff - P would lie below the heap for a value that
    // starts within P bytes of it; every later block is value bytes alone, from boff - P >= 0.
    __device__ __forceinline__ void block(uint64_t boff, uint32_t blen, uint32_t m[16]) const {
        const uint32_t p = plen();
        const bool b0 = boff == 0, b1 = PMAX > 64 && boff == 64 && p > 64u;
        const uint32_t pbytes = b0 ? (p < 64u ? p : 64u) : b1 ? p - 64u : 0u;  // prefix bytes here
        const uint64_t voff = (b0 || b1) ? 0ull : boff - (uint64_t)p;
        const uint32_t vb = blen > pbytes ? blen - pbytes : 0u;  // (a tombstone: blen = p - 8, none)
        Head h;
        if (b0) load_head(h);
        if constexpr (W == 64) {
            if (b1) load_head_hi(h);
        }
        uint32_t v[16];
        if (vb) {
            // partial: zero past the vb value bytes, so a composed block is zero past blen; a full
            // block's words past vb land at or past word 16 of this block and are dropped
            load_block(c.values, vstart + voff, vb, c.vlimit, v, blen < 64);
        } else {  // an empty value, a tombstone, or a block 0 that is all prefix: nothing is read
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = 0u;
        }
        if constexpr (W == 64) {
            if (b0 || b1) {
                compose64(b1, h, v, m);
            } else {
#pragma unroll
                for (int j = 0; j < 16; j++) m[j] = v[j];
            }
        } else {
            if (b0) {
                compose(h, v, m);
            } else if (b1) {
                if constexpr (PMAX > 64) compose_hi(v, m);
            } else {
#pragma unroll
                for (int j = 0; j < 16; j++) m[j] = v[j];
            }
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

// one-chunk messages: k_lift_var_short's lane-refill loop over a StrReader.  bsums (in-order path
// only, no DevCols::dst): the wave's 256 records are one 256-row block, summed at the end from the
// fingerprints just written
template <int W, int RK, bool TAGS>
__global__ __launch_bounds__(256) void k_lift_str_short(VarCols c, uint64_t n, uint8_t *fps, uint8_t *bsums) {
    const uint64_t wave = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint64_t w0 = wave * STR_PER_WAVE;
    if (w0 >= n) return;  // uniform per wave
    const uint32_t rows = (uint32_t)(n - w0 < (uint64_t)STR_PER_WAVE ? n - w0 : (uint64_t)STR_PER_WAVE);
    uint32_t next = 0;  // first unclaimed row of the wave's range (same in every lane)
    StrReader<W, RK> rd(c, w0);
    uint64_t len = 0;
    uint32_t b = 0, nb = 0, cv[8];
    bool active = false;
    for (;;) {
        // lanes without a record claim the next ones, in order; a multi-chunk message is skipped
        // (k_lift_str_long hashes it) and the lane claims again
        bool need = !active;
        for (;;) {
            const uint64_t mask = __ballot(need && next < rows);
            if (!mask) break;
            const uint32_t cand = next + lanes_below(mask);
            next += (uint32_t)__popcll(mask);
            if (need && cand < rows) {
                StrReader<W, RK> cnd = rd;
                const uint64_t l0 = cnd.template take<TAGS>(cand);
                if (l0 <= (uint64_t)CHUNK_LEN) {
                    rd.t = cnd.t, rd.klen = cnd.klen, rd.tomb = cnd.tomb, rd.vstart = cnd.vstart, rd.vlen = cnd.vlen;
                    len = l0;
                    b = 0;
                    nb = (uint32_t)((l0 + 63) / 64);  // l0 >= 12: at least u64 L and a variant word or a length
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
    if (bsums) wave_block_sums<STR_PER_WAVE>(fps, w0, n, bsums);
}

// messages longer than one chunk: one per lane (shorter ones return at once)
template <int W, int RK, bool TAGS>
__global__ __launch_bounds__(256) void k_lift_str_long(VarCols c, uint64_t n, uint8_t *fps) {
    const uint64_t b0 = (uint64_t)blockIdx.x * 256;
    if (b0 + threadIdx.x >= n) return;
    {
        // Most records are short, and the offsets alone say so: the prefix is at most PMAX bytes
        // and clipping to the heap only shortens a span.  Such a lane leaves before the strided
        // byte load of its key row's length.
        const uint2 *o = reinterpret_cast<const uint2 *>(c.voffs + b0) + threadIdx.x;
        const uint2 a2 = o[0], b2 = o[1];
        const uint64_t a = ((uint64_t)a2.y << 32) | a2.x, b = ((uint64_t)b2.y << 32) | b2.x;
        if (b <= a || b - a + (uint64_t)StrReader<W, RK>::PMAX <= (uint64_t)CHUNK_LEN) return;
    }
    StrReader<W, RK> rd(c, b0);
    const uint64_t len = rd.template take<TAGS>(threadIdx.x);
    if (len <= (uint64_t)CHUNK_LEN) return;
    uint32_t cv[8];
    hash_message(rd, len, cv);
    rd.store(n, fps, cv);
}

}  // namespace rh
