// msg_reader.hpp -- BLAKE3 over a message of run-time length whose bytes come from a reader: the
// byte-granular block loaders, and the chunk loop with its CV stack and parent nodes.  One block
// schedule, two byte sources: a span of pre-encoded canonical bytes (aggregate_kernels.hip) and a
// prefix synthesised in registers followed by a value's bytes in a heap (lift_var.hpp).
//
// A reader provides
//   void block(uint64_t boff, uint32_t blen, uint32_t m[16]) const
// the 16 message words of the block at message byte offset boff (a multiple of 64) with blen
// (0..64) valid bytes; bytes past blen are zero.
#pragma once
#include "blake3_device.hpp"
#include "lift_kernels.hpp"
#include "round_device.hpp"

namespace rh {

// 16 message words of the block starting at byte `addr`, `blen` (0..64) valid bytes; bytes
// past blen are zero.  Dwords at or beyond `limit` (buffer size rounded up to 4) are not read.
__device__ __forceinline__ void load_block_bytes(const uint8_t *base, uint64_t addr, uint32_t blen,
                                                 uint64_t limit, uint32_t m[16]) {
    const uint64_t a4 = addr & ~3ull;
    const uint32_t sh = (uint32_t)(addr & 3) * 8u;
    uint32_t d[17];
#pragma unroll
    for (int k = 0; k < 17; k++) {
        const uint64_t at = a4 + 4ull * k;
        d[k] = (at < limit && (uint32_t)(4 * k) < blen + 4) ? *reinterpret_cast<const uint32_t *>(base + at) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
        uint32_t w = __builtin_amdgcn_alignbit(d[j + 1], d[j], sh);
        const int valid = (int)blen - 4 * j;
        const uint32_t mask = valid >= 4 ? 0xFFFFFFFFu : valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u);
        m[j] = w & mask;
    }
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// record i's bytes [start, start + len), clipped to the buffer: offsets that decrease or run
// past `limit` (a caller error) give a wrong fingerprint, never an out-of-bounds read or a loop
// over a wrapped-around length
__device__ __forceinline__ void record_span(const uint64_t *offs, uint64_t i, uint64_t limit, uint64_t &start,
                                            uint64_t &len) {
    uint64_t a = offs[i], b = offs[i + 1];
    if (a > limit) a = limit;
    if (b > limit) b = limit;
    start = a;
    len = b > a ? b - a : 0;
}

// 16 message words of the block at byte `addr` with `blen` valid bytes (bytes past blen are
// zero): 4 x 16-byte + 1 dword loads from the dword-aligned address, then a funnel shift.  Past
// blen: whole words below the boundary word are kept, the boundary word is masked to its valid
// bytes, the rest are zeroed (compares against constants, selects and an AND per word).  A
// uniform skip of the funnel shift for all-aligned waves measured no faster (the branch's
// register copies cost what the 16 shifts did: profiles/r02_s3_encoded_ab.log).
__device__ __forceinline__ void load_block_fast(const uint8_t *base, uint64_t addr, uint32_t blen, bool partial,
                                                uint32_t m[16]) {
    const uint64_t a4 = addr & ~3ull;
    const uint32_t sh = (uint32_t)(addr & 3) * 8u;
    uint32_t d[17];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const u32x4_a4 v = *reinterpret_cast<const u32x4_a4 *>(base + a4 + 16 * q);
        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
    }
    d[16] = *reinterpret_cast<const uint32_t *>(base + a4 + 64);
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = __builtin_amdgcn_alignbit(d[j + 1], d[j], sh);
    if (partial) {
        const uint32_t jb = blen >> 2, bm = (1u << ((blen & 3u) * 8u)) - 1u;
#pragma unroll
        for (int j = 0; j < 16; j++) m[j] = (uint32_t)j < jb ? m[j] : ((uint32_t)j == jb ? (m[j] & bm) : 0u);
    }
}

// the block of `blen` valid bytes at byte `addr` of a buffer readable below `limit`: the wide
// loads where the 68 bytes they touch lie inside the buffer, dword by dword at its end.
// partial = false: the caller uses no word past blen, so the wide path leaves them unmasked
__device__ __forceinline__ void load_block(const uint8_t *bytes, uint64_t addr, uint32_t blen, uint64_t limit,
                                           uint32_t m[16], bool partial) {
    if (addr + 68 <= limit) load_block_fast(bytes, addr, blen, partial, m);
    else load_block_bytes(bytes, addr, blen, limit, m);  // the buffer's last bytes
}
__device__ __forceinline__ void load_block(const uint8_t *bytes, uint64_t addr, uint32_t blen, uint64_t limit,
                                           uint32_t m[16]) {
    load_block(bytes, addr, blen, limit, m, blen < 64);
}

// reader over a span of a byte buffer: message byte k is bytes[start + k]
struct SpanReader {
    const uint8_t *bytes;
    uint64_t start, limit;
    __device__ __forceinline__ void block(uint64_t boff, uint32_t blen, uint32_t m[16]) const {
        load_block(bytes, start + boff, blen, limit, m);
    }
};

constexpr int ENC_STACK = 40;

// BLAKE3 of a reader's message of `len` bytes, any length: chunk CVs on a stack, parent nodes
template <class R>
__device__ __forceinline__ void hash_message(const R &rd, uint64_t len, uint32_t cv[8]) {
    const uint64_t nchunks = len == 0 ? 1 : (len + CHUNK_LEN - 1) / CHUNK_LEN;
    uint32_t stk[ENC_STACK][8];
    int sp = 0;
    for (uint64_t c = 0; c < nchunks; c++) {
        const uint64_t cbeg = c * CHUNK_LEN;
        const uint64_t clen = len - cbeg < (uint64_t)CHUNK_LEN ? len - cbeg : (uint64_t)CHUNK_LEN;
        const uint32_t nb = clen == 0 ? 1u : (uint32_t)((clen + 63) / 64);
        cv_iv(cv);
        for (uint32_t b = 0; b < nb; b++) {
            const uint64_t boff = cbeg + 64ull * b;
            const uint32_t blen = (uint32_t)(len - boff < 64 ? len - boff : 64);
            uint32_t m[16];
            rd.block(boff, blen, m);
            uint32_t flags = (b == 0 ? CHUNK_START : 0u) | (b == nb - 1 ? CHUNK_END : 0u);
            if (nchunks == 1 && b == nb - 1) flags |= ROOT;
            compress(cv, m, (uint32_t)c, (uint32_t)(c >> 32), blen, flags);
        }
        if (c + 1 < nchunks) {
            uint64_t total = c + 1;
            while ((total & 1) == 0) {
                sp--;
                uint32_t p[8];
                parent(p, stk[sp], cv, 0u);
                for (int q = 0; q < 8; q++) cv[q] = p[q];
                total >>= 1;
            }
            for (int q = 0; q < 8; q++) stk[sp][q] = cv[q];
            sp++;
        }
    }
    for (int s2 = sp - 1; s2 >= 0; s2--) {
        uint32_t p[8];
        parent(p, stk[s2], cv, s2 == 0 ? ROOT : 0u);
        for (int q = 0; q < 8; q++) cv[q] = p[q];
    }
}

// BLAKE3 of bytes [start, start + len)
__device__ __forceinline__ void hash_span(const uint8_t *bytes, uint64_t start, uint64_t len, uint64_t limit,
                                          uint32_t cv[8]) {
    hash_message(SpanReader{bytes, start, limit}, len, cv);
}

// The 256-row block sums of a wave's ROWS consecutive records (whole 256-row blocks, from row w0),
// formed at the end of a lane-refill kernel from the fingerprints just written -- its own, and
// those the long-record kernel wrote before this launch: L2-resident reads, not a second pass.
template <int ROWS>
__device__ __forceinline__ void wave_block_sums(const uint8_t *fps, uint64_t w0, uint64_t n, uint8_t *bsums) {
    static_assert(ROWS % 256 == 0, "a wave's records must be whole 256-row blocks");
    __threadfence_block();  // workgroup scope: this wave reads its own stores back (same L2); an agent-scope fence would write back L2
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int blk = 0; blk < ROWS / 256; blk++) {
        const uint64_t r0 = w0 + 256ull * blk;
        if (r0 >= n) break;  // uniform
        Acc a;
        acc_zero(a);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t r = r0 + lane + 64 * k;
            if (r < n) {
                uint32_t f[8];
                load_fp(fps, r, f);
                acc_add_fp(a, f);
            }
        }
        acc_wave_reduce(a);
        if (lane == 0) {
            uint32_t f[8];
            acc_normalise(a, f);
            store_sum(bsums, r0 / 256, f);
        }
    }
}

}  // namespace rh
