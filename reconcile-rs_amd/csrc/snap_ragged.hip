// snap_ragged.hip -- the byte-granular snapshot locate and decode (snap_ragged.hpp).
//
// An entry's length is in its own bytes (a String key's u64 L, a Vec<u8> value's u64 M), so an
// entry may start at any byte.  next(p), the end of the entry that starts at p, depends only on
// the bytes at p (rag_parse: at most RagFmt::hdr of them, never a value's bytes).  The file is cut
// into segments of S bytes; one wave per segment stages its bytes and hdr more in LDS.
//   guess   every segment takes the first position in it whose header is valid and walks the
//           chain from there to the first entry start at or past its end: first, cnt, exit
//           (segment 0 starts at 16 by definition; a walk that meets an invalid position exits
//           INVALID and remembers where)
//   rounds  every segment s >= 1 compares exit[s - 1] of the round before with its first; if they
//           differ it walks again from there (or, where the chain passes over it, hands the exit
//           on).  A segment whose predecessor exited INVALID stays as it is.  By induction from
//           segment 0 the first wrong segment moves up by at least one per round, so a round that
//           changes nothing comes after at most `segments` rounds and leaves every segment up to
//           the first INVALID exit on the true chain.
//   scan    of cnt: the index of every segment's first entry; the chain holds
//           base[fi] + cnt[fi] entries, fi the first segment with an INVALID exit.
// Then every segment lists its entries from its first position and one lane per entry writes the
// columns; value bytes are copied from the file by a wave per 64 entries, 64 bytes a step.
#include "snap_ragged.hpp"

#include <cstdlib>

namespace rh {

namespace {

constexpr uint64_t RAG_INVALID = ~0ull, RAG_NONE = ~0ull - 1;

struct RagHdr {
    uint64_t end = 0, vpos = 0, vlen = 0, blen = 0;
    uint32_t koff = 0, klen = 0, tag = 0, why = RAG_OK;
};

// Unaligned reads of the staged bytes: the two aligned words around the position, shifted (the
// stage is 16-byte aligned and has RAG_STAGE_SLACK bytes behind it, so the second word is in LDS)
struct LdsRd {
    const uint8_t *b;
    uint64_t org;
    __device__ uint32_t u8(uint64_t p) const { return b[p - org]; }
    __device__ uint32_t u32(uint64_t p) const {
        const uint32_t off = (uint32_t)(p - org);
        const uint32_t *w = reinterpret_cast<const uint32_t *>(b) + (off >> 2);
        return (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> ((off & 3) * 8));
    }
};
struct GlobRd {
    const uint8_t *b;
    __device__ uint32_t u8(uint64_t p) const { return b[p]; }
    __device__ uint32_t u32(uint64_t p) const { return u8(p) | (u8(p + 1) << 8) | (u8(p + 2) << 16) | (u8(p + 3) << 24); }
};
template <class Rd>
__device__ inline uint32_t rd_u32(const Rd &r, uint64_t p) {
    return r.u32(p);
}
template <class Rd>
__device__ inline uint64_t rd_u64(const Rd &r, uint64_t p) {
    return (uint64_t)r.u32(p) | ((uint64_t)r.u32(p + 4) << 32);
}

// The entry that starts at p: every read is checked against the file's length first, and lies
// below p + f.hdr.  A position is invalid (why != RAG_OK) if a length or the variant fails its
// check or the entry would end past the file.
template <class Rd>
__device__ inline RagHdr rag_parse(const RagFmt &f, const Rd &rd, uint64_t p) {
    RagHdr h;
    const uint64_t len = f.len;
    if (p > len) {
        h.why = RAG_EOF;
        return h;
    }
    uint64_t q = p;
    uint32_t kl = f.key_len;
    if (f.key_mode != RagFmt::KEY_RAW) {
        if (len - q < 8) {
            h.why = RAG_EOF;
            return h;
        }
        const uint64_t L = rd_u64(rd, q);
        q += 8;
        if (f.key_mode == RagFmt::KEY_VEC ? L != f.key_len : L >= f.key_len) {
            h.why = RAG_KEY_LEN;
            h.blen = L;
            return h;
        }
        kl = (uint32_t)L;
    }
    h.koff = (uint32_t)(q - p);
    h.klen = kl;
    if (len - q < (uint64_t)kl + 24) {
        h.why = RAG_EOF;
        return h;
    }
    q += kl;
    h.tag = rd_u32(rd, q + 20);
    if (h.tag > 1) {
        h.why = RAG_VARIANT;
        return h;
    }
    q += 24;
    if (h.tag == 0) {
        uint64_t M = f.val_len;
        if (f.val_mode != RagFmt::VAL_RAW) {
            if (len - q < 8) {
                h.why = RAG_EOF;
                return h;
            }
            M = rd_u64(rd, q);
            q += 8;
            if (f.val_mode == RagFmt::VAL_VEC && M != f.val_len) {
                h.why = RAG_VAL_LEN;
                h.blen = M;
                return h;
            }
        }
        if (M > len - q) {
            h.why = RAG_EOF;
            h.blen = M;
            return h;
        }
        h.vlen = M;
    }
    h.vpos = q;
    h.end = q + h.vlen;
    return h;
}

constexpr uint32_t RAG_STAGE_SLACK = 16;
__host__ __device__ inline uint32_t rag_stage_bytes(const RagFmt &f) {
    return ((f.seg + f.hdr + 15u) & ~15u) + RAG_STAGE_SLACK;
}
__host__ __device__ inline uint32_t rag_list_cap(const RagFmt &f) { return f.seg / f.min_entry + 2; }

// bytes [segbase, min(segbase + S + hdr, len)) of the file into LDS (blob 16-byte aligned, S a
// multiple of 16); nothing at or past len is read
__device__ inline void rag_stage(const RagFmt &f, const uint8_t *blob, uint64_t segbase, uint8_t *lds) {
    const uint64_t want = (uint64_t)f.seg + f.hdr, left = f.len - segbase;
    const uint32_t bytes = (uint32_t)(want < left ? want : left);
    const uint32_t nq = bytes / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(blob + segbase);
    uint4 *dst = reinterpret_cast<uint4 *>(lds);
    for (uint32_t i = threadIdx.x; i < nq; i += 64) dst[i] = src[i];
    for (uint32_t i = nq * 16 + threadIdx.x; i < bytes; i += 64) lds[i] = blob[segbase + i];
    __syncthreads();
}

// lane 0: the chain from `start` (in this segment) to the first entry start at or past the
// segment's end
__device__ inline void rag_walk(const RagFmt &f, const LdsRd &rd, uint64_t start, uint64_t segend, uint64_t *ex,
                                uint64_t *cnt, uint64_t *bad) {
    uint64_t p = start, c = 0, b = 0, e;
    for (;;) {
        if (p >= segend) {
            e = p;
            break;
        }
        const RagHdr h = rag_parse(f, rd, p);
        if (h.why != RAG_OK) {
            e = RAG_INVALID;
            b = p;
            break;
        }
        c++;
        p = h.end;  // > p: an entry holds at least its 24 fixed bytes
    }
    *ex = e;
    *cnt = c;
    *bad = b;
}

// guess != 0: the first launch.  Otherwise one fix-up round: exit_prev is read, exit_new written
// (every segment), first / cnt / bad are each segment's own.
__global__ __launch_bounds__(64) void k_rag_walk(RagFmt f, const uint8_t *blob, uint64_t nseg, int guess,
                                                 const uint64_t *exit_prev, uint64_t *exit_new, uint64_t *first,
                                                 uint64_t *cnt, uint64_t *bad, unsigned long long *changed) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint64_t s = blockIdx.x;
    if (s >= nseg) return;
    const uint64_t segbase = s * f.seg, segend = segbase + f.seg;
    const uint32_t lane = threadIdx.x;
    uint64_t start = 16;
    if (!guess) {
        if (s == 0) {
            if (lane == 0) exit_new[0] = exit_prev[0];
            return;
        }
        const uint64_t want = exit_prev[s - 1];
        if (want == RAG_INVALID || want == first[s]) {
            if (lane == 0) exit_new[s] = exit_prev[s];
            return;
        }
        if (lane == 0) atomicAdd(changed, 1ull);
        if (want >= segend) {  // the chain passes over this segment
            if (lane == 0) first[s] = want, cnt[s] = 0, bad[s] = 0, exit_new[s] = want;
            return;
        }
        start = want;
    }
    rag_stage(f, blob, segbase, lds);
    const LdsRd rd{lds, segbase};
    if (guess && s > 0) {
        const uint64_t lim = segend < f.len ? segend : f.len;
        start = RAG_NONE;
        for (uint64_t p0 = segbase; p0 < lim; p0 += 64) {
            const uint64_t p = p0 + lane;
            const bool ok = p < lim && rag_parse(f, rd, p).why == RAG_OK;
            const unsigned long long m = __ballot(ok);
            if (m) {
                start = p0 + (uint64_t)(__ffsll((long long)m) - 1);
                break;
            }
        }
        if (start == RAG_NONE) {
            if (lane == 0) first[s] = RAG_NONE, cnt[s] = 0, bad[s] = segbase, exit_new[s] = RAG_INVALID;
            return;
        }
    }
    if (lane == 0) {
        uint64_t e, c, b;
        rag_walk(f, rd, start, segend, &e, &c, &b);
        first[s] = start;
        cnt[s] = c;
        bad[s] = b;
        exit_new[s] = e;
    }
}

__global__ void k_rag_first_invalid(uint64_t nseg, const uint64_t *exitv, unsigned long long *words) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg && exitv[s] == RAG_INVALID) atomicMin(&words[RAGW_FI], (unsigned long long)s);
}

// one thread: how many entries the chain holds, where and why it ends, the segment of entry n - 1
__global__ void k_rag_verdict(RagFmt f, const uint8_t *blob, uint64_t nseg, uint64_t n, const uint64_t *cnt,
                              const uint64_t *basev, const uint64_t *bad, unsigned long long *words) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t fi = words[RAGW_FI];
    uint64_t parsed, bp = f.len, why = RAG_EOF, bl = 0;
    if (fi >= nseg) {  // the chain ends exactly at the end of the last segment
        fi = nseg - 1;
        parsed = basev[fi] + cnt[fi];
    } else {
        parsed = basev[fi] + cnt[fi];
        bp = bad[fi];
        const RagHdr h = rag_parse(f, GlobRd{blob}, bp);
        why = h.why;
        bl = h.blen;
    }
    uint64_t lo = 0, hi = fi;  // the last segment whose first entry has an index below n
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) / 2;
        if (basev[mid] < n) lo = mid;
        else hi = mid - 1;
    }
    words[RAGW_LAST] = lo;
    words[RAGW_PARSED] = parsed;
    words[RAGW_BAD] = bp;
    words[RAGW_WHY] = why;
    words[RAGW_BADLEN] = bl;
}

struct RagOutDev {
    uint8_t *keys;
    uint64_t *phys;
    uint32_t *logical;
    uint64_t *node;
    uint8_t *tags;
    uint8_t *values;
    uint64_t *vlen, *vsrc;
};

// values of at most this many bytes are written by the listing kernel itself
constexpr uint32_t RAG_INLINE_VAL = 16;

__global__ __launch_bounds__(64) void k_rag_list(RagFmt f, const uint8_t *blob, uint64_t n, const uint64_t *first,
                                                 const uint64_t *cnt, const uint64_t *basev, RagOutDev o,
                                                 uint64_t *tomb, unsigned long long *words) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint64_t s = blockIdx.x;
    const uint64_t b = basev[s];
    uint64_t c = cnt[s];
    if (!c || b >= n) {
        if (threadIdx.x == 0) tomb[s] = 0;
        return;
    }
    if (c > n - b) c = n - b;
    const uint32_t cap = rag_list_cap(f);
    if (c > cap) c = cap;  // (a segment holds at most seg / min_entry + 1 entry starts)
    const uint64_t segbase = s * f.seg;
    const uint32_t lane = threadIdx.x;
    rag_stage(f, blob, segbase, lds);
    const LdsRd rd{lds, segbase};
    uint32_t *pos = reinterpret_cast<uint32_t *>(lds + rag_stage_bytes(f));
    if (lane == 0) {
        uint64_t p = first[s];
        if (p < segbase || p >= segbase + f.seg) c = 0;  // (a counted entry starts inside its segment)
        for (uint64_t i = 0; i < c; i++) {
            pos[i] = (uint32_t)(p - segbase);
            const RagHdr h = rag_parse(f, rd, p);
            if (h.why != RAG_OK) {  // not reached: the same bytes parsed when they were counted
                c = i;
                break;
            }
            p = h.end;
            if (b + i == n - 1) words[RAGW_END] = p;
        }
        pos[cap] = (uint32_t)c;
    }
    __syncthreads();
    c = pos[cap];
    uint32_t tombs = 0;
    for (uint64_t e = lane; e < c; e += 64) {
        const uint64_t p = segbase + pos[e], idx = b + e;
        const RagHdr h = rag_parse(f, rd, p);
        const uint64_t kp = p + h.koff;
        const uint32_t W = f.key_len;
        if (W) {
            uint8_t *row = o.keys + idx * W;
            const bool str = f.key_mode == RagFmt::KEY_STR;
            // a word at a time: the key's bytes below klen (the words read lie inside the
            // entry's header), zero padding, and a string's length in the row's last byte
            auto kw = [&](uint32_t j) -> uint32_t {
                uint32_t v = 0;
                if (j < h.klen) {
                    v = rd.u32(kp + j);
                    if (h.klen - j < 4) v &= (1u << ((h.klen - j) * 8)) - 1u;
                }
                if (str && j == W - 4) v |= h.klen << 24;
                return v;
            };
            if (W % 16 == 0) {  // (the key column is 16-byte aligned)
                for (uint32_t j = 0; j < W; j += 16)
                    reinterpret_cast<uint4 *>(row)[j / 16] = make_uint4(kw(j), kw(j + 4), kw(j + 8), kw(j + 12));
            } else if (W % 4 == 0) {
                for (uint32_t j = 0; j < W; j += 4) reinterpret_cast<uint32_t *>(row)[j / 4] = kw(j);
            } else {
                for (uint32_t j = 0; j < W; j++)
                    row[j] = (uint8_t)(str && j == W - 1 ? h.klen : j < h.klen ? rd.u8(kp + j) : 0u);
            }
        }
        const uint64_t q = kp + h.klen;
        o.phys[idx] = rd_u64(rd, q);
        o.logical[idx] = rd_u32(rd, q + 8);
        o.node[idx] = rd_u64(rd, q + 12);
        o.tags[idx] = (uint8_t)h.tag;
        tombs += h.tag;
        if (f.val_mode == RagFmt::VAL_VAR) {
            o.vlen[idx] = h.vlen;
            o.vsrc[idx] = h.vpos;
        } else if (f.val_len > RAG_INLINE_VAL) {
            o.vsrc[idx] = h.vpos;
        } else {
            uint8_t *row = o.values + idx * f.val_len;
            for (uint32_t j = 0; j < f.val_len; j++) row[j] = h.tag ? 0 : blob[h.vpos + j];  // vpos + val_len <= len
        }
    }
    for (int d = 32; d; d >>= 1) tombs += __shfl_xor(tombs, d);
    // a count per segment, summed by k_rag_sum: one same-address atomic per wave would queue
    // every segment of the file in the L2's atomic unit
    if (lane == 0) tomb[s] = tombs;
}

// words[RAGW_TOMB] += the segments' tombstone counts, RAG_SUM_TILE segments and one atomic per workgroup
constexpr uint64_t RAG_SUM_TILE = 4096;
__global__ __launch_bounds__(256) void k_rag_sum(const uint64_t *tomb, uint64_t nseg, unsigned long long *words) {
    __shared__ unsigned long long part[256];
    unsigned long long t = 0;
    const uint64_t lo = (uint64_t)blockIdx.x * RAG_SUM_TILE, hi = lo + RAG_SUM_TILE < nseg ? lo + RAG_SUM_TILE : nseg;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) t += tomb[i];
    part[threadIdx.x] = t;
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(&words[RAGW_TOMB], part[0]);
}

// zero the bytes between the values' end and the next multiple of 4 (the heap is handed to the
// lift as whole words)
__global__ void k_rag_pad_heap(const uint64_t *voffs, uint64_t n, uint8_t *heap, uint64_t cap) {
    const uint64_t end = voffs[n];
    const uint64_t p = end + threadIdx.x;
    if (threadIdx.x < 4 && p < ((end + 3) & ~3ull) && p < cap) heap[p] = 0;
}

// A wave per 64 entries: each entry's value in turn, 64 bytes a step.  VAL_VAR: value i to
// heap[voffs[i] .. voffs[i + 1]); fixed rows: to values[i * val_len ..), a tombstone's zeroed.
// A span that would leave the file or the heap is skipped.
__global__ __launch_bounds__(256) void k_rag_copy(RagFmt f, const uint8_t *blob, uint64_t n, const uint8_t *tags,
                                                  const uint64_t *vsrc, const uint64_t *voffs, uint8_t *values,
                                                  uint64_t cap) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    uint64_t src = 0, dst = 0, ln = 0;
    uint32_t zero = 0;
    if (idx < n) {
        zero = tags[idx];
        if (f.val_mode == RagFmt::VAL_VAR) {
            dst = voffs[idx];
            const uint64_t nx = voffs[idx + 1];
            ln = zero || nx < dst ? 0 : nx - dst;
            zero = 0;
        } else {
            dst = idx * f.val_len;
            ln = f.val_len;
        }
        if (dst > cap || ln > cap - dst) ln = 0;
        if (!zero && ln) {
            src = vsrc[idx];
            if (src > f.len || ln > f.len - src) ln = 0;
        }
    }
    for (int k = 0; k < 64; k++) {
        const uint64_t L = ((uint64_t)__shfl((uint32_t)(ln >> 32), k) << 32) | __shfl((uint32_t)ln, k);
        if (!L) continue;
        const uint64_t S = ((uint64_t)__shfl((uint32_t)(src >> 32), k) << 32) | __shfl((uint32_t)src, k);
        const uint64_t D = ((uint64_t)__shfl((uint32_t)(dst >> 32), k) << 32) | __shfl((uint32_t)dst, k);
        const uint32_t Z = __shfl(zero, k);
        if (Z) {
            for (uint64_t i = lane; i < L; i += 64) values[D + i] = 0;
        } else {
            for (uint64_t i = lane; i < L; i += 64) values[D + i] = blob[S + i];
        }
    }
}

}  // namespace

uint32_t ragged_segment_bytes() {
    static const uint32_t seg = [] {
        const char *e = getenv("RSOS_HIP_RAGGED_SEG");
        const long v = e ? atol(e) : 0;
        return v >= 256 && v <= 32768 && v % 16 == 0 ? (uint32_t)v : 8192u;
    }();
    return seg;
}

hipError_t ragged_locate(const RagFmt &f, const uint8_t *blob, uint64_t n, Scratch &s, hipStream_t st, RagTables *t,
                         RagResult *res) {
    hipError_t e;
    const uint64_t nseg = (f.len + f.seg - 1) / f.seg;
    uint64_t *first = static_cast<uint64_t *>(s.get(100, nseg * 8));
    uint64_t *cnt = static_cast<uint64_t *>(s.get(101, nseg * 8));
    uint64_t *bad = static_cast<uint64_t *>(s.get(102, nseg * 8));
    uint64_t *ex[2] = {static_cast<uint64_t *>(s.get(103, nseg * 8)), static_cast<uint64_t *>(s.get(104, nseg * 8))};
    uint64_t *basev = static_cast<uint64_t *>(s.get(105, nseg * 8));
    unsigned long long *words = static_cast<unsigned long long *>(s.get(106, (RAGW_N + 1) * 8));
    if (s.err) return s.err;
    unsigned long long *changed = words + RAGW_N;
    const uint32_t lds = rag_stage_bytes(f);
    if ((e = hipMemsetAsync(words, 0, (RAGW_N + 1) * 8, st))) return e;
    if ((e = hipMemsetAsync(words + RAGW_FI, 0xff, 8, st))) return e;
    hipLaunchKernelGGL(k_rag_walk, dim3((unsigned)nseg), dim3(64), lds, st, f, blob, nseg, 1, ex[1], ex[0], first, cnt, bad,
                       changed);
    if ((e = hipGetLastError())) return e;
    int cur = 0;
    uint64_t rounds = 0, rewalked = 0;
    // the first wrong segment moves up by at least one per round: at most nseg rounds change something
    while (nseg > 1 && rounds < nseg + 1) {
        unsigned long long ch = 0;
        if ((e = hipMemsetAsync(changed, 0, 8, st))) return e;
        hipLaunchKernelGGL(k_rag_walk, dim3((unsigned)nseg), dim3(64), lds, st, f, blob, nseg, 0, ex[cur], ex[1 - cur], first,
                           cnt, bad, changed);
        if ((e = hipGetLastError())) return e;
        if ((e = hipMemcpyAsync(&ch, changed, 8, hipMemcpyDeviceToHost, st))) return e;
        if ((e = hipStreamSynchronize(st))) return e;
        cur = 1 - cur;
        rounds++;
        rewalked += ch;
        if (!ch) break;
    }
    if ((e = launch_exclusive_scan_u64(cnt, basev, nseg, s, st))) return e;
    hipLaunchKernelGGL(k_rag_first_invalid, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, st, nseg, ex[cur], words);
    hipLaunchKernelGGL(k_rag_verdict, dim3(1), dim3(64), 0, st, f, blob, nseg, n, cnt, basev, bad, words);
    if ((e = hipGetLastError())) return e;
    unsigned long long w[RAGW_N];
    if ((e = hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, st))) return e;
    if ((e = hipStreamSynchronize(st))) return e;
    res->parsed = w[RAGW_PARSED];
    res->last_seg = w[RAGW_LAST];
    res->bad_pos = w[RAGW_BAD];
    res->bad_len = w[RAGW_BADLEN];
    res->why = (uint32_t)w[RAGW_WHY];
    res->segments = nseg;
    res->rounds = rounds;
    res->rewalked = rewalked;
    t->first = first;
    t->cnt = cnt;
    t->basev = basev;
    t->tomb = bad;  // (the verdict has read where the chain broke)
    t->words = words;
    return hipSuccess;
}

hipError_t ragged_decode(const RagFmt &f, const uint8_t *blob, uint64_t n, const RagTables &t, const RagResult &res,
                         const RagCols &c, Scratch &s, hipStream_t st) {
    hipError_t e;
    const bool var = f.val_mode == RagFmt::VAL_VAR;
    uint64_t *vlen = var ? static_cast<uint64_t *>(s.get(107, (n + 1) * 8)) : nullptr;
    uint64_t *vsrc = var || f.val_len > RAG_INLINE_VAL ? static_cast<uint64_t *>(s.get(108, n * 8)) : nullptr;
    if (s.err) return s.err;
    if (var && (e = hipMemsetAsync(vlen + n, 0, 8, st))) return e;
    const RagOutDev o{c.keys, c.phys, c.logical, c.node, c.tags, c.values, vlen, vsrc};
    const uint32_t lds = rag_stage_bytes(f) + (rag_list_cap(f) + 1) * 4;
    hipLaunchKernelGGL(k_rag_list, dim3((unsigned)(res.last_seg + 1)), dim3(64), lds, st, f, blob, n, t.first, t.cnt,
                       t.basev, o, t.tomb, t.words);
    hipLaunchKernelGGL(k_rag_sum, dim3((unsigned)(res.last_seg / RAG_SUM_TILE + 1)), dim3(256), 0, st, t.tomb,
                       res.last_seg + 1, t.words);
    if ((e = hipGetLastError())) return e;
    if (var && (e = launch_exclusive_scan_u64(vlen, c.voffs, n + 1, s, st))) return e;
    return hipSuccess;
}

hipError_t ragged_copy_values(const RagFmt &f, const uint8_t *blob, uint64_t n, const RagCols &c, Scratch &s,
                              hipStream_t st) {
    const bool var = f.val_mode == RagFmt::VAL_VAR;
    if (!var && f.val_len <= RAG_INLINE_VAL) return hipSuccess;
    const uint64_t *vsrc = static_cast<const uint64_t *>(s.get(108, n * 8));
    if (s.err) return s.err;
    const uint64_t cap = var ? c.heap_cap : n * f.val_len;
    if (var) hipLaunchKernelGGL(k_rag_pad_heap, dim3(1), dim3(64), 0, st, c.voffs, n, c.values, cap);
    hipLaunchKernelGGL(k_rag_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f, blob, n, c.tags, vsrc, c.voffs,
                       c.values, cap);
    return hipGetLastError();
}

}  // namespace rh
