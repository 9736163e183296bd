// snap_encode.hip -- device columns into RCNL v1 bytes (snap_encode.hpp).
//
// An entry's length follows from its own row (its tag, a string key's length byte, a VARBYTES
// value's two offsets), so the file is laid out by one pass and a scan:
//   lengths  one lane per entry: len[i]; tombstones counted per workgroup, summed by k_enc_sum
//   scan     exclusive, over n + 1 lengths: start[i] relative to offset 16, start[n] = the total
//   write    a workgroup per 256 consecutive entries.  Their bytes are one contiguous span of the
//            file, [16 + start[b0], 16 + start[b1]) (workgroup 0 owns the 16 header bytes too).
//            The span is cut into windows of ENC_WIN bytes on 16-byte boundaries of the file; a
//            window is assembled in LDS at its final relative positions -- every lane its entry's
//            fixed part (key prefix, key, stamp, variant, value prefix or a u32 / u64 value) from
//            full-width column loads, every wave its 64 entries' value bytes, eight values at a
//            time, 8 lanes a value, a lane's loads all issued before its first LDS store -- and
//            then streamed out: whole 16-byte granules as one aligned store per lane, a wave's
//            lanes on consecutive granules.  A value's part of a window of
//            ENC_DIRECT bytes or more does not pass the LDS: the whole wave copies its granules
//            from the source straight to the file, 4 KiB a step (enc_direct).
// Two workgroups meet only in the granule that holds a span's edge.  There each writes its own
// bytes with byte stores; nothing is read back and no word is rewritten, so there is no race.
// The length pass and the write pass clip through the same functions (enc_klen, enc_value): with
// malformed columns the file is wrong but well-formed, and every access stays inside the columns,
// the LDS window and out[0 .. total).
#include "snap_encode.hpp"

#include "byte_window.hpp"

namespace rh {

namespace {

constexpr uint32_t ENC_BLOCK = 256;   // entries per workgroup
// the window and the value copies are byte_window.hpp's (shared with the ragged route, shard_route.hip)
constexpr uint32_t ENC_WIN = BW_WIN, ENC_DIRECT = BW_DIRECT, ENC_GROUP = BW_GROUP, ENC_LDS = BW_LDS;
constexpr uint64_t ENC_SUM_TILE = 4096;

// a string key's length: the row's last byte, clipped as the lift clips it
__device__ inline uint32_t enc_klen(const RagFmt &f, const uint8_t *keys, uint64_t i) {
    if (f.key_mode != RagFmt::KEY_STR) return f.key_len;
    const uint32_t W = f.key_len;
    const uint32_t last = reinterpret_cast<const uint32_t *>(keys + i * W)[W / 4 - 1] >> 24;
    return last < W - 1 ? last : W - 1;
}

// where a present entry's value bytes are read and how many: a span that decreases or starts past
// the heap is empty, one that ends past it is cut at the heap's end
__device__ inline void enc_value(const RagFmt &f, const EncCols &c, uint64_t i, uint64_t *src, uint64_t *len) {
    if (f.val_mode == RagFmt::VAL_VAR) {
        const uint64_t o0 = c.voffs[i], o1 = c.voffs[i + 1];
        if (o0 > c.vlimit || o1 < o0) {
            *src = 0, *len = 0;
        } else {
            *src = o0;
            *len = (o1 < c.vlimit ? o1 : c.vlimit) - o0;
        }
    } else {
        *src = i * f.val_len;
        *len = f.val_len;
    }
}

__device__ inline uint32_t enc_key_prefix(const RagFmt &f) { return f.key_mode != RagFmt::KEY_RAW ? 8u : 0u; }
// the bytes of an entry before the value's own bytes (a u32 / u64 value counts as fixed)
__device__ inline uint32_t enc_fixed_len(const RagFmt &f, uint32_t klen, uint32_t tag) {
    return enc_key_prefix(f) + klen + 24u + (tag ? 0u : f.val_mode != RagFmt::VAL_RAW ? 8u : f.val_len);
}

__global__ __launch_bounds__(256) void k_enc_len(RagFmt f, EncCols c, uint64_t n, uint64_t *len, uint64_t *tomb) {
    __shared__ uint32_t part[4];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t t = 0;
    if (i < n) {
        t = c.tags && c.tags[i] ? 1u : 0u;
        uint64_t l = enc_fixed_len(f, enc_klen(f, c.keys, i), t);
        if (!t && f.val_mode != RagFmt::VAL_RAW) {
            uint64_t vs, vl;
            enc_value(f, c, i, &vs, &vl);
            l += vl;
        }
        len[i] = l;
    } else if (i == n) {
        len[i] = 0;
    }
    for (int d = 32; d; d >>= 1) t += __shfl_xor(t, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    // a count per workgroup, summed by k_enc_sum (no same-address atomic per wave)
    if (threadIdx.x == 0) tomb[blockIdx.x] = (uint64_t)part[0] + part[1] + part[2] + part[3];
}

// *total += the workgroups' tombstone counts, ENC_SUM_TILE of them and one atomic per workgroup
__global__ __launch_bounds__(256) void k_enc_sum(const uint64_t *tomb, uint64_t nblk, unsigned long long *total) {
    __shared__ unsigned long long part[256];
    unsigned long long t = 0;
    const uint64_t lo = (uint64_t)blockIdx.x * ENC_SUM_TILE, hi = lo + ENC_SUM_TILE < nblk ? lo + ENC_SUM_TILE : nblk;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += 256) t += tomb[i];
    part[threadIdx.x] = t;
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && part[0]) atomicAdd(total, part[0]);
}

__device__ inline uint64_t shfl64(uint64_t v, int k) { return bw_shfl64(v, k); }

// the low nb bytes of v to win[r ..), the bytes that fall outside the window dropped
__device__ inline void enc_put(uint8_t *win, int32_t r, uint32_t v, uint32_t nb) {
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
        if (b < nb && (uint32_t)(r + (int32_t)b) < ENC_WIN) win[r + (int32_t)b] = (uint8_t)(v >> (8 * b));
}
__device__ inline void enc_put64(uint8_t *win, int32_t r, uint64_t v) {
    enc_put(win, r, (uint32_t)v, 4);
    enc_put(win, r + 4, (uint32_t)(v >> 32), 4);
}
__device__ inline uint32_t enc_left(uint32_t klen, uint32_t j) { return klen > j ? (klen - j < 4 ? klen - j : 4u) : 0u; }

// Bytes [S, S + N) of the value column to win[R .. R + N) (inside the window, N < ENC_DIRECT), by
// ENC_GROUP lanes (bw_copy).  Every read lies inside [S, S + N).
__device__ inline void enc_copy(const EncCols &c, uint8_t *win, uint64_t S, uint32_t R, uint32_t N, uint32_t sub) {
    bw_copy(c.values + S, win, R, N, sub);
}

// A long part of a value (N >= ENC_DIRECT), by the whole wave, straight to the file (bw_direct: its
// whole 16-byte granules are all this value's, so all this workgroup's).  File offset of the part:
// w + R (w a multiple of 16).
__device__ inline void enc_direct(const EncCols &c, uint8_t *win, uint32_t *direct, uint8_t *out, uint64_t w,
                                  uint64_t S, uint32_t R, uint32_t N, uint32_t lane) {
    bw_direct(c.values + S, win, direct, out + w, R, N, lane);
}

__global__ __launch_bounds__(256) void k_enc_write(RagFmt f, EncCols c, uint64_t n, const uint64_t *start, uint8_t *out) {
    extern __shared__ __align__(16) uint8_t win[];  // (no static LDS in this kernel: the base stays 16-byte aligned)
    uint32_t *direct = reinterpret_cast<uint32_t *>(win + ENC_WIN);
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t b0 = (uint64_t)blockIdx.x * ENC_BLOCK;
    const uint64_t b1 = b0 + ENC_BLOCK < n ? b0 + ENC_BLOCK : n;
    const uint64_t lo = blockIdx.x ? 16 + start[b0] : 0;  // the span this workgroup owns
    const uint64_t hi = n ? 16 + start[b1] : 16;
    const uint64_t i = b0 + tid;
    const bool have = i < b1;
    uint64_t es = 0, vsrc = 0, vdst = 0, cl = 0;  // entry start; the value's bytes: source, file offset, count
    uint32_t klen = 0, tag = 0, fixlen = 0;
    if (have) {
        es = 16 + start[i];
        tag = c.tags && c.tags[i] ? 1u : 0u;
        klen = enc_klen(f, c.keys, i);
        fixlen = enc_fixed_len(f, klen, tag);
        vdst = es + fixlen;
        if (!tag && f.val_mode != RagFmt::VAL_RAW) enc_value(f, c, i, &vsrc, &cl);
    }
    for (uint64_t w = lo & ~15ull; w < hi; w += ENC_WIN) {
        const uint64_t whi = w + ENC_WIN;
        if (tid < ENC_WIN / 16 / 32) direct[tid] = 0;
        __syncthreads();
        if (blockIdx.x == 0 && w == 0 && tid == 0) {
            uint32_t *h = reinterpret_cast<uint32_t *>(win);
            h[0] = 0x4c4e4352u;  // "RCNL"
            h[1] = 1u;
            h[2] = (uint32_t)n;
            h[3] = (uint32_t)(n >> 32);
        }
        if (have && es < whi && es + fixlen > w) {
            int32_t r = (int32_t)(int64_t)(es - w);
            if (f.key_mode != RagFmt::KEY_RAW) {
                enc_put64(win, r, klen);
                r += 8;
            }
            const uint32_t W = f.key_len;
            if (W >= 16) {
                const uint4 *row = reinterpret_cast<const uint4 *>(c.keys + i * W);
                for (uint32_t j = 0; j < W && j < klen; j += 16) {
                    const uint4 q = row[j / 16];
                    enc_put(win, r + (int32_t)j, q.x, enc_left(klen, j));
                    enc_put(win, r + (int32_t)j + 4, q.y, enc_left(klen, j + 4));
                    enc_put(win, r + (int32_t)j + 8, q.z, enc_left(klen, j + 8));
                    enc_put(win, r + (int32_t)j + 12, q.w, enc_left(klen, j + 12));
                }
            } else if (W == 8) {
                enc_put64(win, r, reinterpret_cast<const uint64_t *>(c.keys)[i]);
            } else if (W == 4) {
                enc_put(win, r, reinterpret_cast<const uint32_t *>(c.keys)[i], 4);
            }
            r += (int32_t)klen;
            enc_put64(win, r, c.phys[i]);
            enc_put(win, r + 8, c.logical[i], 4);
            enc_put64(win, r + 12, c.node[i]);
            enc_put(win, r + 20, tag, 4);
            r += 24;
            if (!tag) {
                if (f.val_mode != RagFmt::VAL_RAW) enc_put64(win, r, cl);
                else if (f.val_len == 8) enc_put64(win, r, reinterpret_cast<const uint64_t *>(c.values)[i]);
                else if (f.val_len == 4) enc_put(win, r, reinterpret_cast<const uint32_t *>(c.values)[i], 4);
            }
        }
        // the part of every value that lies in this window, a wave's 64 entries in turn
        uint64_t cs = 0;
        uint32_t cr = 0, cn = 0;
        if (cl) {
            const uint64_t a = vdst > w ? vdst : w, e = vdst + cl < whi ? vdst + cl : whi;
            if (a < e) cs = vsrc + (a - vdst), cr = (uint32_t)(a - w), cn = (uint32_t)(e - a);
        }
        unsigned long long ml = __ballot(cn >= ENC_DIRECT);  // the long parts, one at a time
        while (ml) {
            const int k = __ffsll((long long)ml) - 1;
            ml &= ml - 1;
            enc_direct(c, win, direct, out, w, shfl64(cs, k), __shfl(cr, k), __shfl(cn, k), lane);
        }
        const unsigned long long m = __ballot(cn != 0 && cn < ENC_DIRECT);  // the others, NG at a time
        constexpr uint32_t NG = 64 / ENC_GROUP;
        for (uint32_t r = 0; r < 64 / NG; r++) {
            if (!((m >> (r * NG)) & ((1ull << NG) - 1))) continue;  // (the same in every lane)
            const int k = (int)(r * NG + lane / ENC_GROUP);
            const uint64_t S = shfl64(cs, k);
            const uint32_t R = __shfl(cr, k), N = __shfl(cn, k);
            if (N && N < ENC_DIRECT) enc_copy(c, win, S, R, N, lane % ENC_GROUP);
        }
        __syncthreads();
        for (uint32_t g = tid; g < ENC_WIN / 16; g += ENC_BLOCK) {
            const uint64_t a = w + (uint64_t)g * 16;
            if (a >= hi) break;
            if ((direct[g >> 5] >> (g & 31)) & 1) continue;
            if (a >= lo && a + 16 <= hi) {
                reinterpret_cast<uint4 *>(out)[a / 16] = reinterpret_cast<const uint4 *>(win)[g];
            } else {  // a span's edge: its own bytes only (the rest of the granule is a neighbour's)
                for (uint32_t b = 0; b < 16; b++)
                    if (a + b >= lo && a + b < hi) out[a + b] = win[g * 16 + b];
            }
        }
        __syncthreads();
    }
}

}  // namespace

hipError_t encode_measure(const RagFmt &f, const EncCols &c, uint64_t n, Scratch &s, hipStream_t st, EncSizes *sz) {
    hipError_t e;
    const uint64_t nblk = n / 256 + 1;  // (covers row n, the scan's extra element)
    uint64_t *len = static_cast<uint64_t *>(s.get(110, (n + 1) * 8));
    uint64_t *start = static_cast<uint64_t *>(s.get(111, (n + 1) * 8));
    uint64_t *tomb = static_cast<uint64_t *>(s.get(112, nblk * 8));
    unsigned long long *total = static_cast<unsigned long long *>(s.get(113, 8));
    if (s.err) return s.err;
    if ((e = hipMemsetAsync(total, 0, 8, st))) return e;
    hipLaunchKernelGGL(k_enc_len, dim3((unsigned)nblk), dim3(256), 0, st, f, c, n, len, tomb);
    hipLaunchKernelGGL(k_enc_sum, dim3((unsigned)((nblk + ENC_SUM_TILE - 1) / ENC_SUM_TILE)), dim3(256), 0, st, tomb, nblk,
                       total);
    if ((e = hipGetLastError())) return e;
    if ((e = launch_exclusive_scan_u64(len, start, n + 1, s, st))) return e;
    unsigned long long w[2] = {0, 0};
    if ((e = hipMemcpyAsync(&w[0], start + n, 8, hipMemcpyDeviceToHost, st))) return e;
    if ((e = hipMemcpyAsync(&w[1], total, 8, hipMemcpyDeviceToHost, st))) return e;
    if ((e = hipStreamSynchronize(st))) return e;
    sz->entry_bytes = w[0];
    sz->tombstones = w[1];
    return hipSuccess;
}

hipError_t encode_write(const RagFmt &f, const EncCols &c, uint64_t n, uint8_t *out, Scratch &s, hipStream_t st) {
    const uint64_t *start = n ? static_cast<const uint64_t *>(s.get(111, (n + 1) * 8)) : nullptr;
    if (s.err) return s.err;
    const uint64_t nblk = n ? (n + ENC_BLOCK - 1) / ENC_BLOCK : 1;
    hipLaunchKernelGGL(k_enc_write, dim3((unsigned)nblk), dim3(ENC_BLOCK), ENC_LDS, st, f, c, n, start, out);
    return hipGetLastError();
}

}  // namespace rh
