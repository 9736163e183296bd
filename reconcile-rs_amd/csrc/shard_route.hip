// shard_route.hip -- a stable multi-way partition of record columns by the sharded store's splitters.
//
// Record i goes to shard s(i) = the number of splitters <= key[i] (bisect_right: rh_sstore's owner()),
// in the store kernels' key order.  The output holds one contiguous segment per shard, the rows of a
// shard in input order, every segment starting at a multiple of 16 rows (so that each column pointer
// of a segment meets the 16-byte rule for device columns); the rows between a segment's end and the
// next multiple of 16 are zero-filled.  Four steps on one stream:
//   count    a workgroup per tile of ROUTE_TILE rows: the splitters normalised into LDS, every row's
//            shard by binary search, a histogram of the tile per shard -> cnt[shard][workgroup]
//   scan     exclusive, over cnt in (shard, workgroup) order (the library's 64-bit scan): the rows
//            of lower shards plus this shard's rows of earlier tiles
//   starts   one wave: per-shard counts and the aligned segment starts -> meta (read back by the host)
//   scatter  the count pass again, now keeping each row's rank among its tile's rows of the same
//            shard (tile_ranks: the same code forms the histogram and the ranks, so the two passes
//            cannot disagree), which with the scan gives its output row -- kept in LDS; then every
//            column is moved, the tile's elements taken by consecutive lanes: a row wider than 16
//            bytes is copied by as many lanes as it has 16-byte pieces (a 1 KiB value by a whole
//            wave), reads fully coalesced, writes coalesced within a row and across rows that stay
//            neighbours.  The last `shards` workgroups zero the gap rows instead.
// Nothing is read at or past row n; nothing is written at or past row start[G - 1] +
// roundup16(count[G - 1]) <= n + 15 * shards.
// A VARBYTES value column (rh_route_columns_var_device) adds three steps, described at route_span:
// the scatter pass leaves each output row's clipped value length and source offset in scratch, a
// scan of the lengths gives the heap offsets, and a copy pass packs the bytes in output-row order.
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsos_hip.h"
#include "abi_error.hpp"
#include "byte_window.hpp"
#include "shard_route.hpp"

namespace rh {

namespace {

constexpr uint32_t WG = 256, WAVES = WG / 64, STEPS = ROUTE_TILE / WG;

template <int KB>
constexpr int digits_of() {
    return KB <= 8 ? 1 : KB / 8;
}

// A key row as 64-bit digits, most significant first, whose unsigned order is the key order:
// u32 / u64 keys by value, byte rows by their bytes read big-endian
template <int KB, bool NUM>
__device__ __forceinline__ void route_digits(const uint8_t *row, uint64_t *d) {
    if constexpr (KB == 4) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(row);
        d[0] = NUM ? v : __builtin_bswap32(v);
    } else if constexpr (KB == 8) {
        const uint64_t v = *reinterpret_cast<const uint64_t *>(row);
        d[0] = NUM ? v : __builtin_bswap64(v);
    } else {
#pragma unroll
        for (int q = 0; q < KB / 16; q++) {
            const uint4 v = reinterpret_cast<const uint4 *>(row)[q];
            d[2 * q] = __builtin_bswap64((uint64_t)v.x | ((uint64_t)v.y << 32));
            d[2 * q + 1] = __builtin_bswap64((uint64_t)v.z | ((uint64_t)v.w << 32));
        }
    }
}

// the number of splitters <= the key (sp: G - 1 normalised splitters, non-decreasing)
template <int ND>
__device__ __forceinline__ int route_owner(const uint64_t *sp, int G, const uint64_t *d) {
    int lo = 0, hi = G - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint64_t *s = sp + mid * ND;
        bool le = true;  // splitter <= key
#pragma unroll
        for (int q = 0; q < ND; q++)
            if (s[q] != d[q]) {
                le = s[q] < d[q];
                break;
            }
        if (le) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct RouteArgs {
    const uint8_t *keys;
    const uint8_t *split;
    uint64_t n;
    int shards;
    uint32_t nwg;          // tiles
    uint64_t *cnt;         // [shard][tile] (count pass out)
    const uint64_t *scan;  // its exclusive scan (scatter pass in)
    uint64_t *meta;        // counts, then starts
    RouteCol cols[ROUTE_MAX_COLS];
    int ncols;
};

// The LDS both passes share.  dest is used by the scatter pass only.
template <int ND, bool SCATTER>
struct RouteLds {
    uint64_t sp[(ROUTE_MAX_SHARDS - 1) * ND];
    uint32_t wcnt[2][WAVES][ROUTE_MAX_SHARDS];  // a step's rows per (wave, shard), double-buffered
    uint32_t running[ROUTE_MAX_SHARDS];         // the tile's rows per shard in the steps so far
    uint64_t base[ROUTE_MAX_SHARDS];            // the output row of the tile's first row of a shard
    uint64_t dest[SCATTER ? ROUTE_TILE : 1];    // each tile row's output row
};

// Every tile row's shard and its rank among the tile's earlier rows of that shard (tile order: row
// k * 256 + tid at step k).  On return L.running is the tile's histogram and, with SCATTER,
// L.dest[r] = L.base[shard] + rank.  The lanes of a wave that hold one shard find each other with
// six ballots (a shard number has six bits); the lowest of them posts the wave's count.
template <int KB, bool NUM, bool SCATTER>
__device__ __forceinline__ void tile_ranks(const RouteArgs &a, RouteLds<digits_of<KB>(), SCATTER> &L, uint64_t tile0,
                                           uint32_t rows) {
    constexpr int ND = digits_of<KB>();
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = a.shards;
    for (uint32_t k = 0; k * WG < rows; k++) {
        const uint32_t r = k * WG + tid;
        const bool valid = r < rows;
        int s = 0;
        if (valid) {
            uint64_t d[ND];
            route_digits<KB, NUM>(a.keys + (tile0 + r) * KB, d);
            s = route_owner<ND>(L.sp, G, d);
        }
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 6; b++) {
            const unsigned long long bal = __ballot((s >> b) & 1);
            peers &= ((s >> b) & 1) ? bal : ~bal;
        }
        const uint32_t rank = __popcll(peers & ((1ull << lane) - 1));
        uint32_t(*wc)[ROUTE_MAX_SHARDS] = L.wcnt[k & 1];
        if (valid && rank == 0) wc[wave][s] = __popcll(peers);
        __syncthreads();
        if (SCATTER && valid) {
            uint32_t pre = L.running[s] + rank;
            for (uint32_t w = 0; w < wave; w++) pre += wc[w][s];
            L.dest[r] = L.base[s] + pre;
        }
        __syncthreads();
        if (tid < ROUTE_MAX_SHARDS) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < WAVES; w++) t += wc[w][tid];
            L.running[tid] += t;
        }
        (&L.wcnt[(k + 1) & 1][0][0])[tid] = 0;  // the other buffer, read last a step ago
        __syncthreads();
    }
}

template <int KB, bool NUM, bool SCATTER>
__device__ __forceinline__ void tile_setup(const RouteArgs &a, RouteLds<digits_of<KB>(), SCATTER> &L) {
    constexpr int ND = digits_of<KB>();
    const uint32_t tid = threadIdx.x;
    static_assert(WAVES * ROUTE_MAX_SHARDS == WG, "one wcnt entry per thread");
    if ((int)tid < a.shards - 1) route_digits<KB, NUM>(a.split + (uint64_t)tid * KB, L.sp + tid * ND);
    (&L.wcnt[0][0][0])[tid] = 0;
    (&L.wcnt[1][0][0])[tid] = 0;
    if (tid < ROUTE_MAX_SHARDS) L.running[tid] = 0;
    if (SCATTER && (int)tid < a.shards) {
        const uint64_t *row = a.scan + (uint64_t)tid * a.nwg;  // this shard's tiles
        L.base[tid] = a.meta[a.shards + tid] + (row[blockIdx.x] - row[0]);
    }
    __syncthreads();
}

template <int KB, bool NUM>
__global__ __launch_bounds__(256) void k_route_count(RouteArgs a) {
    __shared__ RouteLds<digits_of<KB>(), false> L;
    const uint64_t tile0 = (uint64_t)blockIdx.x * ROUTE_TILE;
    const uint32_t rows = (uint32_t)(a.n - tile0 < ROUTE_TILE ? a.n - tile0 : ROUTE_TILE);
    tile_setup<KB, NUM, false>(a, L);
    tile_ranks<KB, NUM, false>(a, L, tile0, rows);
    if ((int)threadIdx.x < a.shards) a.cnt[(uint64_t)threadIdx.x * a.nwg + blockIdx.x] = L.running[threadIdx.x];
}

// counts and aligned starts from the scan: shard s's rows begin at scan[s][0] in the unpadded order
__global__ __launch_bounds__(64) void k_route_starts(const uint64_t *scan, uint32_t nwg, uint64_t n, int G,
                                                     uint64_t *meta) {
    __shared__ uint64_t cnt[ROUTE_MAX_SHARDS];
    const int t = threadIdx.x;
    if (t < G) {
        const uint64_t lo = scan[(uint64_t)t * nwg], hi = t + 1 < G ? scan[(uint64_t)(t + 1) * nwg] : n;
        cnt[t] = hi - lo;
        meta[t] = hi - lo;
    }
    __syncthreads();
    if (t == 0) {
        uint64_t at = 0;
        for (int s = 0; s < G; s++) {
            meta[G + s] = at;
            at += (cnt[s] + ROUTE_ALIGN - 1) & ~(ROUTE_ALIGN - 1);
        }
    }
}

// a tile's rows of one column to their output rows, element c of the tile by thread c mod 256
template <class T>
__device__ __forceinline__ void move_column(const RouteCol &c, uint64_t tile0, uint32_t rows, const uint64_t *dest) {
    const T *__restrict__ src = reinterpret_cast<const T *>(c.src) + tile0 * c.units;
    T *__restrict__ dst = reinterpret_cast<T *>(c.dst);
    const uint32_t total = rows * c.units;
#pragma unroll 4
    for (uint32_t e = threadIdx.x; e < total; e += WG) {
        const uint32_t r = c.shift >= 0 ? e >> c.shift : e / c.units;
        dst[dest[r] * c.units + (e - r * c.units)] = src[e];
    }
}

template <class T>
__device__ __forceinline__ void zero_rows(const RouteCol &c, uint64_t row0, uint64_t row1) {
    T *dst = reinterpret_cast<T *>(c.dst) + row0 * c.units;
    const uint64_t total = (row1 - row0) * c.units;
    for (uint64_t e = threadIdx.x; e < total; e += WG) dst[e] = T{};
}

// workgroups [0, nwg): a tile each; workgroups [nwg, nwg + shards): a shard's gap rows each.
// Returns the tile's rows with L.dest complete (0 for a gap workgroup).
template <int KB, bool NUM>
__device__ __forceinline__ uint32_t scatter_tile(const RouteArgs &a, RouteLds<digits_of<KB>(), true> &L) {
    if (blockIdx.x >= a.nwg) {
        const int s = (int)(blockIdx.x - a.nwg);
        const uint64_t end = a.meta[a.shards + s] + a.meta[s];
        const uint64_t stop = (end + ROUTE_ALIGN - 1) & ~(ROUTE_ALIGN - 1);  // (a start is a multiple of 16)
        for (int j = 0; j < a.ncols; j++) {
            const RouteCol &c = a.cols[j];
            if (c.unit == 16) zero_rows<uint4>(c, end, stop);
            else if (c.unit == 8) zero_rows<uint64_t>(c, end, stop);
            else if (c.unit == 4) zero_rows<uint32_t>(c, end, stop);
            else zero_rows<uint8_t>(c, end, stop);
        }
        return 0;
    }
    const uint64_t tile0 = (uint64_t)blockIdx.x * ROUTE_TILE;
    const uint32_t rows = (uint32_t)(a.n - tile0 < ROUTE_TILE ? a.n - tile0 : ROUTE_TILE);
    tile_setup<KB, NUM, true>(a, L);
    tile_ranks<KB, NUM, true>(a, L, tile0, rows);  // (ends with a barrier: dest is complete)
    for (int j = 0; j < a.ncols; j++) {
        const RouteCol &c = a.cols[j];
        if (c.unit == 16) move_column<uint4>(c, tile0, rows, L.dest);
        else if (c.unit == 8) move_column<uint64_t>(c, tile0, rows, L.dest);
        else if (c.unit == 4) move_column<uint32_t>(c, tile0, rows, L.dest);
        else move_column<uint8_t>(c, tile0, rows, L.dest);
    }
    return rows;
}

template <int KB, bool NUM>
__global__ __launch_bounds__(256) void k_route_scatter(RouteArgs a) {
    __shared__ RouteLds<digits_of<KB>(), true> L;
    scatter_tile<KB, NUM>(a, L);
}

// ---- a VARBYTES value column (rh_route_columns_var_device) ------------------------------------------
// The scatter pass also leaves, per output row, the row's clipped value length and where its bytes
// start in the input heap (vlen / vsrc: scratch of rows + 1 entries, vlen zeroed before the pass, so
// gap rows and the entry behind the last row hold 0); an exclusive scan of vlen gives every output
// row's heap offset (vpos); the copy pass then moves the bytes.  The one place a span is clipped:
// a span that decreases or starts past the heap is empty, one that ends past it is cut at its end
// (snap_encode.hip's enc_value)
__device__ __forceinline__ void route_span(const uint64_t *offs, uint64_t limit, uint64_t i, uint64_t *src, uint64_t *len) {
    const uint64_t o0 = offs[i], o1 = offs[i + 1];
    if (o0 > limit || o1 < o0) {
        *src = 0, *len = 0;
    } else {
        *src = o0;
        *len = (o1 < limit ? o1 : limit) - o0;
    }
}

template <int KB, bool NUM>
__global__ __launch_bounds__(256) void k_route_scatter_var(RouteArgs a, RouteVar v, uint64_t *vlen, uint64_t *vsrc) {
    __shared__ RouteLds<digits_of<KB>(), true> L;
    const uint32_t rows = scatter_tile<KB, NUM>(a, L);
    const uint64_t tile0 = (uint64_t)blockIdx.x * ROUTE_TILE;
    for (uint32_t r = threadIdx.x; r < rows; r += WG) {
        uint64_t src, len;
        route_span(v.offs_in, v.limit_in, tile0 + r, &src, &len);
        vlen[L.dest[r]] = len;
        vsrc[L.dest[r]] = src;
    }
}

// The copy pass: a workgroup per VAR_BLOCK consecutive output rows.  Their values are one contiguous
// span of the output heap, [vpos[b0], vpos[b1]), at byte granularity against sources of any alignment
// -- snap_encode.hip's write pass without an entry's fixed part.  The span is cut into windows of
// VAR_WIN bytes on 16-byte boundaries of the output's address; a window is assembled in LDS at its
// final relative positions (every wave its 64 rows' parts, eight at a time, VAR_GROUP lanes a part, a
// lane's loads all issued before its first LDS store) and streamed out as one aligned 16-byte store
// per lane.  A part of VAR_DIRECT bytes or more does not pass the LDS: the whole wave copies its
// whole granules straight from the source, 4 KiB a step.  Two workgroups meet only in the granule
// holding a span's edge, where each writes its own bytes with byte stores: nothing is read back and
// no word is rewritten.  Positions are kept relative to the 16-byte boundary at or below bytes_out
// (`mis` bytes before it: the heap is only 4-byte aligned).
constexpr uint32_t VAR_BLOCK = 256;
// the window and the copies of a part are byte_window.hpp's (shared with snap_encode.hip)
constexpr uint32_t VAR_WIN = BW_WIN, VAR_DIRECT = BW_DIRECT, VAR_GROUP = BW_GROUP, VAR_LDS = BW_LDS;

// meta: counts, starts (G each), then [2 G] <- the routed heap's bytes.  vpos: the scan of vlen.
__global__ __launch_bounds__(256) void k_route_var_copy(RouteVar v, const uint64_t *meta, int G, const uint64_t *vlen,
                                                        const uint64_t *vsrc, const uint64_t *vpos, uint64_t *meta_total) {
    extern __shared__ __align__(16) uint8_t win[];  // (no static LDS in this kernel: the base stays 16-byte aligned)
    uint32_t *direct = reinterpret_cast<uint32_t *>(win + VAR_WIN);
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t R = meta[2 * G - 1] + ((meta[G - 1] + ROUTE_ALIGN - 1) & ~(ROUTE_ALIGN - 1));
    const uint64_t b0 = (uint64_t)blockIdx.x * VAR_BLOCK;
    if (b0 >= R) return;  // (the grid covers the most rows R can be)
    const uint64_t b1 = b0 + VAR_BLOCK < R ? b0 + VAR_BLOCK : R;
    const uint64_t total = vpos[R];
    const uint64_t i = b0 + tid;
    const bool have = i < b1;
    uint64_t vdst = 0, cl = 0, src = 0;
    if (have) {
        vdst = vpos[i];
        v.offs_out[i] = vdst;
        cl = vlen[i];
        if (cl) src = vsrc[i];
    }
    if (b1 == R && tid == 0) {
        v.offs_out[R] = total;
        *meta_total = total;
    }
    if (((total + 3) & ~3ull) > v.cap_out) return;  // does not fit: no heap byte is written (every workgroup agrees)
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(v.bytes_out) & 15u);
    uint8_t *base = v.bytes_out - mis;  // 16-byte aligned; nothing below base + mis is touched
    const uint64_t lo = vpos[b0] + mis, hi = vpos[b1] + mis;  // the span this workgroup owns
    vdst += mis;
    for (uint64_t w = lo & ~15ull; w < hi; w += VAR_WIN) {
        const uint64_t whi = w + VAR_WIN;
        if (tid < VAR_WIN / 16 / 32) direct[tid] = 0;
        __syncthreads();
        // the part of every value that lies in this window, a wave's 64 rows in turn
        uint64_t cs = 0;
        uint32_t cr = 0, cn = 0;
        if (cl) {
            const uint64_t a = vdst > w ? vdst : w, e = vdst + cl < whi ? vdst + cl : whi;
            if (a < e) cs = src + (a - vdst), cr = (uint32_t)(a - w), cn = (uint32_t)(e - a);
        }
        unsigned long long ml = __ballot(cn >= VAR_DIRECT);  // the long parts, one at a time
        while (ml) {
            const int k = __ffsll((long long)ml) - 1;
            ml &= ml - 1;
            bw_direct(v.bytes_in + bw_shfl64(cs, k), win, direct, base + w, __shfl(cr, k), __shfl(cn, k), lane);
        }
        const unsigned long long m = __ballot(cn != 0 && cn < VAR_DIRECT);  // the others, NG at a time
        constexpr uint32_t NG = 64 / VAR_GROUP;
        for (uint32_t r = 0; r < 64 / NG; r++) {
            if (!((m >> (r * NG)) & ((1ull << NG) - 1))) continue;  // (the same in every lane)
            const int k = (int)(r * NG + lane / VAR_GROUP);
            const uint64_t S = bw_shfl64(cs, k);
            const uint32_t Rw = __shfl(cr, k), N = __shfl(cn, k);
            if (N && N < VAR_DIRECT) bw_copy(v.bytes_in + S, win, Rw, N, lane % VAR_GROUP);
        }
        __syncthreads();
        for (uint32_t g = tid; g < VAR_WIN / 16; g += VAR_BLOCK) {
            const uint64_t a = w + (uint64_t)g * 16;
            if (a >= hi) break;
            if ((direct[g >> 5] >> (g & 31)) & 1) continue;
            if (a >= lo && a + 16 <= hi) {
                reinterpret_cast<uint4 *>(base)[a / 16] = reinterpret_cast<const uint4 *>(win)[g];
            } else {  // a span's edge: its own bytes only (the rest of the granule is a neighbour's)
                for (uint32_t b = 0; b < 16; b++)
                    if (a + b >= lo && a + b < hi) base[a + b] = win[g * 16 + b];
            }
        }
        __syncthreads();
    }
    // the bytes from the heap's end to the next multiple of 4 (inside cap_out: checked above)
    if (b1 == R && tid < ((4u - (uint32_t)(total & 3u)) & 3u)) v.bytes_out[total + tid] = 0;
}

template <int KB, bool NUM>
__global__ __launch_bounds__(256) void k_first_unsorted(const uint8_t *keys, uint64_t n, unsigned long long *first) {
    constexpr int ND = digits_of<KB>();
    const uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x + 1;
    if (i >= n) return;
    uint64_t a[ND], b[ND];
    route_digits<KB, NUM>(keys + (i - 1) * KB, a);
    route_digits<KB, NUM>(keys + i * KB, b);
    bool below = false;  // key[i - 1] < key[i]
#pragma unroll
    for (int q = 0; q < ND; q++)
        if (a[q] != b[q]) {
            below = a[q] < b[q];
            break;
        }
    if (!below) atomicMin(first, (unsigned long long)i);
}

template <int KB, bool NUM>
hipError_t first_unsorted_launch(const uint8_t *keys, uint64_t n, unsigned long long *first, hipStream_t st) {
    hipLaunchKernelGGL((k_first_unsorted<KB, NUM>), dim3((uint32_t)((n + WG - 1) / WG)), dim3(WG), 0, st, keys, n, first);
    return hipGetLastError();
}

template <int KB, bool NUM>
hipError_t route_launch(const RouteArgs &a0, Scratch &s, hipStream_t st, const RouteVar *var) {
    RouteArgs a = a0;
    const uint64_t cells = (uint64_t)a.shards * a.nwg;
    hipLaunchKernelGGL((k_route_count<KB, NUM>), dim3(a.nwg), dim3(WG), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e) return e;
    if ((e = launch_exclusive_scan_u64(a.cnt, const_cast<uint64_t *>(a.scan), cells, s, st))) return e;
    hipLaunchKernelGGL(k_route_starts, dim3(1), dim3(64), 0, st, a.scan, a.nwg, a.n, a.shards, a.meta);
    if (!var) {
        hipLaunchKernelGGL((k_route_scatter<KB, NUM>), dim3(a.nwg + (uint32_t)a.shards), dim3(WG), 0, st, a);
        return hipGetLastError();
    }
    // the most rows the output can hold (every segment but the first starts after at most 15 gap
    // rows, and so ends the last): the host learns the exact number only from the read-back
    const uint64_t rmax = a.n + ROUTE_ALIGN * (uint64_t)a.shards;
    uint64_t *vlen = static_cast<uint64_t *>(s.get(124, (rmax + 1) * 8));
    uint64_t *vsrc = static_cast<uint64_t *>(s.get(125, (rmax + 1) * 8));
    uint64_t *vpos = static_cast<uint64_t *>(s.get(126, (rmax + 1) * 8));
    if (s.err) return s.err;
    if ((e = hipMemsetAsync(vlen, 0, (rmax + 1) * 8, st))) return e;
    hipLaunchKernelGGL((k_route_scatter_var<KB, NUM>), dim3(a.nwg + (uint32_t)a.shards), dim3(WG), 0, st, a, *var, vlen,
                       vsrc);
    if ((e = hipGetLastError())) return e;
    if ((e = launch_exclusive_scan_u64(vlen, vpos, rmax + 1, s, st))) return e;
    hipLaunchKernelGGL(k_route_var_copy, dim3((uint32_t)((rmax + VAR_BLOCK - 1) / VAR_BLOCK)), dim3(VAR_BLOCK), VAR_LDS, st,
                       *var, a.meta, a.shards, vlen, vsrc, vpos, a.meta + 2 * a.shards);
    return hipGetLastError();
}

}  // namespace

RouteCol route_col(const void *src, void *dst, uint32_t row_bytes) {
    RouteCol c;
    c.src = static_cast<const uint8_t *>(src);
    c.dst = static_cast<uint8_t *>(dst);
    c.unit = row_bytes % 16 == 0 ? 16 : row_bytes % 8 == 0 ? 8 : row_bytes % 4 == 0 ? 4 : 1;
    c.units = row_bytes / c.unit;
    c.shift = -1;
    for (int b = 0; b < 31; b++)
        if (c.units == (1u << b)) c.shift = b;
    return c;
}

bool route_key_supported(uint32_t kb, bool numeric) {
    return numeric ? (kb == 4 || kb == 8) : (kb == 8 || kb == 16 || kb == 32 || kb == 64);
}

hipError_t launch_route(const RouteJob &job, const uint8_t *split, uint64_t *meta, Scratch &s, hipStream_t st,
                        const RouteVar *var) {
    RouteArgs a;
    a.keys = job.keys;
    a.split = split;
    a.n = job.n;
    a.shards = job.shards;
    a.nwg = (uint32_t)((job.n + ROUTE_TILE - 1) / ROUTE_TILE);
    const uint64_t cells = (uint64_t)a.shards * a.nwg;
    a.cnt = static_cast<uint64_t *>(s.get(120, cells * 8));
    a.scan = static_cast<uint64_t *>(s.get(121, cells * 8));
    if (s.err) return s.err;
    a.meta = meta;
    a.ncols = job.ncols;
    for (int j = 0; j < job.ncols; j++) a.cols[j] = job.cols[j];
    if (job.numeric) return job.key_bytes == 4 ? route_launch<4, true>(a, s, st, var) : route_launch<8, true>(a, s, st, var);
    switch (job.key_bytes) {
    case 8: return route_launch<8, false>(a, s, st, var);
    case 16: return route_launch<16, false>(a, s, st, var);
    case 32: return route_launch<32, false>(a, s, st, var);
    default: return route_launch<64, false>(a, s, st, var);
    }
}

hipError_t launch_first_unsorted(const uint8_t *keys, uint32_t kb, bool numeric, uint64_t n, unsigned long long *first,
                                 hipStream_t st) {
    hipError_t e = hipMemsetAsync(first, 0xff, 8, st);
    if (e || n < 2) return e;
    if (numeric) return kb == 4 ? first_unsorted_launch<4, true>(keys, n, first, st) : first_unsorted_launch<8, true>(keys, n, first, st);
    switch (kb) {
    case 8: return first_unsorted_launch<8, false>(keys, n, first, st);
    case 16: return first_unsorted_launch<16, false>(keys, n, first, st);
    case 32: return first_unsorted_launch<32, false>(keys, n, first, st);
    default: return first_unsorted_launch<64, false>(keys, n, first, st);
    }
}

}  // namespace rh

// =================================================================================================
namespace {

int fail(int code, const std::string &msg) { return rh::set_error(code, msg); }

#define RH_HIP(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return fail(e_ == hipErrorOutOfMemory ? RH_ERR_OOM : RH_ERR_HIP,                              \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                               \
    } while (0)

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

uint32_t key_row(const rh_schema &s) {
    return s.key_kind == RH_KEY_UNIT ? 0 : s.key_kind == RH_KEY_U32 ? 4 : s.key_kind == RH_KEY_U64 ? 8 : s.key_len;
}
uint32_t value_row(const rh_schema &s) {
    return s.value_kind == RH_VAL_UNIT ? 0 : s.value_kind == RH_VAL_U32 ? 4 : s.value_kind == RH_VAL_U64 ? 8 : s.value_len;
}

// the route's device scratch, one per device, kept between calls and held for a whole call (the
// call is synchronous): slots 120-121 the counts and their scan, 122 the splitters, 123 meta,
// 124-126 a VARBYTES column's per-row lengths, source offsets and heap offsets
struct RouteScratch {
    std::mutex mu;
    std::vector<rh::Scratch> by_dev;
};
RouteScratch &route_scratch() {
    static RouteScratch s;
    return s;
}

int key_cmp(const rh_schema &s, const uint8_t *a, const uint8_t *b) {
    if (s.key_kind == RH_KEY_U64) {
        uint64_t x, y;
        memcpy(&x, a, 8), memcpy(&y, b, 8);
        return (x > y) - (x < y);
    }
    if (s.key_kind == RH_KEY_U32) {
        uint32_t x, y;
        memcpy(&x, a, 4), memcpy(&y, b, 4);
        return (x > y) - (x < y);
    }
    return memcmp(a, b, s.key_len);
}

// rh_route_columns_device (heap_bytes NULL: VARBYTES refused) and rh_route_columns_var_device
int route_columns(const rh_schema *schema, const void *host_splitters, int shards, const rh_columns *in,
                  const uint8_t *ops_in, size_t n, const rh_columns *out, uint8_t *ops_out, size_t cap_rows,
                  uint64_t *counts, uint64_t *starts, uint64_t *heap_bytes, void *stream) {
    // every check on the arguments first: nothing below them fails for a reason the caller could have seen
    int rc = rh::check_schema_arg(schema);
    if (rc) return rc;
    const rh_schema &s = *schema;
    const bool var = s.value_kind == RH_VAL_VARBYTES;
    if (var && !heap_bytes)
        return fail(RH_ERR_UNSUPPORTED, "route: VARBYTES values are not routed (fixed-width value rows only; the "
                                        "sharded store does not take them either)");
    if (heap_bytes) *heap_bytes = 0;
    if (shards < 1 || shards > rh::ROUTE_MAX_SHARDS) return fail(RH_ERR_ARG, "route: shards must be 1..64");
    if (!counts || !starts) return fail(RH_ERR_ARG, "route: counts / starts is NULL");
    if (shards > 1 && !host_splitters) return fail(RH_ERR_ARG, "route: splitters is NULL");
    const uint32_t kl = key_row(s), vr = value_row(s);
    const bool numeric = s.key_kind == RH_KEY_U32 || s.key_kind == RH_KEY_U64;
    if (s.key_kind == RH_KEY_UNIT) return fail(RH_ERR_ARG, "route: unit keys have no key order to route by");
    if (!rh::route_key_supported(kl, numeric))
        return fail(RH_ERR_UNSUPPORTED, "route: keys must be u32, u64 or byte / string rows of 8, 16, 32 or 64 bytes");
    const uint8_t *sp = static_cast<const uint8_t *>(host_splitters);
    for (int j = 1; j + 1 < shards; j++)
        if (key_cmp(s, sp + (size_t)(j - 1) * kl, sp + (size_t)j * kl) > 0)
            return fail(RH_ERR_ARG, "route: splitters must not decrease");
    if (n >= (1ull << 32)) return fail(RH_ERR_ARG, "route: fewer than 2^32 rows per call");
    if (cap_rows < n + rh::ROUTE_ALIGN * (size_t)shards)
        return fail(RH_ERR_ARG, "route: cap_rows must be at least n + 16 * shards (nothing written)");
    for (int t = 0; t < shards; t++) counts[t] = starts[t] = 0;
    if (n == 0) return RH_OK;
    if (!in || !out) return fail(RH_ERR_ARG, "route: columns is NULL");
    rh::RouteJob job{};
    const char *bad = nullptr;
    auto add = [&](const void *src, const void *dst, uint32_t w, bool required, const char *name) {
        if (!src && !required) return;  // an absent column stays absent
        if (!src || !dst) bad = bad ? bad : name;
        else if (w % 4 == 0 && (!aligned16(src) || !aligned16(dst))) bad = bad ? bad : "alignment";
        else job.cols[job.ncols++] = rh::route_col(src, const_cast<void *>(dst), w);
    };
    const bool dated = s.record_kind == RH_REC_DATED;
    add(in->keys, out->keys, kl, true, "keys");
    if (dated) {
        add(in->phys, out->phys, 8, true, "phys");
        add(in->logical, out->logical, 4, true, "logical");
        add(in->node, out->node, 8, true, "node");
    }
    if (s.record_kind != RH_REC_PLAIN) add(in->tags, out->tags, 1, false, "tags");
    if (vr) add(in->values, out->values, vr, true, "values");
    add(ops_in, ops_out, 1, false, "ops");
    if (bad && !strcmp(bad, "alignment")) return fail(RH_ERR_ARG, "route: device columns must be 16-byte aligned");
    if (bad) return fail(RH_ERR_ARG, std::string("route: column ") + bad + " is NULL in the input or the output");
    rh::RouteVar rv{};
    if (var) {
        const rh_var_values *iv = static_cast<const rh_var_values *>(in->values);
        const rh_var_values *ov = static_cast<const rh_var_values *>(out->values);
        if (!iv || !ov) return fail(RH_ERR_ARG, "route: column values is NULL in the input or the output");
        auto misaligned = [](const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
        if (!iv->offsets || !ov->offsets || misaligned(iv->offsets, 8) || misaligned(ov->offsets, 8))
            return fail(RH_ERR_ARG, "route: VARBYTES offsets must be non-NULL and 8-byte aligned");
        if ((!iv->bytes && iv->bytes_len) || (!ov->bytes && ov->bytes_len))
            return fail(RH_ERR_ARG, "route: VARBYTES heap is NULL");
        if (misaligned(iv->bytes, 4) || misaligned(ov->bytes, 4) || iv->bytes_len % 4 || ov->bytes_len % 4)
            return fail(RH_ERR_ARG, "route: a VARBYTES heap must be 4-byte aligned and bytes_len a multiple of 4");
        rv = rh::RouteVar{iv->bytes,   iv->offsets, iv->bytes_len, const_cast<uint8_t *>(ov->bytes),
                          const_cast<uint64_t *>(ov->offsets), ov->bytes_len};
    }
    job.keys = static_cast<const uint8_t *>(in->keys);
    job.key_bytes = kl;
    job.numeric = numeric;
    job.n = n;
    job.shards = shards;

    hipStream_t st = static_cast<hipStream_t>(stream);
    int dev = 0;
    RH_HIP(hipGetDevice(&dev));
    RouteScratch &rs = route_scratch();
    std::lock_guard<std::mutex> g(rs.mu);
    if ((int)rs.by_dev.size() <= dev) rs.by_dev.resize(dev + 1);
    rh::Scratch &scr = rs.by_dev[dev];
    scr.stream = st;
    scr.err = hipSuccess;
    uint8_t *split = static_cast<uint8_t *>(scr.get(122, (size_t)rh::ROUTE_MAX_SHARDS * 64));
    uint64_t *meta = static_cast<uint64_t *>(scr.get(123, (2 * rh::ROUTE_MAX_SHARDS + 1) * 8));
    if (scr.err) return fail(RH_ERR_OOM, "route: scratch allocation failed");
    if (shards > 1) RH_HIP(hipMemcpyAsync(split, sp, (size_t)(shards - 1) * kl, hipMemcpyHostToDevice, st));
    RH_HIP(rh::launch_route(job, split, meta, scr, st, var ? &rv : nullptr));
    if (scr.err) return fail(RH_ERR_OOM, "route: scratch allocation failed");
    uint64_t h[2 * rh::ROUTE_MAX_SHARDS + 1];
    RH_HIP(hipMemcpyAsync(h, meta, (2 * (size_t)shards + (var ? 1 : 0)) * 8, hipMemcpyDeviceToHost, st));
    RH_HIP(hipStreamSynchronize(st));
    for (int t = 0; t < shards; t++) counts[t] = h[t], starts[t] = h[shards + t];
    if (var) {
        *heap_bytes = h[2 * shards];
        if (((h[2 * shards] + 3) & ~3ull) > rv.cap_out)
            return fail(RH_ERR_ARG, "route: the routed values need " + std::to_string(h[2 * shards]) +
                                        " bytes (rounded up to 4), more than the output heap's bytes_len");
    }
    return RH_OK;
}

}  // namespace

extern "C" int rh_route_columns_device(const rh_schema *schema, const void *host_splitters, int shards,
                                       const rh_columns *in, const uint8_t *ops_in, size_t n, const rh_columns *out,
                                       uint8_t *ops_out, size_t cap_rows, uint64_t *counts, uint64_t *starts,
                                       void *stream) {
    return route_columns(schema, host_splitters, shards, in, ops_in, n, out, ops_out, cap_rows, counts, starts, nullptr,
                         stream);
}

extern "C" int rh_route_columns_var_device(const rh_schema *schema, const void *host_splitters, int shards,
                                           const rh_columns *in, const uint8_t *ops_in, size_t n, const rh_columns *out,
                                           uint8_t *ops_out, size_t cap_rows, uint64_t *counts, uint64_t *starts,
                                           uint64_t *heap_bytes, void *stream) {
    if (!heap_bytes) return fail(RH_ERR_ARG, "route: heap_bytes is NULL");
    return route_columns(schema, host_splitters, shards, in, ops_in, n, out, ops_out, cap_rows, counts, starts, heap_bytes,
                         stream);
}
