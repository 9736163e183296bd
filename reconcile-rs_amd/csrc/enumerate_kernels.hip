// enumerate_kernels.hip -- Rsos::enumerate for many key ranges at once (rh_store_enumerate_segments):
// the keys of every IDLIST range a protocol round returns (rbsr/src/protocol.rs, enumeration_ranges;
// rsos/src/rsos_trait.rs:73-83), read from the base run and any delta run as they stand.
//
// After the bound keys' searches (the store's search_sampled over the base, search_run over the delta
// run), k_enum_plan turns each range's searched ranks into its first view rank, its row count and,
// over the view, its places (internal.hpp RoundRun); launch_exclusive_scan_u64 over the counts gives
// the row offsets and the total; k_enum_emit copies the keys, tiled over the output rows (not over the
// ranges: 10^4 ranges of 3 rows and one range of 10^6 rows fill the same tiles); k_enum_copy_out
// brings first ranks, offsets and rows down into mapped page-locked memory in one layout.
#include "round_device.hpp"
#include "store_kernels.hpp"

namespace rh {

namespace {

constexpr uint32_t ENUM_WG = 256, ENUM_UNROLL = 4;  // lanes a workgroup, 16-byte units a lane and tile
constexpr uint32_t ENUM_MAX_WGS = 2048;
// 8- and 16-byte units as the compiler's own vectors (an array of them stays in registers)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// range j < r: first = the view rank of its start bound (Unbounded: 0), cnt = max(end rank - first, 0),
// and over a delta run its places (start b, start j, end b, end j); cnt[r] = 0, so that the scan of
// r + 1 counts ends in the total.  rank_b / rank_j: row 2 j the start key's, 2 j + 1 the end key's.
__global__ __launch_bounds__(ENUM_WG) void k_enum_plan(const uint32_t *rank_b, const uint32_t *rank_j,
                                                       const uint8_t *sk, const uint8_t *ek, RoundRun R, uint64_t r,
                                                       uint64_t *first, uint64_t *cnt, uint64_t *place) {
    const uint64_t j = (uint64_t)blockIdx.x * ENUM_WG + threadIdx.x;
    if (j > r) return;
    if (j == r) {
        cnt[r] = 0;
        return;
    }
    const uint64_t bs = sk[j] ? rank_b[2 * j] : 0, be = ek[j] ? rank_b[2 * j + 1] : R.nb;
    uint64_t l = bs, h = be;
    if (R.n) {
        const uint64_t js = sk[j] ? rank_j[2 * j] : 0, je = ek[j] ? rank_j[2 * j + 1] : R.n;
        l = (uint64_t)((int64_t)bs + R.cntp[js]);
        h = (uint64_t)((int64_t)be + R.cntp[je]);
        place[4 * j] = bs;
        place[4 * j + 1] = js;
        place[4 * j + 2] = be;
        place[4 * j + 3] = je;
    }
    first[j] = l;
    cnt[j] = h > l ? h - l : 0;
}

// where output unit u (unit u % U of output row u / U, whose range lies in [ja, jz]) is read from
template <class V, uint32_t U>
__device__ __forceinline__ const V *enum_unit(const uint64_t *first, const uint64_t *offs, const uint64_t *place,
                                              const RoundRun &R, const uint8_t *bkeys, uint64_t ja, uint64_t jz,
                                              uint64_t u) {
    constexpr uint32_t kl = sizeof(V) * U;
    const uint64_t t = u / U;
    uint64_t a = ja + 1, z = jz + 1;  // j = the last range in [ja, jz] with offs[j] <= t
    while (a < z) {
        const uint64_t mid = (a + z) >> 1;
        if (offs[mid] <= t) a = mid + 1;
        else z = mid;
    }
    const uint64_t j = a - 1, row = t - offs[j];
    const uint8_t *src;
    if (R.n == 0) {
        src = bkeys + (first[j] + row) * kl;
    } else {
        const uint64_t *p = place + 4 * j;
        src = p[1] == p[3] ? bkeys + (p[0] + row) * kl : view_at(R, bkeys, kl, first[j] + row).key;
    }
    return reinterpret_cast<const V *>(src) + u % U;
}

// Output row t of range j (offs[j] <= t < offs[j + 1]) is view key first[j] + t - offs[j].  A row is
// U units of type V (4, 8 or 16 bytes; 64-byte rows: 4 x 16); a workgroup owns tiles of ENUM_WG *
// ENUM_UNROLL consecutive units, lane i of a pass unit i: whole lines read (contiguous base rows) and
// written.  The tile's first and last rows' ranges are found by binary search over offs (uniform), and
// each lane's row's range between them (for rows of few ranges, no step at all).  Base only, or a
// range no run entry falls in (its places' run indices are equal): base row first place + t - offs[j];
// else the view key by view_at, the select behind launch_select_view.  Nothing is written when the
// total exceeds `limit` rows (the caller then learns the total from offs[r] and decides).
template <class V, uint32_t U>
__global__ __launch_bounds__(ENUM_WG) void k_enum_emit(const uint64_t *first, const uint64_t *offs,
                                                       const uint64_t *place, uint64_t r, RoundRun R,
                                                       const uint8_t *bkeys, uint64_t limit, uint8_t *out) {
    const uint64_t total = offs[r];
    if (total > limit) return;
    constexpr uint64_t TILE = (uint64_t)ENUM_WG * ENUM_UNROLL;  // units
    const uint64_t units = total * U;
    V *o = reinterpret_cast<V *>(out);
    for (uint64_t u0 = (uint64_t)blockIdx.x * TILE; u0 < units; u0 += (uint64_t)gridDim.x * TILE) {
        const uint64_t u1 = u0 + TILE < units ? u0 + TILE : units;
        const uint64_t ja = round_owner(offs, r, u0 / U), jz = round_owner(offs, r, (u1 - 1) / U);
        const V *src[ENUM_UNROLL];  // every unit's address first, then the loads together, then the stores
#pragma unroll
        for (uint32_t k = 0; k < ENUM_UNROLL; k++) {
            const uint64_t u = u0 + k * ENUM_WG + threadIdx.x;
            src[k] = nullptr;
            if (u < u1) src[k] = enum_unit<V, U>(first, offs, place, R, bkeys, ja, jz, u);
        }
        V val[ENUM_UNROLL];
#pragma unroll
        for (uint32_t k = 0; k < ENUM_UNROLL; k++)
            if (src[k]) val[k] = *src[k];
#pragma unroll
        for (uint32_t k = 0; k < ENUM_UNROLL; k++)
            if (src[k]) o[u0 + k * ENUM_WG + threadIdx.x] = val[k];
    }
}

// first ranks and offsets (hdr: enum_layout's first L.keys bytes) and, unless the total exceeds
// `limit` rows, the rows, into dst (mapped page-locked memory, enum_layout): 16-byte stores, whole
// lines per wave, exactly the bytes the answer has (rounded up to 16; both sides have the slack)
__global__ __launch_bounds__(256) void k_enum_copy_out(const uint8_t *hdr, const uint8_t *keys, uint64_t r, uint32_t kl,
                                                       uint64_t limit, uint8_t *dst) {
    const EnumLayout L = enum_layout(r);
    const uint64_t total = reinterpret_cast<const uint64_t *>(hdr + L.offs)[r];
    const uint64_t nh = L.keys / 16, nk = total > limit ? 0 : (total * kl + 15) / 16;
    const uint4 *h = reinterpret_cast<const uint4 *>(hdr), *s = reinterpret_cast<const uint4 *>(keys);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nh + nk; i += stride)
        d[i] = i < nh ? h[i] : s[i - nh];
}

uint32_t enum_grid(uint64_t rows, uint32_t kl) {
    const uint64_t tile_bytes = (uint64_t)ENUM_WG * ENUM_UNROLL * (kl < 16 ? kl : 16);
    const uint64_t tiles = (rows * kl + tile_bytes - 1) / tile_bytes;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), ENUM_MAX_WGS);
}

}  // namespace

hipError_t launch_enum_plan(const uint32_t *rank_b, const uint32_t *rank_j, const uint8_t *sk, const uint8_t *ek,
                            const RoundRun &run, uint64_t r, uint64_t *first, uint64_t *cnt, uint64_t *place,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_enum_plan, dim3((uint32_t)((r + 1 + ENUM_WG - 1) / ENUM_WG)), dim3(ENUM_WG), 0, st, rank_b,
                       rank_j, sk, ek, run, r, first, cnt, place);
    return hipGetLastError();
}

hipError_t launch_enum_emit(const uint64_t *first, const uint64_t *offs, const uint64_t *place, uint64_t r,
                            const RoundRun &run, const uint8_t *bkeys, uint32_t kl, uint64_t limit, uint64_t rows,
                            uint8_t *out, hipStream_t st) {
    if (rows == 0) return hipSuccess;
    const dim3 grid(enum_grid(rows, kl)), wg(ENUM_WG);
    using Emit = void (*)(const uint64_t *, const uint64_t *, const uint64_t *, uint64_t, RoundRun, const uint8_t *,
                          uint64_t, uint8_t *);
    Emit k;
    switch (kl) {  // the widest unit the row is a whole number of
    case 4: k = k_enum_emit<uint32_t, 1>; break;
    case 8: k = k_enum_emit<u32x2, 1>; break;
    case 16: k = k_enum_emit<u32x4, 1>; break;
    case 32: k = k_enum_emit<u32x4, 2>; break;
    case 64: k = k_enum_emit<u32x4, 4>; break;
    default: return hipErrorInvalidValue;  // no store has such rows (store_key_ops)
    }
    hipLaunchKernelGGL(k, grid, wg, 0, st, first, offs, place, r, run, bkeys, limit, out);
    return hipGetLastError();
}

hipError_t launch_enum_copy_out(const uint8_t *hdr, const uint8_t *keys, uint64_t r, uint32_t kl, uint64_t limit,
                                uint64_t rows, uint8_t *dst, hipStream_t st) {
    const uint64_t n16 = (enum_layout(r).keys + rows * kl + 15) / 16;
    const uint32_t wgs = (uint32_t)std::min<uint64_t>((n16 + 255) / 256, 256);
    hipLaunchKernelGGL(k_enum_copy_out, dim3(wgs), dim3(256), 0, st, hdr, keys, r, kl, limit, dst);
    return hipGetLastError();
}

}  // namespace rh
