// byte_window.hpp -- the byte-granular write pass shared by the snapshot encode (snap_encode.hip) and
// the ragged route (shard_route.hip): values of any length and any source alignment written to one
// contiguous span of an output.  The span is cut into windows of BW_WIN bytes on 16-byte boundaries
// of the output; a window is assembled in LDS at its final relative positions -- a part shorter than
// BW_DIRECT bytes by BW_GROUP lanes (bw_copy), a lane's loads all issued before its first LDS store
// -- and then streamed out by the caller as aligned 16-byte stores.  A part of BW_DIRECT bytes or
// more does not pass the LDS: the whole wave copies its whole 16-byte granules from the source
// straight to the output, 4 KiB a step (bw_direct), and marks them in a bitmap so that the stream-out
// leaves them alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rh {

constexpr uint32_t BW_WIN = 32768;   // bytes of one LDS window (a multiple of 512)
constexpr uint32_t BW_DIRECT = 256;  // a part of a window of at least this many bytes skips the LDS
constexpr uint32_t BW_GROUP = 8;     // lanes that copy one shorter part: a wave works on 64 / BW_GROUP parts at a time
constexpr uint32_t BW_BATCH = BW_DIRECT / 4 / BW_GROUP;  // words per lane that cover such a part
constexpr uint32_t BW_LDS = BW_WIN + BW_WIN / 16 / 8;    // the window, and a bit per 16-byte granule of it

__device__ inline uint64_t bw_shfl64(uint64_t v, int k) {
    return ((uint64_t)__shfl((uint32_t)(v >> 32), k) << 32) | __shfl((uint32_t)v, k);
}

// src[0 .. N) to win[R .. R + N) (inside the window, N < BW_DIRECT), by BW_GROUP lanes (sub: the
// lane's number among them).  The whole words of the window inside the range are each one load
// from the source, at whatever alignment that has there, and one LDS store -- a lane's loads all
// issued before its first store, so a part costs one memory latency, not one per step; the at most
// 3 bytes before and behind them go byte by byte.  Every read lies inside src[0 .. N).
__device__ inline void bw_copy(const uint8_t *src, uint8_t *win, uint32_t R, uint32_t N, uint32_t sub) {
    const uint32_t pre = (4u - (R & 3u)) & 3u, head = pre < N ? pre : N;
    const uint32_t nw = (N - head) >> 2, tail = N - head - 4 * nw;  // nw < BW_BATCH * BW_GROUP
    uint32_t *dst = reinterpret_cast<uint32_t *>(win + R + head);
    uint32_t v[BW_BATCH];
#pragma unroll
    for (uint32_t u = 0; u < BW_BATCH; u++) {
        const uint32_t j = sub + u * BW_GROUP;
        v[u] = 0;
        if (j < nw) __builtin_memcpy(&v[u], src + head + 4 * j, 4);
    }
#pragma unroll
    for (uint32_t u = 0; u < BW_BATCH; u++) {
        const uint32_t j = sub + u * BW_GROUP;
        if (j < nw) dst[j] = v[u];
    }
    static_assert(BW_GROUP >= 3, "one lane per edge byte");
    if (sub < head) win[R + sub] = src[sub];
    if (sub < tail) win[R + head + 4 * nw + sub] = src[head + 4 * nw + sub];
}

// A long part (N >= BW_DIRECT), by the whole wave, straight to the output: its whole 16-byte
// granules are loaded from the source at whatever alignment it has and stored aligned -- 16 bytes a
// lane, four granules a lane in flight, 4 KiB a step -- and marked in `direct`; the at most 15 + 15
// bytes before and behind them take the window like a short part.  out_w: the output at the
// window's first byte (16-byte aligned); the part begins R bytes behind it.
__device__ inline void bw_direct(const uint8_t *src, uint8_t *win, uint32_t *direct, uint8_t *out_w, uint32_t R,
                                 uint32_t N, uint32_t lane) {
    const uint32_t head = (16u - (R & 15u)) & 15u;
    const uint32_t G = (N - head) / 16, tail = N - head - 16 * G, g0 = (R + head) / 16;
    const uint8_t *s = src + head;
    uint4 *dst = reinterpret_cast<uint4 *>(out_w) + g0;
    for (uint32_t g = lane; g < G; g += 256) {
        uint4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            v[u] = make_uint4(0, 0, 0, 0);
            if (g + 64 * u < G) __builtin_memcpy(&v[u], s + 16ull * (g + 64 * u), 16);
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t gg = g + 64 * u;
            if (gg < G) {
                dst[gg] = v[u];
                atomicOr(&direct[(g0 + gg) >> 5], 1u << ((g0 + gg) & 31));
            }
        }
    }
    if (lane < BW_GROUP) {
        if (head) bw_copy(src, win, R, head, lane);
        if (tail) bw_copy(src + head + 16ull * G, win, R + head + 16 * G, tail, lane);
    }
}

}  // namespace rh
