// enum_tiny.hpp -- Enumerate for a handful of key ranges (r <= ROUND_TINY_SEGS, at most
// ENUM_TINY_ROWS rows in all) in ONE launch, over the base run and any pending delta run: the
// IDLIST ranges of a round under EnumerateBelowThreshold (rbsr/src/policy/enumerate_below_threshold.rs;
// Rsos::enumerate, rsos/src/rsos_trait.rs:73-83).
//
// One workgroup of 16 waves, in k_query_tiny's protocol: the ranges' kinds and bound keys come in
// from the kernel's arguments into LDS; the 2r bound keys are searched in the base run (its search
// table, then W-way probes) and in the delta run, a 16-lane group per (key, run), all at once; a
// lane per range forms its first view rank, row count and places (what k_enum_plan forms); wave 0
// scans the counts; a 16-lane group per output row finds where the row is read from (a base row,
// or the view's key by view_at_group); then a lane per 16-byte unit of the answer copies it into
// mapped page-locked memory in enum_layout().  First ranks, offsets and the total are always
// written; the rows only when the total is within a.limit (the host then takes the general path:
// enumerate_kernels.hip).  The sequence word is stored last, after a system-scope fence.
// Replaces, for such requests, a copy up, two searches, k_enum_plan, a scan, k_enum_emit and
// k_enum_copy_out.
#pragma once
#include "round_device.hpp"
#include "search_device.hpp"

namespace rh {

constexpr uint32_t ENUM_TINY_THREADS = 1024;
template <int KK, int KL>
__global__ __launch_bounds__(ENUM_TINY_THREADS) void k_enum_tiny(EnumTiny a) {
    constexpr uint32_t RT = ROUND_TINY_SEGS, NG = ENUM_TINY_THREADS / 16;
    static_assert(KL <= (int)ROUND_TINY_KL && KL % 4 == 0 && RT <= 64, "EnumTiny's inline keys; a wave scans the counts");
    __shared__ __align__(16) uint8_t keys[2 * RT * KL];
    __shared__ uint8_t sk[RT], ek[RT];
    __shared__ uint32_t rb[2 * RT], rj[2 * RT];
    __shared__ uint64_t first[RT], offs[RT + 1], place[4 * RT];
    __shared__ const uint8_t *src[ENUM_TINY_ROWS];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t grp = t >> 4, gl = t & 15;
    const uint32_t r = (uint32_t)a.r;
    const RoundRun &R = a.run;
    {
        const uint32_t nk = 2 * r * KL / 4;
        const uint32_t *in = reinterpret_cast<const uint32_t *>(a.ikeys);
        for (uint32_t i = t; i < nk; i += blockDim.x) reinterpret_cast<uint32_t *>(keys)[i] = in[i];
        if (t < r) sk[t] = a.isk[t], ek[t] = a.iek[t];
    }
    __syncthreads();
    // the bound keys' lower bounds, a 16-lane group per (key, run): jobs 0..2r-1 in the base run,
    // 2r..4r-1 in the delta run; key 2 j is range j's start, 2 j + 1 its end; an unbounded side is
    // not searched
    for (uint32_t job = grp; job < 4 * r; job += NG) {  // uniform per group
        const bool in_run = job >= 2 * r;
        const uint32_t q = in_run ? job - 2 * r : job;
        const bool bounded = (q & 1) ? ek[q >> 1] : sk[q >> 1];
        uint32_t rank = 0;
        if (bounded && !in_run) search_group<KK, KL, 16>(a.bkeys, R.nb, a.btab, keys + q * KL, gl, &rank, nullptr);
        if (bounded && in_run && R.n) search_group<KK, KL, 16>(R.keys, R.n, SearchTable{}, keys + q * KL, gl, &rank, nullptr);
        if (gl == 0) (in_run ? rj : rb)[q] = rank;
    }
    __syncthreads();
    // range j's first view rank, row count and places (k_enum_plan), a lane each; wave 0 scans the
    // counts into the offsets and writes the answer's header
    if (w == 0) {
        const bool mine = t < r;
        uint64_t l = 0, cnt = 0;
        if (mine) {
            const uint32_t j = t;
            const uint64_t bs = sk[j] ? rb[2 * j] : 0, be = ek[j] ? rb[2 * j + 1] : R.nb;
            const uint64_t js = (R.n && sk[j]) ? rj[2 * j] : 0, je = R.n ? (ek[j] ? rj[2 * j + 1] : R.n) : 0;
            uint64_t h = be;
            l = bs;
            if (R.n) {
                l = (uint64_t)((int64_t)bs + R.cntp[js]);
                h = (uint64_t)((int64_t)be + R.cntp[je]);
            }
            cnt = h > l ? h - l : 0;
            first[j] = l;
            place[4 * j] = bs, place[4 * j + 1] = js, place[4 * j + 2] = be, place[4 * j + 3] = je;
        }
        unsigned long long cs = cnt;  // inclusive scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long x = __shfl_up(cs, o);
            if (lane >= (uint32_t)o) cs += x;
        }
        const uint64_t total = __shfl(cs, 63);
        const EnumLayout L = enum_layout(r);
        uint64_t *of = reinterpret_cast<uint64_t *>(a.out + L.first), *oo = reinterpret_cast<uint64_t *>(a.out + L.offs);
        if (mine) {
            offs[t] = cs - cnt;
            of[t] = l;
            oo[t] = cs - cnt;
        }
        if (t == 0) offs[r] = total, oo[r] = total;
    }
    __syncthreads();
    const uint64_t total = offs[r];
    if (total <= a.limit && total <= ENUM_TINY_ROWS) {  // uniform
        // where output row i (of range j: offs[j] <= i < offs[j + 1]) is read from, a group per row:
        // base only, or a range no run entry falls in -- base row (start place + i - offs[j]); else
        // the view's key of rank first[j] + i - offs[j]
        for (uint32_t i = grp; i < (uint32_t)total; i += NG) {  // uniform per group
            uint32_t j = 0;
            while (j + 1 < r && offs[j + 1] <= i) j++;
            const uint64_t row = i - offs[j];
            // The base row's address first, for every lane, then replaced over the view.  Observed
            // with the if / else form (p assigned in each branch), AMD clang 22.0.0git roc-7.2.0,
            // -O3, gfx950: the first range with a run present and no run entry inside it faulted
            // (illegal address), and in that build's assembly the block that adds the row index to
            // the base pointer was reached on that path with the pointer's VGPR pair marked
            // implicit-def (set only on the run-less path and inside the view branch).  With this
            // form the address is complete before the branch; the cause inside the compiler was
            // not reduced further.
            const uint8_t *p = a.bkeys + (place[4 * j] + row) * KL;
            if (R.n != 0 && place[4 * j + 1] != place[4 * j + 3])
                p = view_at_group<16>(R, a.bkeys, KL, first[j] + row, gl).key;
            if (gl == 0) src[i] = p;
        }
        __syncthreads();
        // the rows, in whole 16-byte units (the last one zero-filled past the last row)
        const EnumLayout L = enum_layout(r);
        uint4 *o = reinterpret_cast<uint4 *>(a.out + L.keys);
        const uint32_t units = (uint32_t)((total * KL + 15) / 16);
        for (uint32_t u = t; u < units; u += blockDim.x) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if constexpr (KL >= 16) {
                constexpr uint32_t U = KL / 16;
                v = reinterpret_cast<const uint4 *>(src[u / U])[u % U];
            } else {
                constexpr uint32_t PER = 16 / KL, W = KL / 4;  // rows a unit, words a row
                uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
                for (uint32_t k = 0; k < PER; k++) {
                    const uint32_t i = u * PER + k;
                    if (i < (uint32_t)total) {
                        const uint32_t *s = reinterpret_cast<const uint32_t *>(src[i]);
#pragma unroll
                        for (uint32_t q = 0; q < W; q++) x[k * W + q] = s[q];
                    }
                }
                v = make_uint4(x[0], x[1], x[2], x[3]);
            }
            o[u] = v;
        }
    }
    // every thread's host-visible writes before the sequence word
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(a.seq_word, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace rh
