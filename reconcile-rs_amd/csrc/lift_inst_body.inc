// Body of one per-shape lift translation unit: instantiates the 7 kernels of a (key, value)
// shape (PLAIN; DATED and PROJECTION with/without tags; DATED+PROJECTION dual with/without
// tags) and its launcher, and the fused snapshot reload pass (snap_lift.hpp).  Included by
// lift_<shape>.hip after defining RH_NAME, RH_KK, RH_KL, RH_VK, RH_VL.
#include <hip/hip_ext.h>

#include <cstdlib>

#include "internal.hpp"
#include "lift_kernels.hpp"
#include "snap_lift.hpp"
#include "lift_search.hpp"
#include "small_batch.hpp"

#define RH_CAT2(a, b) a##b
#define RH_CAT(a, b) RH_CAT2(a, b)

namespace rh {

// k_lift in the form the launch asks for: Layout::SMALL shapes (the whole message in registers)
// have a second instantiation that compresses with compress_prio; streamed shapes have one form
template <int RK, bool T, bool D>
static void RH_CAT(lift_form_, RH_NAME)(bool prio, dim3 grid, dim3 block, hipStream_t st, const DevCols &c, uint64_t n,
                                        uint8_t *fps, uint8_t *bsums, uint8_t *fps2, uint8_t *bsums2) {
    if constexpr (Layout<RH_KK, RH_KL, RH_VK, RH_VL, RK>::SMALL) {
        if (prio) {
            hipLaunchKernelGGL((k_lift<RH_KK, RH_KL, RH_VK, RH_VL, RK, T, D, true>), grid, block, 0, st, c, n, fps, bsums,
                               fps2, bsums2);
            return;
        }
    }
    hipLaunchKernelGGL((k_lift<RH_KK, RH_KL, RH_VK, RH_VL, RK, T, D, false>), grid, block, 0, st, c, n, fps, bsums, fps2,
                       bsums2);
}

hipError_t RH_CAT(launch_lift_, RH_NAME)(int rk, bool tags, bool dual, const DevCols &c, uint64_t n,
                                         uint8_t *fps, uint8_t *bsums, uint8_t *fps2,
                                         uint8_t *bsums2, hipStream_t st) {
    static_assert(Layout<RH_KK, RH_KL, RH_VK, RH_VL, REC_DATED>::OK, "shape layout");
    if (n == 0) return hipSuccess;
    const uint64_t nblk = (n + LIFT_THREADS - 1) / LIFT_THREADS;
    const dim3 grid((uint32_t)nblk), block(LIFT_THREADS);
    // read at every launch, so one process can run both forms (RSOS_HIP_LIFT_PRIO=0: the plain compression)
    const char *form = getenv("RSOS_HIP_LIFT_PRIO");
    const bool prio = !(form && *form == '0');
#define RH_L(RK, T, D) RH_CAT(lift_form_, RH_NAME)<RK, T, D>(prio, grid, block, st, c, n, fps, bsums, fps2, bsums2)
    if (dual) {
        if (tags) RH_L(REC_DATED, true, true);
        else RH_L(REC_DATED, false, true);
    } else if (rk == REC_PLAIN) {
        RH_L(REC_PLAIN, false, false);
    } else if (rk == REC_DATED) {
        if (tags) RH_L(REC_DATED, true, false);
        else RH_L(REC_DATED, false, false);
    } else {
        if (tags) RH_L(REC_PROJECTION, true, false);
        else RH_L(REC_PROJECTION, false, false);
    }
#undef RH_L
    return hipGetLastError();
}

// the batch path's fused lift (into the sorted rows c.dst) + base / delta searches of the sorted
// keys q (lift_search.hpp); *supported = false for keyless shapes
// ev0 / ev1 (optional): events the launch itself stamps with the kernel's start and end
// (hipExtLaunchKernel: no marker packets around it, so timing it leaves no gaps on the stream)
hipError_t RH_CAT(launch_lift_search_, RH_NAME)(int rk, bool tags, const DevCols &c, uint64_t n, uint8_t *fps,
                                                const uint8_t *q, const SearchJob &jb, const SearchJob &jd,
                                                const NextMinmax &nx, hipStream_t st, bool *supported,
                                                hipEvent_t ev0, hipEvent_t ev1) {
    *supported = RH_KK != KEY_UNIT && c.dst != nullptr;
    if (!*supported || n == 0) return hipSuccess;
    if constexpr (RH_KK != KEY_UNIT) {
        const uint64_t nblk = (n + LIFT_THREADS - 1) / LIFT_THREADS;
        const uint64_t nmm = nx.keys && nx.part ? (nx.m + MINMAX_TILE - 1) / MINMAX_TILE : 0;
        const dim3 grid((uint32_t)(3 * nblk + nmm)), block(LIFT_THREADS);
#define RH_L(RK, T)                                                                                                   \
    do {                                                                                                              \
        if (ev0 || ev1)                                                                                               \
            hipExtLaunchKernelGGL((k_lift_search<RH_KK, RH_KL, RH_VK, RH_VL, RK, T>), grid, block, 0, st, ev0, ev1, 0, \
                                  c, n, fps, q, jb, jd, nmm ? nx : NextMinmax{});                                      \
        else                                                                                                          \
            hipLaunchKernelGGL((k_lift_search<RH_KK, RH_KL, RH_VK, RH_VL, RK, T>), grid, block, 0, st, c, n, fps, q,   \
                               jb, jd, nmm ? nx : NextMinmax{});                                                      \
    } while (0)
        if (rk == REC_PLAIN) {
            RH_L(REC_PLAIN, false);
        } else if (rk == REC_DATED) {
            if (tags) RH_L(REC_DATED, true);
            else RH_L(REC_DATED, false);
        } else {
            if (tags) RH_L(REC_PROJECTION, true);
            else RH_L(REC_PROJECTION, false);
        }
#undef RH_L
    }
    return hipGetLastError();
}

// the small-batch path's one-workgroup front (small_batch.hpp); *supported = false for keyless
// shapes and batches past small_batch_max
hipError_t RH_CAT(launch_small_batch_, RH_NAME)(int rk, bool tags, const SmallBatch &a, hipStream_t st,
                                                bool *supported) {
    *supported = RH_KK != KEY_UNIT && a.m <= small_batch_max(RH_KL);
    if (!*supported || a.m == 0) return hipSuccess;
    if constexpr (RH_KK != KEY_UNIT) {
        const dim3 grid(1), block(small_batch_threads(a.m));
#define RH_L(RK, T) hipLaunchKernelGGL((k_small_batch<RH_KK, RH_KL, RH_VK, RH_VL, RK, T>), grid, block, 0, st, a)
        if (rk == REC_PLAIN) {
            RH_L(REC_PLAIN, false);
        } else if (rk == REC_DATED) {
            if (tags) RH_L(REC_DATED, true);
            else RH_L(REC_DATED, false);
        } else {
            if (tags) RH_L(REC_PROJECTION, true);
            else RH_L(REC_PROJECTION, false);
        }
#undef RH_L
    }
    return hipGetLastError();
}

hipError_t RH_CAT(launch_snap_lift_, RH_NAME)(int mode, const SnapLift &a, uint64_t lds, hipStream_t st,
                                              bool *supported) {
    return launch_snap_lift_t<RH_KK, RH_KL, RH_VK, RH_VL>(mode, a, lds, st, supported);
}

}  // namespace rh
