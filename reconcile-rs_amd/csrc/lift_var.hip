// lift_var.hip -- the variable-length-value lift (lift_var.hpp) instantiated for the store's key
// shapes and the unit key, and its launcher.
#include "internal.hpp"
#include "lift_var.hpp"

namespace rh {

namespace {

template <int KK, int KL, int RK, bool TAGS>
hipError_t launch_var(const VarCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums, hipStream_t st) {
    const uint64_t waves = (n + VAR_PER_WAVE - 1) / VAR_PER_WAVE;
    // multi-chunk messages first: the short kernel's block sums read their fingerprints
    hipLaunchKernelGGL((k_lift_var_long<KK, KL, RK, TAGS>), dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, c, n,
                       fps);
    hipLaunchKernelGGL((k_lift_var_short<KK, KL, RK, TAGS>), dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, st, c, n,
                       fps, c.dst ? nullptr : bsums);
    return hipGetLastError();
}

template <int KK, int KL>
hipError_t launch_var_key(int rk, bool tags, const VarCols &c, uint64_t n, uint8_t *fps, uint8_t *bsums,
                          hipStream_t st) {
    switch (rk) {
    case REC_PLAIN: return launch_var<KK, KL, REC_PLAIN, false>(c, n, fps, bsums, st);
    case REC_DATED:
        return tags ? launch_var<KK, KL, REC_DATED, true>(c, n, fps, bsums, st)
                    : launch_var<KK, KL, REC_DATED, false>(c, n, fps, bsums, st);
    case REC_PROJECTION:
        return tags ? launch_var<KK, KL, REC_PROJECTION, true>(c, n, fps, bsums, st)
                    : launch_var<KK, KL, REC_PROJECTION, false>(c, n, fps, bsums, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

bool var_key_supported(int kk, int kl) {
    return kk == KEY_UNIT || (kk == KEY_U32 && kl == 4) || (kk == KEY_U64 && kl == 8) ||
           (kk == KEY_BYTES && (kl == 16 || kl == 32));
}

hipError_t launch_lift_var(int kk, int kl, int rk, bool tags, const VarCols &c, uint64_t n, uint8_t *fps,
                           uint8_t *bsums, hipStream_t st, bool *supported) {
    *supported = var_key_supported(kk, kl);
    if (!*supported || n == 0) return hipSuccess;
    hipError_t e;
    if (kk == KEY_UNIT) e = launch_var_key<KEY_UNIT, 0>(rk, tags, c, n, fps, bsums, st);
    else if (kk == KEY_U32) e = launch_var_key<KEY_U32, 4>(rk, tags, c, n, fps, bsums, st);
    else if (kk == KEY_U64) e = launch_var_key<KEY_U64, 8>(rk, tags, c, n, fps, bsums, st);
    else if (kl == 16) e = launch_var_key<KEY_BYTES, 16>(rk, tags, c, n, fps, bsums, st);
    else e = launch_var_key<KEY_BYTES, 32>(rk, tags, c, n, fps, bsums, st);
    return e;
}

}  // namespace rh
