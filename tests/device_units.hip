// device_units.hip -- device-unit driver: the library's own device functions and launchers run on
// inputs a test chooses, where the public API only ever feeds them BLAKE3 outputs and spans of a
// few thousand rows.  Built by reconcile-rs_amd/Makefile from the library's headers with the
// library's flags (the same -O3 and no maths flags: round_decide's square root must lower as it
// does in the library) and linked against librsos_hip.so for the rh::launch_* entry points.
//
//   device_units <cases-file> <results-file>     every case once, in order (device_units_io.hpp)
//   device_units --constants                     the workgroup sizes the cases depend on, as JSON
//
// Each case calls the project's code and reimplements nothing: round_decide, fp_add / fp_sub, the
// carry-save helpers (acc_add_fp, acc_normalise, acc_wave_reduce, acc_block_reduce<NT>,
// block_sum_fps256), launch_reduce, launch_total, launch_range_query, launch_prefix,
// launch_row_prefix, launch_block_prefix.  The expected values are the test's (Python integers).
//
// Every HIP call's status is checked, and hipDeviceSynchronize after each case; at the first error
// the case's name is printed, nothing more is launched and the exit status is non-zero.  Every
// output buffer lies between guard bytes (0xA5), verified after the case; buffer sizes are checked
// against the case's counts before anything is launched.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include "../reconcile-rs_amd/csrc/fp_device.hpp"
#include "../reconcile-rs_amd/csrc/round_device.hpp"
#include "device_units_io.hpp"

namespace {

constexpr size_t GUARD = 64;  // keeps the 16-byte alignment the 128-bit stores need
const char *g_case = "(start)";

[[noreturn]] void die(int status, const char *what, const char *detail) {
    fprintf(stderr, "device_units: case %s: %s: %s\n", g_case, what, detail);
    fflush(stderr);
    _exit(status);  // no destructors, no further device work
}
#define HIPCHK(expr)                                          \
    do {                                                      \
        const hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) die(3, #expr, hipGetErrorString(e_)); \
    } while (0)
#define REQUIRE(cond) \
    do {              \
        if (!(cond)) die(2, "malformed case", #cond); \
    } while (0)

// ---- the kernels: thin callers of the library's device functions ---------------------------------
__global__ __launch_bounds__(256) void k_du_round(const uint64_t *rec, uint64_t cnt, uint64_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    const uint64_t *r = rec + 15 * i;
    const rh::RoundSeg g = rh::round_decide(r[0], r[1], r + 2, r + 7, r[12], (int)r[13], r[14]);
    uint64_t *o = out + 6 * i;
    o[0] = (uint64_t)g.kind, o[1] = g.stride, o[2] = g.si, o[3] = g.ei, o[4] = g.children, o[5] = g.enums;
}

// one segment [0, span) of a span-row store against a remote side of one element: the policy's stride
__global__ __launch_bounds__(256) void k_du_round_spans(const uint64_t *spans, uint64_t cnt, int sqrt_policy,
                                                        uint64_t b, uint64_t *stride, uint64_t *children,
                                                        uint8_t *kind) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    const uint64_t span = spans[i];
    const uint64_t L[5] = {1, 0, 0, 0, span}, R[5] = {0, 0, 0, 0, 1};
    const rh::RoundSeg g = rh::round_decide(0, span, L, R, span, sqrt_policy, b);
    stride[i] = g.stride, children[i] = g.children, kind[i] = (uint8_t)g.kind;
}

__global__ __launch_bounds__(256) void k_du_fp(const uint8_t *a, const uint8_t *b, uint64_t cnt, uint8_t *sum,
                                               uint8_t *diff) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    uint32_t x[8], y[8], o[8];
    rh::fp_load(a + 32 * i, x);
    rh::fp_load(b + 32 * i, y);
    rh::fp_add(x, y, o);
    rh::fp_store(sum + 32 * i, o);
    rh::fp_sub(x, y, o);
    rh::fp_store(diff + 32 * i, o);
}

__global__ __launch_bounds__(64) void k_du_acc_seq(const uint64_t *off, const uint8_t *fps, uint64_t cnt,
                                                   uint8_t *out) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= cnt) return;
    rh::Acc a;
    rh::acc_zero(a);
    for (uint64_t j = off[i]; j < off[i + 1]; j++) {
        uint32_t f[8];
        rh::load_fp(fps, j, f);
        rh::acc_add_fp(a, f);
    }
    uint32_t f[8];
    rh::acc_normalise(a, f);
    rh::store_sum(out, i, f);
}

// lane l of case c adds fingerprints [(64 c + l) m, (64 c + l + 1) m); every lane's total is kept
__global__ __launch_bounds__(64) void k_du_acc_wave(const uint8_t *fps, uint64_t m, uint8_t *out) {
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    rh::Acc a;
    rh::acc_zero(a);
    for (uint64_t j = 0; j < m; j++) {
        uint32_t f[8];
        rh::load_fp(fps, t * m + j, f);
        rh::acc_add_fp(a, f);
    }
    rh::acc_wave_reduce(a);
    uint32_t f[8];
    rh::acc_normalise(a, f);
    rh::store_sum(out, t, f);
}

template <int NT>
__global__ __launch_bounds__(NT) void k_du_acc_block(const uint8_t *fps, uint64_t m, uint8_t *out) {
    __shared__ uint64_t lds[(NT / 64) * 8];
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    rh::Acc a;
    rh::acc_zero(a);
    for (uint64_t j = 0; j < m; j++) {
        uint32_t f[8];
        rh::load_fp(fps, t * m + j, f);
        rh::acc_add_fp(a, f);
    }
    uint32_t f[8];
    rh::acc_block_reduce<NT>(a, lds, f);
    if (threadIdx.x == 0) rh::store_sum(out, blockIdx.x, f);
}

__global__ __launch_bounds__(256) void k_du_block_sum(const uint8_t *fps, uint8_t *out) {
    __shared__ rh::SumTile tile;
    uint32_t h[8], f[8];
    rh::load_fp(fps, (uint64_t)blockIdx.x * 256 + threadIdx.x, h);
    rh::block_sum_fps256(h, tile, f);
    if (threadIdx.x == 0) rh::store_sum(out, blockIdx.x, f);
}

// ---- buffers ---------------------------------------------------------------------------------
struct In {
    uint8_t *p = nullptr;
    size_t bytes = 0;
};
struct Out {
    uint8_t *base = nullptr;
    size_t bytes = 0;
    uint8_t *data() const { return base + GUARD; }
};

std::vector<void *> g_allocs;

In upload(const std::vector<uint8_t> &h) {
    In d;
    d.bytes = h.size();
    HIPCHK(hipMalloc((void **)&d.p, std::max<size_t>(h.size(), 64)));
    g_allocs.push_back(d.p);
    if (!h.empty()) HIPCHK(hipMemcpy(d.p, h.data(), h.size(), hipMemcpyHostToDevice));
    return d;
}

Out guarded(size_t bytes) {
    Out o;
    o.bytes = bytes;
    HIPCHK(hipMalloc((void **)&o.base, bytes + 2 * GUARD));
    g_allocs.push_back(o.base);
    HIPCHK(hipMemset(o.base, 0xA5, bytes + 2 * GUARD));
    return o;
}

void emit(du::Results &res, const char *what, const Out &o) {
    std::vector<uint8_t> h(o.bytes + 2 * GUARD);
    HIPCHK(hipMemcpy(h.data(), o.base, h.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < GUARD; i++)
        if (h[i] != 0xA5 || h[GUARD + o.bytes + i] != 0xA5) die(4, what, "guard bytes overwritten");
    if (!res.put(g_case, what, h.data() + GUARD, o.bytes)) die(5, what, "cannot write the results file");
}

void free_all() {
    for (void *p : g_allocs) HIPCHK(hipFree(p));
    g_allocs.clear();
}

uint32_t grid_of(uint64_t n, uint64_t per) {
    const uint64_t g = (n + per - 1) / per;
    if (g == 0 || g > (1u << 24)) die(2, "malformed case", "grid size");
    return (uint32_t)g;
}

void run_case(const du::Cases &cs, const du::Case &c, du::Results &res) {
    auto host = [&](int k) -> const std::vector<uint8_t> & {
        if (c.buf[k] < 0) die(2, "malformed case", "missing buffer");
        return cs.bufs[(size_t)c.buf[k]];
    };
    auto has = [&](int k) { return c.buf[k] >= 0; };
    const uint64_t a0 = c.arg[0], a1 = c.arg[1], a2 = c.arg[2], a3 = c.arg[3];
    switch (c.op) {
        case du::OP_ROUND: {
            REQUIRE(a0 > 0 && host(0).size() == a0 * 15 * 8);
            const In rec = upload(host(0));
            const Out out = guarded(a0 * 6 * 8);
            hipLaunchKernelGGL(k_du_round, dim3(grid_of(a0, 256)), dim3(256), 0, 0, (const uint64_t *)rec.p, a0,
                               (uint64_t *)out.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_ROUND_SPANS: {
            REQUIRE(a0 > 0 && host(0).size() == a0 * 8 && a1 <= 1);
            const In sp = upload(host(0));
            const Out st = guarded(a0 * 8), ch = guarded(a0 * 8), kd = guarded(a0);
            hipLaunchKernelGGL(k_du_round_spans, dim3(grid_of(a0, 256)), dim3(256), 0, 0, (const uint64_t *)sp.p, a0,
                               (int)a1, a2, (uint64_t *)st.data(), (uint64_t *)ch.data(), kd.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "stride", st);
            emit(res, "children", ch);
            emit(res, "kind", kd);
            break;
        }
        case du::OP_FP_ADDSUB: {
            REQUIRE(a0 > 0 && host(0).size() == a0 * 32 && host(1).size() == a0 * 32);
            const In a = upload(host(0)), b = upload(host(1));
            const Out sum = guarded(a0 * 32), diff = guarded(a0 * 32);
            hipLaunchKernelGGL(k_du_fp, dim3(grid_of(a0, 256)), dim3(256), 0, 0, a.p, b.p, a0, sum.data(), diff.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "add", sum);
            emit(res, "sub", diff);
            break;
        }
        case du::OP_ACC_SEQ: {
            REQUIRE(a0 > 0 && host(0).size() == (a0 + 1) * 8 && host(1).size() % 32 == 0);
            const uint64_t *off = (const uint64_t *)host(0).data();
            for (uint64_t i = 0; i < a0; i++) REQUIRE(off[i] <= off[i + 1]);
            REQUIRE(off[a0] * 32 <= host(1).size());
            const In o = upload(host(0)), f = upload(host(1));
            const Out out = guarded(a0 * 32);
            hipLaunchKernelGGL(k_du_acc_seq, dim3(grid_of(a0, 64)), dim3(64), 0, 0, (const uint64_t *)o.p, f.p, a0,
                               out.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_ACC_WAVE: {
            REQUIRE(a0 > 0 && a1 < 4096 && host(0).size() == a0 * 64 * a1 * 32);
            const In f = upload(host(0));
            const Out out = guarded(a0 * 64 * 32);
            hipLaunchKernelGGL(k_du_acc_wave, dim3(grid_of(a0, 1)), dim3(64), 0, 0, f.p, a1, out.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_ACC_BLOCK: {  // a2: 0 = 256 (k_total, k_range_query), 1 = DB_WG, 2 = DP_WG
            const uint64_t nt = a2 == 0 ? 256 : a2 == 1 ? (uint64_t)rh::DB_WG : (uint64_t)rh::DP_WG;
            REQUIRE(a0 > 0 && a1 < 4096 && a2 <= 2 && host(0).size() == a0 * nt * a1 * 32);
            const In f = upload(host(0));
            const Out out = guarded(a0 * 32);
            if (a2 == 0)
                hipLaunchKernelGGL(k_du_acc_block<256>, dim3(grid_of(a0, 1)), dim3(256), 0, 0, f.p, a1, out.data());
            else if (a2 == 1)
                hipLaunchKernelGGL(k_du_acc_block<rh::DB_WG>, dim3(grid_of(a0, 1)), dim3(rh::DB_WG), 0, 0, f.p, a1,
                                   out.data());
            else
                hipLaunchKernelGGL(k_du_acc_block<rh::DP_WG>, dim3(grid_of(a0, 1)), dim3(rh::DP_WG), 0, 0, f.p, a1,
                                   out.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_BLOCK_SUM: {
            REQUIRE(a0 > 0 && host(0).size() == a0 * 256 * 32);
            const In f = upload(host(0));
            const Out out = guarded(a0 * 32);
            hipLaunchKernelGGL(k_du_block_sum, dim3(grid_of(a0, 1)), dim3(256), 0, 0, f.p, out.data());
            HIPCHK(hipGetLastError());
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_REDUCE: {
            REQUIRE((a1 == 32 || a1 == 40) && host(0).size() == a0 * a1);
            const In f = upload(host(0));
            const Out out = guarded((a0 + 255) / 256 * 32);
            HIPCHK(rh::launch_reduce(f.p, a0, out.data(), 0, (uint32_t)a1));
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_TOTAL: {
            REQUIRE(host(0).size() == a0 * 32);
            const In f = upload(host(0));
            const Out out = guarded(32);
            HIPCHK(rh::launch_total(f.p, a0, (uint64_t *)out.data(), 0));
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_RANGE: {  // a0 n, a1 stride, a2 r, a3 records in buf0 (>= n; slots index them)
            const uint64_t n = a0, nbk = (n + 255) / 256, ns = (nbk + 255) / 256;
            REQUIRE((a1 == 32 || a1 == 40) && a2 > 0 && a2 <= 4096 && a3 >= n && host(0).size() == a3 * a1);
            REQUIRE(host(4).size() == a2 * 8 && host(5).size() == a2 * 8);
            if (has(1)) {
                REQUIRE(host(1).size() == n * 4);
                const uint32_t *s = (const uint32_t *)host(1).data();
                for (uint64_t i = 0; i < n; i++) REQUIRE(s[i] < a3);
            } else {
                REQUIRE(a3 == n);
            }
            if (has(2)) REQUIRE(host(2).size() == nbk * 32);
            if (has(3)) REQUIRE(host(3).size() == ns * 32);
            const In f = upload(host(0)), lo = upload(host(4)), hi = upload(host(5));
            const In sl = has(1) ? upload(host(1)) : In{}, bs = has(2) ? upload(host(2)) : In{},
                     ss = has(3) ? upload(host(3)) : In{};
            const Out out = guarded(a2 * 40);
            HIPCHK(rh::launch_range_query(f.p, bs.p, ss.p, n, (const uint64_t *)lo.p, (const uint64_t *)hi.p, a2,
                                          (uint64_t *)out.data(), 0, (uint32_t)a1, (const uint32_t *)sl.p));
            HIPCHK(hipDeviceSynchronize());
            emit(res, "out", out);
            break;
        }
        case du::OP_PREFIX: {  // a0 n, a1 max_wgs, a2: also launch_row_prefix from the bpre just formed
            const uint64_t n = a0, nbk = (n + 255) / 256, ns = (nbk + 255) / 256;
            REQUIRE(n < (1u << 24) && a1 <= 1024 && host(0).size() == n * 32 && host(1).size() == nbk * 32 &&
                    host(2).size() == ns * 32);
            const In f = upload(host(0)), bs = upload(host(1)), ss = upload(host(2));
            const Out spre = guarded((ns + 1) * 32), bpre = guarded((nbk + 1) * 32), out = guarded((n + 1) * 32);
            HIPCHK(rh::launch_prefix(f.p, n, bs.p, ss.p, spre.data(), bpre.data(), out.data(), 0, (uint32_t)a1));
            HIPCHK(hipDeviceSynchronize());
            emit(res, "spre", spre);
            emit(res, "bpre", bpre);
            emit(res, "out", out);
            if (a2) {
                const Out row = guarded((n + 1) * 32);
                HIPCHK(rh::launch_row_prefix(f.p, n, bpre.data(), row.data(), 0));
                HIPCHK(hipDeviceSynchronize());
                emit(res, "row", row);
            }
            break;
        }
        case du::OP_BLOCK_PREFIX: {
            const uint64_t n = a0, nbk = (n + 255) / 256, ns = (nbk + 255) / 256;
            REQUIRE(n < (1ull << 31) && host(0).size() == nbk * 32 && host(1).size() == ns * 32);
            const In bs = upload(host(0)), ss = upload(host(1));
            const Out spre = guarded((ns + 1) * 32), bpre = guarded((nbk + 1) * 32);
            HIPCHK(rh::launch_block_prefix(n, bs.p, ss.p, spre.data(), bpre.data(), 0));
            HIPCHK(hipDeviceSynchronize());
            emit(res, "spre", spre);
            emit(res, "bpre", bpre);
            break;
        }
        default:
            die(2, "malformed case", "unknown op");
    }
    free_all();
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "--constants")) {  // no device call
        printf("{\"DB_WG\": %d, \"DP_WG\": %d, \"guard\": %zu}\n", rh::DB_WG, rh::DP_WG, GUARD);
        return 0;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: device_units <cases-file> <results-file> | device_units --constants\n");
        return 2;
    }
    du::Cases cs;
    std::string why;
    if (!du::load_cases(argv[1], cs, why)) {
        fprintf(stderr, "device_units: %s\n", why.c_str());
        return 2;
    }
    du::Results res;
    if (!res.open(argv[2])) {
        fprintf(stderr, "device_units: cannot write %s\n", argv[2]);
        return 2;
    }
    for (const du::Case &c : cs.cases) {
        g_case = c.name;
        run_case(cs, c, res);
    }
    if (!res.close()) {
        fprintf(stderr, "device_units: cannot finish %s\n", argv[2]);
        return 5;
    }
    printf("device_units: %zu cases ok\n", cs.cases.size());
    return 0;
}
