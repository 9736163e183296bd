"""Generates valu_rule.hip: what turns gfx950's 2.2-cycle VALU issue into the ~3.9 of a BLAKE3 G stream.

Follows valu_g.py (profiles/r02_micro_valu_g.log), with everything that log left unequal held equal:
every kernel clobbers v8-v63 (64 VGPRs, so 8 waves per SIMD fit), every launch is exactly one
residency round (CUs x workgroups-per-CU blocks), and occupancy is lowered with a dynamic LDS
allocation only, so the instruction stream of a kernel is the same at 2, 4 and 8 waves per SIMD.
Each row prints the VGPR count, the waves per SIMD asked for and the waves per SIMD seen (HW_ID of
every wave), the event-timed cycles per wave-instruction, and the mean wave lifetime (s_memtime) per
instruction and resident wave: that one falls below the event figure where a SIMD's waves ran one
after another (the oldest wave is served first) and not side by side.

  occ    g_cur / g_split / g_simple / g_skew / g_prio with 1, 2, 4, 8 chains at 8, 4, 2 waves per SIMD
         (g_prio: g_cur with s_setprio 1 over every run of half-rate instructions, 0 over the others)
  prov   v_xor, v_add_u32, v_alignbit, v_add3: in place or a new destination, sources never written
         or written k = 1, 2, 4, 8, 16 instructions earlier; v_xor / v_add_u32 with both sources written
         k and k + 1 earlier; mixfast: g_simple's five full-rate opcodes in turn with no dependences
  rl     r slow (v_alignbit) then r fast (v_xor), r = 1 .. 64: free-running, an s_barrier after every
         run, s_setprio raised in the fast runs, s_setprio raised in the slow runs
  split  k of the 8 wave slots of every SIMD on the fast stream, the others on the slow one

The generated source (~700 KB) is not kept in the repository:
  python3 microbench/valu_rule.py > microbench/valu_rule.hip
  hipcc -O3 -Wno-unused-result --offload-arch=gfx950 microbench/valu_rule.hip -o microbench/valu_rule
"""

LO, HI = 8, 64
REGS = list(range(LO, HI))
CONST = [56, 57, 58, 59, 60, 61, 62, 63]  # never written after the init
RING = list(range(8, 40))                 # 32 registers written in turn
BODY = 128


# ---- G encodings: chain j state a..d = v(8+4j)..; 8 message words v40-v47 shared; temps v48+j ----
def regs(j):
    return tuple(8 + 4 * j + k for k in range(4)) + (40 + (2 * j) % 8, 40 + (2 * j + 1) % 8, 48 + j)


def g_cur(j):
    a, b, c, d, m0, m1, t = regs(j)
    return [f"v_add3_u32 v{a}, v{a}, v{b}, v{m0}", f"v_xor_b32 v{d}, v{d}, v{a}", f"v_alignbit_b32 v{d}, v{d}, v{d}, 16",
            f"v_add_u32 v{c}, v{c}, v{d}", f"v_xor_b32 v{b}, v{b}, v{c}", f"v_alignbit_b32 v{b}, v{b}, v{b}, 12",
            f"v_add3_u32 v{a}, v{a}, v{b}, v{m1}", f"v_xor_b32 v{d}, v{d}, v{a}", f"v_alignbit_b32 v{d}, v{d}, v{d}, 8",
            f"v_add_u32 v{c}, v{c}, v{d}", f"v_xor_b32 v{b}, v{b}, v{c}", f"v_alignbit_b32 v{b}, v{b}, v{b}, 7"]


def g_split(j):
    a, b, c, d, m0, m1, t = regs(j)
    return [f"v_add_u32 v{a}, v{a}, v{m0}", f"v_add_u32 v{a}, v{a}, v{b}", f"v_xor_b32 v{d}, v{d}, v{a}",
            f"v_alignbit_b32 v{d}, v{d}, v{d}, 16", f"v_add_u32 v{c}, v{c}, v{d}", f"v_xor_b32 v{b}, v{b}, v{c}",
            f"v_alignbit_b32 v{b}, v{b}, v{b}, 12", f"v_add_u32 v{a}, v{a}, v{m1}", f"v_add_u32 v{a}, v{a}, v{b}",
            f"v_xor_b32 v{d}, v{d}, v{a}", f"v_alignbit_b32 v{d}, v{d}, v{d}, 8", f"v_add_u32 v{c}, v{c}, v{d}",
            f"v_xor_b32 v{b}, v{b}, v{c}", f"v_alignbit_b32 v{b}, v{b}, v{b}, 7"]


def rot_simple(x, n, t):
    return [f"v_lshlrev_b32 v{t}, {32 - n}, v{x}", f"v_lshrrev_b32 v{x}, {n}, v{x}", f"v_or_b32 v{x}, v{x}, v{t}"]


def g_simple(j):
    a, b, c, d, m0, m1, t = regs(j)
    return ([f"v_add_u32 v{a}, v{a}, v{m0}", f"v_add_u32 v{a}, v{a}, v{b}", f"v_xor_b32 v{d}, v{d}, v{a}"] +
            rot_simple(d, 16, t) + [f"v_add_u32 v{c}, v{c}, v{d}", f"v_xor_b32 v{b}, v{b}, v{c}"] + rot_simple(b, 12, t) +
            [f"v_add_u32 v{a}, v{a}, v{m1}", f"v_add_u32 v{a}, v{a}, v{b}", f"v_xor_b32 v{d}, v{d}, v{a}"] +
            rot_simple(d, 8, t) + [f"v_add_u32 v{c}, v{c}, v{d}", f"v_xor_b32 v{b}, v{b}, v{c}"] + rot_simple(b, 7, t))


def interleave(chains):
    out = []
    for k in range(max(len(c) for c in chains)):
        for c in chains:
            if k < len(c):
                out.append(c[k])
    return out


def g_body(kind, nch):
    if kind == "skew":  # g_cur with chain j started 3j steps into its G: every slot mixes the classes
        chains = []
        for j in range(nch):
            g = g_cur(j) * 2
            s = (3 * j) % 12
            chains.append(g[s:] + g[:s])
        return interleave(chains), 2 * nch
    g = {"cur": g_cur, "split": g_split, "simple": g_simple, "prio": g_cur}[kind]
    reps = max(1, 4 // nch)  # keep the loop body long enough that the loop branch does not count
    lines = interleave([g(j) for j in range(nch)]) * reps
    if kind == "prio":  # g_cur with s_setprio raised over every run of half-rate instructions
        out, cur = [], None
        for ln in lines:
            slow = ln.startswith(("v_add3", "v_alignbit"))
            if slow != cur:
                out.append("s_setprio 1" if slow else "s_setprio 0")
                cur = slow
            out.append(ln)
        lines = out
    return lines, nch * reps


# ---- operand provenance: instruction i writes RING[i % 32] -------------------------------------------
def prov_line(op, i, mode, k):
    d = RING[i % 32]
    c0, c1, c2 = CONST[i % 4], CONST[4 + i % 4], CONST[(i + 1) % 4]
    prev = RING[(i - k) % 32] if k else c1
    if mode == "both":  # both sources written k and k + 1 instructions earlier, a third destination
        return f"{op} v{d}, v{RING[(i - k - 1) % 32]}, v{prev}"
    if op in ("v_xor_b32", "v_add_u32"):
        return f"{op} v{d}, v{d}, v{prev}" if mode == "inplace" else f"{op} v{d}, v{c0}, v{prev}"
    if op == "v_alignbit_b32":
        return f"{op} v{d}, v{d}, v{prev}, 7" if mode == "inplace" else f"{op} v{d}, v{c0}, v{prev}, 7"
    return f"{op} v{d}, v{d}, v{prev}, v{c2}" if mode == "inplace" else f"{op} v{d}, v{c0}, v{prev}, v{c2}"


# ---- class-run length: r x v_alignbit then r x v_xor over 16 accumulators ----------------------------
def rl_body(r, variant):
    out, i = [], 0
    for _ in range(BODY // (2 * r)):
        for cls in ("slow", "fast"):
            if variant == "prio_fast":
                out.append("s_setprio 3" if cls == "fast" else "s_setprio 0")
            if variant == "prio_slow":
                out.append("s_setprio 3" if cls == "slow" else "s_setprio 0")
            for _ in range(r):
                d = 8 + i % 16
                out.append(f"v_alignbit_b32 v{d}, v{d}, v{d}, 7" if cls == "slow" else f"v_xor_b32 v{d}, v{d}, v{CONST[i % 8]}")
                i += 1
            if variant == "bar":
                out.append("s_barrier")
    return out


def stream(cls):
    return [f"v_alignbit_b32 v{8 + i % 16}, v{8 + i % 16}, v{8 + i % 16}, 7" if cls == "slow" else
            f"v_xor_b32 v{8 + i % 16}, v{8 + i % 16}, v{CONST[i % 8]}" for i in range(BODY)]


HEAD = r'''// generated by valu_rule.py -- do not edit
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <map>
#include <vector>
typedef void (*KF)(uint32_t *, int, uint64_t *, uint32_t *, int);
'''

CLOB = ", ".join(f'"v{r}"' for r in REGS)
INIT = "".join(f'"v_mov_b32 v{r}, %0\\n"' for r in REGS)


def kernel(name, lines, lines_b=None, select="slot"):
    asm = "\\n".join(lines)
    loop = f'for (int i = 0; i < iters; i++) asm volatile("{asm}" ::: {CLOB});'
    if lines_b is not None:
        asm_b = "\\n".join(lines_b)
        cond = "(hwid & 15u) < (uint32_t)ksplit" if select == "slot" else "!((threadIdx.x >> 6) & 1)"
        loop = (f'if ({cond}) {{ {loop} }}\n'
                f'  else {{ for (int i = 0; i < iters; i++) asm volatile("{asm_b}" ::: {CLOB}); }}')
    return f'''__global__ __launch_bounds__(1024) void k_{name}(uint32_t *out, int iters, uint64_t *clk, uint32_t *hw, int ksplit) {{
  const uint32_t hwid = __builtin_amdgcn_s_getreg(63492), xcc = __builtin_amdgcn_s_getreg(63508);  // HW_ID, XCC_ID
  asm volatile({INIT} :: "v"(threadIdx.x * 2654435761u + 12345u) : {CLOB});
  uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  {loop}
  uint32_t r; asm volatile("v_xor_b32 %0, v8, v9" : "=v"(r));
  uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
  if ((threadIdx.x & 63) == 0) {{ clk[2 * w] = t1 - t0; clk[2 * w + 1] = r1 - r0; hw[2 * w] = hwid; hw[2 * w + 1] = xcc; }}
}}
'''


MAIN = r'''
static int ncu;
static uint32_t *out, *hw; static uint64_t *clk;
// one residency round: ncu x wgs workgroups of nt threads; wgs per CU enforced by dynamic LDS only
void run(const char *name, KF f, int nt, int wgs, int iters, int per_iter, int gs, int ksplit) {
    const int wps = wgs * nt / 256, blocks = ncu * wgs, waves = blocks * nt / 64;
    const size_t lds = wps == 8 ? 0 : (size_t)(160 / wgs - 1) * 1024;
    hipFuncAttributes fa; hipFuncGetAttributes(&fa, (const void *)f);
    if (hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        printf("%-22s skipped: %zu B of LDS refused\n", name, lds); (void)hipGetLastError(); return;
    }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(f, dim3(blocks), dim3(nt), lds, 0, out, 4, clk, hw, ksplit);
    hipEventRecord(e0);
    const int reps = 3;
    for (int r = 0; r < reps; r++) hipLaunchKernelGGL(f, dim3(blocks), dim3(nt), lds, 0, out, iters, clk, hw, ksplit);
    hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) { printf("%-22s failed: %s\n", name, hipGetErrorString(hipGetLastError())); exit(1); }
    float ms; hipEventElapsedTime(&ms, e0, e1);
    std::vector<uint64_t> c(2 * waves); std::vector<uint32_t> h(2 * waves);
    hipMemcpy(c.data(), clk, 16 * waves, hipMemcpyDeviceToHost); hipMemcpy(h.data(), hw, 8 * waves, hipMemcpyDeviceToHost);
    double sc = 0, sr = 0, cyc[2] = {0, 0}; int cnt[2] = {0, 0};
    std::map<uint32_t, int> per_simd, fast_simd;
    for (int w = 0; w < waves; w++) {
        sc += (double)c[2 * w]; sr += (double)c[2 * w + 1];
        const uint32_t id = h[2 * w], key = ((h[2 * w + 1] & 15u) << 16) | (((id >> 8) & 0xffu) << 2) | ((id >> 4) & 3u);
        const int fast = ksplit >= 0 ? (int)(id & 15u) < ksplit : !((w % (nt / 64)) & 1);
        per_simd[key]++; fast_simd[key] += fast;
        cyc[fast] += (double)c[2 * w]; cnt[fast]++;
    }
    int lo = 1 << 30, hi = 0, flo = 1 << 30, fhi = 0;
    for (auto &kv : per_simd) { lo = kv.second < lo ? kv.second : lo; hi = kv.second > hi ? kv.second : hi; }
    for (auto &kv : fast_simd) { flo = kv.second < flo ? kv.second : flo; fhi = kv.second > fhi ? kv.second : fhi; }
    const double ghz = sc / (sr / 100e6) / 1e9;
    const double wi = (double)reps * waves * (double)iters * per_iter;
    const double cpi = ghz * 1e9 / (wi / (ms / 1e3) / (4.0 * ncu));
    const double wcpi = sc / waves / ((double)iters * per_iter * wps);
    printf("%-22s vgpr %3d  w/simd %d (seen %d-%d on %zu)  %7.3f ms %.2f GHz  %5.2f cyc/instr (wave life %5.2f)",
           name, fa.numRegs, wps, lo, hi, per_simd.size(), ms / reps, ghz, cpi, wcpi);
    if (gs) printf("  %5.1f cyc/G", cpi * per_iter / gs);
    if (ksplit != 8 || lo != hi)
        if (cnt[0] && cnt[1])
            printf("  fast waves/simd %d-%d: fast %.2f slow %.2f wave-cyc/instr", flo, fhi,
                   cyc[1] / cnt[1] / ((double)iters * per_iter), cyc[0] / cnt[0] / ((double)iters * per_iter));
    printf("\n"); fflush(stdout);
    hipEventDestroy(e0); hipEventDestroy(e1);
}
int main() {
    hipDeviceProp_t p; hipGetDeviceProperties(&p, 0); ncu = p.multiProcessorCount;
    printf("%s, %d CUs\n", p.gcnArchName, ncu);
    hipMalloc(&out, (size_t)ncu * 2048 * 4); hipMalloc(&clk, (size_t)ncu * 32 * 16); hipMalloc(&hw, (size_t)ncu * 32 * 8);
    for (int k = 0; k < 20; k++) run("warm", k_prov_v_xor_b32_inplace_0, 256, 8, 1000, 128, 0, 8);
'''

GEOM_OCC = [(256, 8), (256, 4), (256, 2)]
GEOM_RL = [(256, 8), (1024, 2), (1024, 1), (512, 1)]


def main():
    out, runs = [HEAD], []
    # operand provenance
    for op in ("v_xor_b32", "v_add_u32", "v_alignbit_b32", "v_add3_u32"):
        for mode in ("inplace", "newdst"):
            for k in (0, 1, 2, 4, 8, 16):
                name = f"prov_{op}_{mode}_{k}"
                out.append(kernel(name, [prov_line(op, i, mode, k) for i in range(BODY)]))
                runs.append((name, 256, 8, 1000, BODY, 0, 8))
    for op in ("v_xor_b32", "v_add_u32"):
        for k in (1, 2, 4, 8):
            name = f"prov_{op}_both_{k}"
            out.append(kernel(name, [prov_line(op, i, "both", k) for i in range(BODY)]))
            runs.append((name, 256, 8, 1000, BODY, 0, 8))
    # the five full-rate opcodes of g_simple in turn, in place, sources never written: opcode variety alone
    fast5 = ["v_add_u32 v{d}, v{d}, v{c}", "v_xor_b32 v{d}, v{d}, v{c}", "v_lshlrev_b32 v{d}, 16, v{d}",
             "v_lshrrev_b32 v{d}, 7, v{d}", "v_or_b32 v{d}, v{d}, v{c}"]
    out.append(kernel("mixfast", [fast5[i % 5].format(d=RING[i % 32], c=CONST[i % 8]) for i in range(BODY)]))
    runs.append(("mixfast", 256, 8, 1000, BODY, 0, 8))
    # whole G functions by occupancy
    for kind in ("cur", "split", "simple", "skew", "prio"):
        for nch in (1, 2, 4, 8):
            lines, gs = g_body(kind, nch)
            name = f"g_{kind}_{nch}"
            out.append(kernel(name, lines))
            for nt, wgs in GEOM_OCC:
                runs.append((name, nt, wgs, 400, sum(ln.startswith("v_") for ln in lines), gs, 8))
    # class-run length
    for variant in ("free", "bar", "prio_fast", "prio_slow"):
        for r in (1, 2, 4, 8, 16, 32, 64):
            name = f"rl_{variant}_{r}"
            out.append(kernel(name, rl_body(r, variant)))
            for nt, wgs in GEOM_RL:
                runs.append((name, nt, wgs, 1000, BODY, 0, 8))
    # cross-wave overlap: k of the 8 wave slots of every SIMD on the fast stream
    out.append(kernel("split_slot", stream("fast"), stream("slow")))
    for k in (0, 2, 4, 6, 8):
        runs.append(("split_slot", 256, 8, 1000, BODY, 0, k))
    out.append(kernel("split_parity", stream("fast"), stream("slow"), select="parity"))  # r02's split_xor_align
    runs.append(("split_parity", 256, 8, 1000, BODY, 0, -1))
    out.append(MAIN)
    for n, nt, wgs, it, per, gs, ks in runs:
        tag = n if (nt, wgs) == (256, 8) and ks in (8, -1) else f"{n}" + (f"/k{ks}" if ks not in (8, -1) else f"/{nt}x{wgs}")
        out.append(f'    run("{tag}", k_{n}, {nt}, {wgs}, {it}, {per}, {gs}, {ks});\n')
    out.append("    return 0;\n}\n")
    print("".join(out))


if __name__ == "__main__":
    main()
