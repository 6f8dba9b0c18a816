// Split-half MFMA GEMM for gfx950:  out = post(act(alpha * A . W^T + bias) + residual)
//
// Both operands arrive as fp16 planes with K contiguous ("NT" form: activations [M][K], torch
// Linear weights [N][K]).  Workgroup tile (WM*64) x (WN*64), one wave per 64x64 sub-tile (4x4 MFMA
// 16x16x32 f16 tiles), BK = 32.  K-tiles stream through an NSTAGE-deep LDS ring filled by 16-byte
// global->LDS DMA (global_load_lds_dwordx4):
//   NSTAGE = 2: one tile ahead, __syncthreads() per K-tile (drains the DMA);
//   NSTAGE = 3: two tiles ahead, counted s_waitcnt vmcnt(N) + raw s_barrier so the newest tile's DMA
//               stays in flight across the barrier (guide §5 "Pipelining across barriers");
//   NSTAGE = 13, 14, 15: the same ring with 3, 4, 5 slots (small grids: latency of cold weights, not issue, bounds them).
// The LDS image is lane-linear (DMA constraint); bank conflicts of the ds_read_b128 fragment reads
// are removed by permuting the 16-byte chunks of each 64-byte row on the *source* address and
// applying the same involution on the read (guide §5.4 rule 21).
//
// The MFMA is issued "swapped" (A-operand = weight rows, B-operand = activation rows) so that each
// lane ends up with 4 consecutive output columns of one output row: the epilogue then stores
// 16-byte float4 / 8-byte half4 vectors instead of scalars.
//
// split == 3: acc += Whi.Ahi + Wlo.Ahi + Whi.Alo  (fp32 accumulate; ~2^-22 relative products)
// split == 1: acc += Whi.Ahi
//
// Which instantiation a call gets, on which grid and with which GemmParams, is decided in gemm_plan.h (plain host C++;
// cvlm_debug_gemm_plan below prints the decision without launching).  This file validates, plans and launches.
#include "gemm_kernel.h"
#include "gemm_plan.h"
using namespace cvlm_gemm_k;
using namespace cvlm_gemm_p;
CVLM_GEMM_IL_KERNELS(extern template)
static_assert(cvlm_gemm_p::BK_MIN == cvlm_gemm_k::BK_MIN && cvlm_gemm_p::SK_MAX_TILES == cvlm_gemm_k::SK_MAX_TILES, "the planner's copy of the kernel's limits");

extern "C" int64_t cvlm_gemm_workspace_bytes(void) { return (int64_t)(TAIL_FLAG_BYTES + TAIL_WS_BYTES); }

#ifdef CVLM_PROBES
static unsigned long long* g_trace = nullptr;
// Probe hook (not part of include/cvlm.h): device buffer of 8 x u64 per workgroup for CVLM_GEMM_VARIANT=47.
extern "C" void cvlm_debug_set_gemm_trace(void* buf) { g_trace = (unsigned long long*)buf; }
#endif

// CUs of the current device (the grid of the persistent kernels)
static int device_cus() {
    static int cus_[16] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int& cus = cus_[dev & 15];
    if (cus == 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    return cus;
}

template <auto... T>
static int launch(const GemmPlan& pl, const GemmParams& p, hipStream_t s) {
    constexpr int smem = gemm_lds_bytes(GemmKernel{T...});
    auto kern = gemm_nt_kernel<T...>;
    static bool attr[16] = {};
    if (smem > 48 * 1024 && cvlm_first_on_device(attr))
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    hipLaunchKernelGGL(kern, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), smem, s, p);
    CVLM_CHECK_LAUNCH();
    return 0;
}

// validate -> knobs -> plan: the launches of a call (their number, or a negative CVLM_E_* code)
template <class Cus>
static int plan_call(const cvlm_gemm_args& g, bool have_ws, Cus&& cus, GemmPlan plans[2]) {
    const int rc = gemm_validate(g);
    if (rc != 0) return rc;
    GemmKnobs kn = gemm_knobs();
#ifdef CVLM_PROBES
    kn.trace = g_trace != nullptr;
#endif
    return gemm_plan(g, kn, have_ws, cus, plans);
}

extern "C" int cvlm_gemm(const cvlm_gemm_args* args, void* stream) {
    if (!args) return CVLM_E_BADARG;
    const cvlm_gemm_args& g = *args;
    GemmPlan plans[2];
    const int n = plan_call(g, g.workspace && g.workspace_bytes >= cvlm_gemm_workspace_bytes(), device_cus, plans);
    if (n < 0) return n;
    int rc = 0;
    for (int i = 0; i < n && rc == 0; ++i) {
        const GemmPlan& pl = plans[i];
        GemmParams p;
        p.a = gemm_sanitised(g);
        if (pl.n0 > 0) {                                                 // second launch of a column split: every per-column operand moves along
            const int64_t n0 = pl.n0;
            p.a.w_hi = (const char*)g.w_hi + n0 * g.ldw * 2;
            if (g.w_lo) p.a.w_lo = (const char*)g.w_lo + n0 * g.ldw * 2;
            if (g.w_il) p.a.w_il = (const char*)g.w_il + n0 * g.ldw_il * 2;
            if (g.bias) p.a.bias = g.bias + n0;
            if (g.ln_colsum) p.a.ln_colsum = g.ln_colsum + n0;
            if (g.residual) p.a.residual = g.residual + n0;
            if (g.out_f32) p.a.out_f32 = g.out_f32 + n0;
            if (g.out_hi) p.a.out_hi = (char*)g.out_hi + n0 * 2 * (g.out_il ? 2 : 1);   // image: column c0 starts 2 * c0 halves into a row
            if (g.out_lo) p.a.out_lo = (char*)g.out_lo + n0 * 2;
        }
        p.a.N = pl.N;
        p.nbx = pl.nbx; p.nby = pl.nby; p.group_m = pl.group_m;
        p.tail_rem = pl.tail_rem; p.tail_split = pl.tail_split; p.total_blocks = pl.total_blocks; p.sk_parts = pl.sk_parts;
        p.flags = pl.use_ws ? (unsigned*)g.workspace : nullptr;
        p.ws = pl.use_ws ? (float*)((unsigned char*)g.workspace + TAIL_FLAG_BYTES) : nullptr;
#ifdef CVLM_PROBES
        p.trace = g_trace;
#endif
        hipStream_t s = (hipStream_t)stream;
        if (pl.k.mx) { rc = launch_mx(p, pl.k.mt, pl.k.epi, pl.grid_x - pl.nbx * pl.nby, pl.k.dbg, s); continue; }
        switch (gemm_kernel_key(pl.k)) {
#define CVLM_X(...) case gemm_kernel_key(GemmKernel{__VA_ARGS__}): rc = launch<__VA_ARGS__>(pl, p, s); break;
            CVLM_GEMM_KERNELS(CVLM_X)
#ifdef CVLM_PROBES
            CVLM_GEMM_PROBE_KERNELS(CVLM_X)
#endif
#undef CVLM_X
            default: rc = CVLM_E_UNSUPPORTED;                            // a plan without a kernel is an error, never another kernel
        }
    }
    return rc;
}

// Dry run (debug entry, include/cvlm.h): the launches cvlm_gemm would make for `args` with / without a workspace on a device of `cus`
// CUs, under the knobs of this process.  Launches nothing, needs no device.
extern "C" int cvlm_debug_gemm_plan(const cvlm_gemm_args* args, int have_ws, int cus, cvlm_gemm_plan_info* out) {
    if (!args || !out) return CVLM_E_BADARG;
    out->launches = 0;
    GemmPlan plans[2];
    const int n = plan_call(*args, have_ws != 0, [cus] { return cus; }, plans);
    if (n < 0) return n;
    out->launches = n;
    for (int i = 0; i < n; ++i) {
        const GemmPlan& pl = plans[i];
        auto& o = out->launch[i];
        o.n0 = pl.n0; o.N = pl.N; o.nbx = pl.nbx; o.nby = pl.nby; o.grid_x = pl.grid_x; o.grid_y = pl.grid_y; o.block = pl.block;
        o.lds_bytes = pl.lds_bytes; o.group_m = pl.group_m; o.tail_rem = pl.tail_rem; o.tail_split = pl.tail_split;
        o.total_blocks = pl.total_blocks; o.sk_parts = pl.sk_parts; o.uses_workspace = pl.use_ws;
        gemm_kernel_name(pl.k, o.kernel, sizeof o.kernel);
    }
    return 0;
}
