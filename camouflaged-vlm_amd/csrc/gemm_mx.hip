// The gemm_nt_kernel variants whose operands are mx images (include/cvlm.h, ABI 10: fp16 hi.hi product + the two correction products
// on the block-scaled e4m3 matrix instruction) and their launcher; called from gemm.hip (cvlm_gemm) with the kernel, the tile counts
// and the K-parts of a partial last round that gemm_plan.h chose.
#include "gemm_kernel.h"
#include "gemm_plan.h"
using namespace cvlm_gemm_k;
using namespace cvlm_gemm_p;

template <int MT_, int EPI_, int DBG_>
static int launch_one(const GemmParams& p, int extra_blocks, hipStream_t s) {
    constexpr int smem_ = gemm_lds_bytes(gemm_mx_kernel(MT_, EPI_, DBG_));
    auto kern_ = gemm_nt_kernel<3, 2, 4, 5, 32, DBG_, MT_, false, EPI_, false, false, true, true, true>;
    static bool attr_[16] = {};
    if (cvlm_first_on_device(attr_))
        (void)hipFuncSetAttribute((const void*)kern_, hipFuncAttributeMaxDynamicSharedMemorySize, smem_);
    hipLaunchKernelGGL(kern_, dim3(p.nbx * p.nby + extra_blocks, 1), dim3(512), smem_, s, p);
    CVLM_CHECK_LAUNCH();
    return 0;
}

int cvlm_gemm_k::launch_mx(GemmParams& p, int mt, int epi, int extra_blocks, int probe, hipStream_t s) {
#define CVLM_X(MT, EPI, DBG) if (mt == MT && epi == EPI && probe == DBG) return launch_one<MT, EPI, DBG>(p, extra_blocks, s);
    CVLM_GEMM_MX_KERNELS(CVLM_X)
#ifdef CVLM_PROBES
    CVLM_GEMM_MX_PROBE_KERNELS(CVLM_X)
#endif
#undef CVLM_X
    return CVLM_E_UNSUPPORTED;                                            /* the plain epilogue has no mx instantiation (no caller) */
}
