// nbldpc_amd/csrc/nbl_cn_bp.hip -- exact log-domain QSPA check node under the flooding schedule: the programme of nbl_cn_bp_core.h
// (which the layered kernel, nbl_cn_bp_layered.hip, shares) on the v2c vectors the variable-node pass wrote.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_bp_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q>
__global__ __launch_bounds__(64) void cn_bp_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const BpV2cInput<Q> in = {w.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	bp_check_node<Q>(g, smem, c0, dc, w.c2v + ((size_t)b * g.E + c0) * Q, in);
}

#define NBL_DISPATCH_Q(q, ...)                                  \
	switch (q) {                                                \
	case 4: { constexpr int QQ = 4; __VA_ARGS__; } break;       \
	case 8: { constexpr int QQ = 8; __VA_ARGS__; } break;       \
	case 16: { constexpr int QQ = 16; __VA_ARGS__; } break;     \
	case 32: { constexpr int QQ = 32; __VA_ARGS__; } break;     \
	case 64: { constexpr int QQ = 64; __VA_ARGS__; } break;     \
	case 128: { constexpr int QQ = 128; __VA_ARGS__; } break;   \
	case 256: { constexpr int QQ = 256; __VA_ARGS__; } break;   \
	default: return hipErrorInvalidValue;                       \
	}

hipError_t nbl_launch_cn_bp(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_bp_lds_bytes(g.q, g.maxdc);
	dim3 grid((unsigned)((long long)r.B * g.M)), block(64);
	NBL_DISPATCH_Q(g.q, {
		if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_bp_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		cn_bp_kernel<QQ><<<grid, block, lds, st>>>(g, w, r);
	})
	return hipGetLastError();
}
