// nbldpc_amd/csrc/nbl_cn_fht.hip -- FHT sum-product check node under the flooding schedule (nbl_create_fht, flags 0): the programme of
// nbl_cn_fht_core.h (which the layered kernel, nbl_cn_fht_layered.hip, shares) on the v2c vectors the variable-node pass wrote.  The
// launch shape is that of nbl_cn_bp.hip: one wave per (codeword, check).  q < 64 leaves lanes idle, as the general kernels do.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_fht_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const BpV2cInput<Q> in = {w.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	fht_check_node<Q, BpV2cInput<Q>, DCM>(g, smem, c0, dc, w.c2v + ((size_t)b * g.E + c0) * Q, in);
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

hipError_t nbl_launch_cn_fht(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	// maxdc q 8 bytes: 16 KB at q = 256 and degree 8, the largest this programme runs (a code with a larger check, up to
	// NBL_FHT_MAX_CHECK_DEGREE, takes nbl_cn_fht_wide.hip)
	const size_t lds = nbl_fht_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (g.maxdc > NBL_MAXDC || lds > 64 * 1024 || blocks > 0x7fffffffLL || !w.v2c) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_DISPATCH_Q(g.q, {
		if (g.maxdc <= 4) cn_fht_kernel<QQ, 4><<<grid, block, lds, st>>>(g, w, r);
		else cn_fht_kernel<QQ, NBL_MAXDC><<<grid, block, lds, st>>>(g, w, r);
	})
	return hipGetLastError();
}
