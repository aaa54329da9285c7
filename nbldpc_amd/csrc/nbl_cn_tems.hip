// nbldpc_amd/csrc/nbl_cn_tems.hip -- trellis-EMS check node (NBLDPC.cpp:1055-1130, helpers :1789-1944) of the flooding schedule.
//
// One wave per (codeword, check).  The check-node programmes -- the general one for any nc and the fast one for nc <= 3 -- live in
// nbl_cn_tems_core.h, which the layered kernel (nbl_cn_tems_layered.hip) shares; here their inputs are the v2c vectors the
// variable-node pass wrote, read through c_epos.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_tems_core.h"
#include <cstdlib>

template <int Q>
__global__ __launch_bounds__(64) void cn_tems_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const TemsV2cInput<Q> in = {w.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	tems_check_node<Q>(g, r, smem, c0, dc, w.c2v + ((size_t)b * g.E + c0) * Q, in);
}

// fast variant (nc <= 3)
template <int Q>
__global__ __launch_bounds__(64) void cn_tems_fast_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const TemsV2cInput<Q> in = {w.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	tems_fast_check_node<Q>(g, r, smem, c0, dc, w.c2v + ((size_t)b * g.E + c0) * Q, in);
}

bool nbl_tems_use_fast(int nc) { return nc <= 3 && !getenv("NBL_TEMS_GENERIC"); }

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

hipError_t nbl_launch_cn_tems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_tems_lds_bytes(g.q, g.maxdc, r.nc);
	if (lds > 160 * 1024) return hipErrorInvalidValue;
	if ((double)g.p * g.maxdc > 32.0) return hipErrorInvalidValue; // path code must fit 32 bits
	dim3 grid((unsigned)((long long)r.B * g.M)), block(64);
	if (nbl_tems_use_fast(r.nc)) {
		const size_t fl = nbl_tems_fast_lds_bytes(g.q, g.maxdc);
		NBL_DISPATCH_Q(g.q, {
			if (fl > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_tems_fast_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl);
			cn_tems_fast_kernel<QQ><<<grid, block, fl, st>>>(g, w, r);
		})
		return hipGetLastError();
	}
	NBL_DISPATCH_Q(g.q, {
		if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_tems_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		cn_tems_kernel<QQ><<<grid, block, lds, st>>>(g, w, r);
	})
	return hipGetLastError();
}
