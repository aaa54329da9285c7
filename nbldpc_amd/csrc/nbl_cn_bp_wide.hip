// nbldpc_amd/csrc/nbl_cn_bp_wide.hip -- exact log-domain QSPA check node for checks of degree up to NBL_BP_MAX_CHECK_DEGREE
// (nbl_create_bp_wide on a code with a check above degree 8, or any such decoder under nbl_debug_force_generic(dec, 3)): the programme of
// nbl_cn_bp_wide_core.h, one instantiation per q for every degree, under both schedules.  One check per workgroup of max(1, q / 64)
// waves.  The input formers are those of cn_bp_kernel and cn_bp_layered_kernel (nbl_cn_bp_inputs.h, unchanged: per wave, one edge at a
// time); the one-buffer argument of the layered schedule (nbl_cn_bp_layered.hip) carries over with "wave" read as "workgroup" -- the
// checks of a layer share no variable, every input of a check is read before the workgroup's first barrier and C is first written after
// it (nbl_cn_bp_wide_core.h, Aliasing), an edge's v2c vector is read and written by the one wave that stages that edge.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_bp_wide_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q>
__global__ __launch_bounds__(BpWide<Q>::NT) void cn_bp_wide_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const BpV2cInput<Q> in = {w.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	bp_wide_check_node<Q>(g, smem, c0, dc, w.c2v + ((size_t)b * g.E + c0) * Q, in);
}

// the checks of one layer: one workgroup per (codeword, check); grid = count * (codeword slots)
template <int Q>
__global__ __launch_bounds__(BpWide<Q>::NT) void cn_bp_wide_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const double *L = w.Lch + (size_t)b * g.N * Q;
	double *Cb = w.c2v + (size_t)b * g.E * Q;
	double *Vb = w.v2c + (size_t)b * g.E * Q;
	const BpLayeredInput<Q> input = {L, Cb, Vb, ly.nbr, g.c_epos, c0, lane_id(), r.damp_old, r.damp_new};
	bp_wide_check_node<Q>(g, smem, c0, dc, Cb + (size_t)c0 * Q, input);
}

#define NBL_BP_WIDE_Q(q, ...)                                   \
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

// [maxdc][q] inputs, one [q] output vector, two [q] XP blocks of 16 bytes, the reduction words
size_t nbl_bp_wide_lds_bytes(int q, int maxdc) { return ((size_t)maxdc + 5) * (size_t)q * 8 + NBL_BP_WIDE_RED_DOUBLES * 8; }

static bool wide_shape_ok(const NblGraphDev &g, const NblWork &w, size_t lds)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_BP_MAX_CHECK_DEGREE && lds <= NBL_BP_WIDE_MAX_LDS && w.c2v && w.v2c;
}

hipError_t nbl_launch_cn_bp_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_bp_wide_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (!wide_shape_ok(g, w, lds) || blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue; // (nbl_create_bp_wide refuses such shapes)
	dim3 grid((unsigned)blocks);
	NBL_BP_WIDE_Q(g.q, {
		if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_bp_wide_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		cn_bp_wide_kernel<QQ><<<grid, dim3(BpWide<QQ>::NT), lds, st>>>(g, w, r);
	})
	return hipGetLastError();
}

hipError_t nbl_launch_cn_bp_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_bp_wide_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (!wide_shape_ok(g, w, lds) || !w.Lch) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks);
	NBL_BP_WIDE_Q(g.q, {
		if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_bp_wide_layered_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		cn_bp_wide_layered_kernel<QQ><<<grid, dim3(BpWide<QQ>::NT), lds, st>>>(g, w, r, ly, offset, count);
	})
	return hipGetLastError();
}
