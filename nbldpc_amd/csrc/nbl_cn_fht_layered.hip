// nbldpc_amd/csrc/nbl_cn_fht_layered.hip -- FHT sum-product decoding under the damped layered (check-serial) schedule of
// include/nbldpc.h (nbl_create_fht with NBL_FHT_LAYERED): nbl_cn_bp_layered.hip with the check-node programme of nbl_cn_fht_core.h in
// place of the exact one.  The input former is that kernel's (nbl_cn_bp_inputs.h), and so is the argument for one c2v and one v2c buffer:
// every global read of a check's inputs happens in the programme's first step and is complete before its first c2v store in the last;
// the checks of a layer share no variable; an edge's v2c vector belongs to its check's wave alone; the launches of a stream order the
// layers.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_fht_core.h"
#include "nbl_cn_bp_inputs.h"

// the checks of one layer: one wave per (codeword, check); grid = count * (codeword slots)
template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	double *Cb = w.c2v + (size_t)b * g.E * Q;
	const BpLayeredInput<Q> input = {w.Lch + (size_t)b * g.N * Q, Cb, w.v2c + (size_t)b * g.E * Q, ly.nbr, g.c_epos, c0, lane_id(), r.damp_old, r.damp_new};
	fht_check_node<Q, BpLayeredInput<Q>, DCM>(g, smem, c0, dc, Cb + (size_t)c0 * Q, input);
}

#define NBL_LAYERED_Q(q, ...)                                   \
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

hipError_t nbl_launch_cn_fht_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_fht_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (g.maxdc > NBL_MAXDC || lds > 64 * 1024 || !w.v2c) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_LAYERED_Q(g.q, {
		if (g.maxdc <= 4) cn_fht_layered_kernel<QQ, 4><<<grid, block, lds, st>>>(g, w, r, ly, offset, count);
		else cn_fht_layered_kernel<QQ, NBL_MAXDC><<<grid, block, lds, st>>>(g, w, r, ly, offset, count);
	})
	return hipGetLastError();
}
