// nbldpc_amd/csrc/nbl_cn_fht32.hip -- single-precision FHT sum-product check node (nbl_create_fht32): the programme of
// nbl_cn_fht32_core.h under the flooding schedule (one wave per (codeword, check), on the float v2c the variable-node pass of
// nbl_fht32.hip wrote) and under the damped layered schedule (the checks of one layer; each forms its inputs from Lf and the one float
// c2v buffer and damps them against the edge's float v2c, updated in place).  The launch shapes, and the argument for one c2v and one
// v2c buffer under the layered schedule, are those of nbl_cn_fht.hip / nbl_cn_fht_layered.hip.  q < 64 leaves lanes idle.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_fht32_core.h"
#include "nbl_cn_fht32_inputs.h" // Bp32V2cInput, Bp32LayeredInput

template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht32_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const Bp32V2cInput<Q> in = {f.v2c + (size_t)b * g.E * Q, g.c_epos + c0, lane_id()};
	fht32_check_node<Q, Bp32V2cInput<Q>, DCM>(g, smem, c0, dc, f.c2v + ((size_t)b * g.E + c0) * Q, in);
}

// the checks of one layer: one wave per (codeword, check); grid = count * (codeword slots)
template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht32_layered_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	float *Cb = f.c2v + (size_t)b * g.E * Q;
	const Bp32LayeredInput<Q> input = {f.Lf + (size_t)b * g.N * Q, Cb, f.v2c + (size_t)b * g.E * Q, ly.nbr, g.c_epos, c0, lane_id(), (float)r.damp_old, (float)r.damp_new};
	fht32_check_node<Q, Bp32LayeredInput<Q>, DCM>(g, smem, c0, dc, Cb + (size_t)c0 * Q, input);
}

#define NBL_FHT32_Q(q, ...)                                     \
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

hipError_t nbl_launch_cn_fht32(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st)
{
	// maxdc q 4 bytes: 8 KB at q = 256 and degree 8, the largest this programme runs (nbl_create_fht32 refuses a larger check)
	const size_t lds = nbl_fht32_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (g.maxdc > NBL_MAXDC || lds > 64 * 1024 || blocks > 0x7fffffffLL || !f.v2c || !f.c2v) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_FHT32_Q(g.q, {
		if (g.maxdc <= 4) cn_fht32_kernel<QQ, 4><<<grid, block, lds, st>>>(g, w, f, r);
		else cn_fht32_kernel<QQ, NBL_MAXDC><<<grid, block, lds, st>>>(g, w, f, r);
	})
	return hipGetLastError();
}

hipError_t nbl_launch_cn_fht32_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                       hipStream_t st)
{
	const size_t lds = nbl_fht32_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (g.maxdc > NBL_MAXDC || lds > 64 * 1024 || !f.v2c || !f.c2v || !f.Lf) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks), block(64);
	NBL_FHT32_Q(g.q, {
		if (g.maxdc <= 4) cn_fht32_layered_kernel<QQ, 4><<<grid, block, lds, st>>>(g, w, f, r, ly, offset, count);
		else cn_fht32_layered_kernel<QQ, NBL_MAXDC><<<grid, block, lds, st>>>(g, w, f, r, ly, offset, count);
	})
	return hipGetLastError();
}
