// nbldpc_amd/csrc/nbl_cn_minmax.hip -- Min-Max check node (method 3; nbl_create_minmax): the programme of nbl_cn_minmax_core.h, one
// instantiation per q for every check degree 2 .. NBL_MINMAX_MAX_CHECK_DEGREE, under both schedules.  One check per workgroup of
// max(1, q / 64) waves.  The launchers and the input formers are those of nbl_cn_ems_wide.hip: flooding reads the v2c vectors of the
// variable-node pass, layered forms L_ch plus the in-place c2v through the layer rows and subtracts the edge's own c2v; the one-buffer
// argument of the layered schedule is unchanged -- the checks of a layer share no variable, every input of a check is read before the
// workgroup's first barrier and every output (the parked forward partials included) written after it.
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"
#include "nbl_cn_minmax_core.h"

template <int Q>
__global__ __launch_bounds__(MinMax<Q>::NT) void cn_minmax_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / g.M), m = blockIdx.x % g.M;
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const double *V = w.v2c + (size_t)b * g.E * Q;
	double *C = w.c2v + ((size_t)b * g.E + c0) * Q;
	minmax_check_node<Q>(g, r, smem, c0, dc, C, [&](int j) {
		const double *Vj = V + (size_t)g.c_epos[c0 + j] * Q;
		return [=](int a) { return Vj[a]; };
	});
}

// the checks of one layer: grid = count * (codeword slots)
template <int Q>
__global__ __launch_bounds__(MinMax<Q>::NT) void cn_minmax_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_codeword(w, r, blockIdx.x / count), m = ly.chk[offset + blockIdx.x % count];
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;
	const int c0 = g.coff[m], dc = g.coff[m + 1] - c0;
	const double *L = w.Lch + (size_t)b * g.N * Q;
	double *Cb = w.c2v + (size_t)b * g.E * Q;
	// input of edge j, variable n: P = L_ch[n], then + c2v of each of n's edges in n's order (the CURRENT values), then - c2v of this
	// edge (include/nbldpc.h); the row gives every address after one index load
	minmax_check_node<Q>(g, r, smem, c0, dc, Cb + (size_t)c0 * Q, [&](int j) {
		const int *row = ly.nbr + (size_t)(c0 + j) * NBL_LAYER_ROW;
		const int dv = row[1];
		const double *Ln = L + (size_t)row[0] * Q;
		const double *own = Cb + (size_t)(c0 + j) * Q;
		const double *nb[NBL_MAXDV];
#pragma unroll
		for (int d = 0; d < NBL_MAXDV; d++) nb[d] = Cb + (size_t)row[4 + (d < dv ? d : 0)] * Q;
		return [=](int a) {
			double P = Ln[a];
#pragma unroll
			for (int d = 0; d < NBL_MAXDV; d++)
				if (d < dv) P = P + nb[d][a];
			return P - own[a];
		};
	});
}

#define NBL_MINMAX_Q(q, ...)                                    \
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

// [maxdc][q] dissimilarities, two [q] operand blocks, two [q] output vectors
size_t nbl_minmax_lds_bytes(int q, int maxdc) { return ((size_t)maxdc + 4) * (size_t)q * 8; }

static bool minmax_shape_ok(const NblGraphDev &g, const NblWork &w, size_t lds)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_MINMAX_MAX_CHECK_DEGREE && lds <= NBL_MINMAX_MAX_LDS && w.c2v;
}

hipError_t nbl_launch_cn_minmax(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_minmax_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (!minmax_shape_ok(g, w, lds) || !w.v2c || blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue; // (nbl_create_minmax refuses such shapes)
	dim3 grid((unsigned)blocks);
	NBL_MINMAX_Q(g.q, {
		if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_minmax_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		cn_minmax_kernel<QQ><<<grid, dim3(MinMax<QQ>::NT), lds, st>>>(g, w, r);
	})
	return hipGetLastError();
}

hipError_t nbl_launch_cn_minmax_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_minmax_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (count < 1 || offset < 0 || offset + count > g.M || blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (!minmax_shape_ok(g, w, lds) || !w.Lch) return hipErrorInvalidValue;
	dim3 grid((unsigned)blocks);
	NBL_MINMAX_Q(g.q, {
		if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)cn_minmax_layered_kernel<QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		cn_minmax_layered_kernel<QQ><<<grid, dim3(MinMax<QQ>::NT), lds, st>>>(g, w, r, ly, offset, count);
	})
	return hipGetLastError();
}
