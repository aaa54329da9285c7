// nbldpc_amd/csrc/nbl_cn_minmax.hip -- Min-Max check node (method 3; nbl_create_minmax): the programme of nbl_cn_minmax_core.h, one
// instantiation per q for every check degree 2 .. NBL_MINMAX_MAX_CHECK_DEGREE, under both schedules.  One check per workgroup of
// max(1, q / 64) waves.  The inputs are the EMS ones (nbl_cn_shell.h): flooding reads the v2c vectors of the variable-node pass
// (EmsV2cInput), layered forms L_ch plus the in-place c2v through the layer rows and subtracts the edge's own c2v (EmsLayeredInput); the
// one-buffer argument of the layered schedule is unchanged -- the checks of a layer share no variable, every input of a check is read
// before the workgroup's first barrier and every output (the parked forward partials included) written after it.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_minmax_core.h"

template <int Q>
__global__ __launch_bounds__(MinMax<Q>::NT) void cn_minmax_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const EmsV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos, k.c0};
	minmax_check_node<Q>(g, r, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer
template <int Q>
__global__ __launch_bounds__(MinMax<Q>::NT) void cn_minmax_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const EmsLayeredInput<Q> in = {w.Lch + (size_t)k.b * g.N * Q, Cb, ly.nbr, k.c0};
	minmax_check_node<Q>(g, r, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, in);
}

// [maxdc][q] dissimilarities, two [q] operand blocks, two [q] output vectors
size_t nbl_minmax_lds_bytes(int q, int maxdc) { return ((size_t)maxdc + 4) * (size_t)q * 8; }

static bool minmax_shape_ok(const NblGraphDev &g, const NblWork &w, size_t lds)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_MINMAX_MAX_CHECK_DEGREE && lds <= NBL_MAX_LDS && w.c2v;
}

hipError_t nbl_launch_cn_minmax(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_minmax_lds_bytes(g.q, g.maxdc);
	if (!minmax_shape_ok(g, w, lds) || !w.v2c) return hipErrorInvalidValue; // (nbl_create_minmax refuses such shapes)
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_minmax_kernel<QQ>, (long long)r.B * g.M, MinMax<QQ>::NT, lds, st, g, w, r))
}

hipError_t nbl_launch_cn_minmax_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_minmax_lds_bytes(g.q, g.maxdc);
	if (!nbl_layer_range_ok(g, offset, count) || !minmax_shape_ok(g, w, lds) || !w.Lch) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_minmax_layered_kernel<QQ>, (long long)r.B * count, MinMax<QQ>::NT, lds, st, g, w, r, ly, offset, count))
}
