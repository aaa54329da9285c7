// nbldpc_amd/csrc/nbl_cn_fht_wide.hip -- FHT sum-product check node for checks of degree up to NBL_FHT_MAX_CHECK_DEGREE (nbl_create_fht on a
// code with a check above degree 8, or any FHT decoder under nbl_debug_force_generic(dec, 3)): the programme of nbl_cn_fht_wide_core.h,
// one instantiation per q for every degree, under both schedules.  The launch shapes, the input formers (nbl_cn_bp_inputs.h) and the
// one-buffer argument of the layered schedule are those of nbl_cn_fht.hip and nbl_cn_fht_layered.hip: one wave per (codeword, check);
// every global read of a check's inputs happens in the programme's first step; between that step and a c2v region's final store the
// region holds the check's forward product, which only the owning wave reads -- the checks of a layer share no variable, and the
// launches of a stream order everything else.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_fht_wide_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q>
__global__ __launch_bounds__(64) void cn_fht_wide_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const BpV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	fht_wide_check_node<Q, BpV2cInput<Q>>(g, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer
template <int Q>
__global__ __launch_bounds__(64) void cn_fht_wide_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const BpLayeredInput<Q> input = {w.Lch + (size_t)k.b * g.N * Q, Cb, w.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), r.damp_old, r.damp_new};
	fht_wide_check_node<Q, BpLayeredInput<Q>>(g, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

// maxdc q 8 bytes of LDS: 64 KB at q = 256 and degree 32, the largest nbl_create_fht accepts and what a launch gets without opting in
static bool wide_shape_ok(const NblGraphDev &g, const NblWork &w)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_FHT_MAX_CHECK_DEGREE && nbl_fht_lds_bytes(g.q, g.maxdc) <= NBL_LDS_OPT_IN && w.v2c && w.c2v;
}

hipError_t nbl_launch_cn_fht_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	if (!wide_shape_ok(g, w)) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_fht_wide_kernel<QQ>, (long long)r.B * g.M, 64, nbl_fht_lds_bytes(g.q, g.maxdc), st, g, w, r))
}

hipError_t nbl_launch_cn_fht_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	if (!nbl_layer_range_ok(g, offset, count) || !wide_shape_ok(g, w)) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_fht_wide_layered_kernel<QQ>, (long long)r.B * count, 64, nbl_fht_lds_bytes(g.q, g.maxdc), st, g, w, r, ly, offset, count))
}
