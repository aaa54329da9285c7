// nbldpc_amd/csrc/nbl_cn_tems_wide.hip -- trellis-EMS check node for checks of degree up to NBL_TEMS_MAX_CHECK_DEGREE over any field
// (nbl_create_tems_wide on a code whose path does not fit tems_check_node's 32-bit code, or any such decoder under
// nbl_debug_force_generic(dec, 3)): the programme of nbl_cn_tems_wide_core.h, one instantiation per q for every degree, under both
// schedules.  One check per workgroup of max(1, q / 64) waves.  The input formers are those of the general kernels: flooding reads the
// v2c vectors of the variable-node pass (TemsV2cInput, nbl_cn_tems_core.h); layered forms the raw input from L_ch and the in-place c2v
// through the layer rows, damps it 0.25 / 0.75 against the edge's stored v2c where the two decide differently and stores it back
// (BpLayeredInput, nbl_cn_bp_inputs.h).  The one-buffer argument of the layered schedule (nbl_cn_tems_layered.hip) is unchanged -- the
// checks of a layer share no variable, an edge's v2c belongs to one wave of one workgroup, every input of a check is read before the
// workgroup's first barrier and every c2v vector written after it.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_tems_core.h" // TemsV2cInput
#include "nbl_cn_bp_inputs.h" // BpLayeredInput
#include "nbl_cn_tems_wide_core.h"

template <int Q>
__global__ __launch_bounds__(TemsWide<Q>::NT) void cn_tems_wide_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const TemsV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	tems_wide_check_node<Q>(g, r, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer
template <int Q>
__global__ __launch_bounds__(TemsWide<Q>::NT) void cn_tems_wide_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const BpLayeredInput<Q> in = {w.Lch + (size_t)k.b * g.N * Q, Cb, w.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), r.damp_old, r.damp_new};
	tems_wide_check_node<Q>(g, r, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, in);
}

size_t nbl_tems_wide_lds_bytes(int q, int maxdc, int nr, int nc)
{
	return nbl_tems_wide_lds_layout((size_t)q, (size_t)maxdc, (size_t)(nr < 1 ? 1 : nr), (size_t)(nc < 0 ? 0 : nc));
}

static bool wide_shape_ok(const NblGraphDev &g, const NblWork &w, const NblRun &r, size_t lds)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_TEMS_MAX_CHECK_DEGREE && r.nr >= 1 && r.nc >= 0 && r.nc <= NBL_TEMS_WIDE_MAX_NC && lds <= NBL_MAX_LDS && w.c2v && w.v2c;
}

hipError_t nbl_launch_cn_tems_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_tems_wide_lds_bytes(g.q, g.maxdc, r.nr, r.nc);
	if (!wide_shape_ok(g, w, r, lds)) return hipErrorInvalidValue; // (nbl_create_tems_wide refuses such shapes)
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_tems_wide_kernel<QQ>, (long long)r.B * g.M, TemsWide<QQ>::NT, lds, st, g, w, r))
}

hipError_t nbl_launch_cn_tems_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_tems_wide_lds_bytes(g.q, g.maxdc, r.nr, r.nc);
	if (!nbl_layer_range_ok(g, offset, count) || !wide_shape_ok(g, w, r, lds)) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_tems_wide_layered_kernel<QQ>, (long long)r.B * count, TemsWide<QQ>::NT, lds, st, g, w, r, ly, offset, count))
}
