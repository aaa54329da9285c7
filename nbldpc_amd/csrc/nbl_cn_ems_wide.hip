// nbldpc_amd/csrc/nbl_cn_ems_wide.hip -- EMS check node for checks of degree up to NBL_EMS_MAX_CHECK_DEGREE (nbl_create_ems_wide on a code
// with a check above degree 8, or any such decoder under nbl_debug_force_generic(dec, 3)): the programme of nbl_cn_ems_wide_core.h, one
// instantiation per q for every degree, under both schedules.  One check per workgroup of max(1, q / 64) waves.  The inputs are
// EmsV2cInput (the v2c vectors of the variable-node pass) and EmsLayeredInput (L_ch and the in-place c2v through the layer rows) of
// nbl_cn_shell.h; the one-buffer argument of the layered schedule is unchanged -- the checks of a layer share no variable, every
// input of a check is read before the workgroup's first barrier and every output written after it.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_ems_wide_core.h"

template <int Q>
__global__ __launch_bounds__(EmsWide<Q>::NT) void cn_ems_wide_kernel(NblGraphDev g, NblWork w, NblRun r, int layers)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const EmsV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos, k.c0};
	ems_wide_check_node<Q>(g, r, layers, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer
template <int Q>
__global__ __launch_bounds__(EmsWide<Q>::NT) void cn_ems_wide_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count, int layers)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const EmsLayeredInput<Q> in = {w.Lch + (size_t)k.b * g.N * Q, Cb, ly.nbr, k.c0};
	ems_wide_check_node<Q>(g, r, layers, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, in);
}

// [maxdc][q] inputs, prefix + ping + pong of [layers][q], one [q] output vector, the lists [maxdc][nm] (8 + 4 bytes an entry)
size_t nbl_ems_wide_lds_bytes(int q, int maxdc, int nm, int nc)
{
	const size_t doubles = (size_t)maxdc * q + (3 * (size_t)nbl_ems_layers(maxdc, nc) + 1) * q + (size_t)maxdc * nm;
	return doubles * 8 + (size_t)maxdc * nm * 4 + 16;
}

static bool wide_shape_ok(const NblGraphDev &g, const NblWork &w, const NblRun &r, size_t lds)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_EMS_MAX_CHECK_DEGREE && r.nm >= 1 && r.nm <= g.q && r.nc >= 0 && lds <= NBL_MAX_LDS && w.c2v;
}

hipError_t nbl_launch_cn_ems_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const int layers = nbl_ems_layers(g.maxdc, r.nc);
	const size_t lds = nbl_ems_wide_lds_bytes(g.q, g.maxdc, r.nm, r.nc);
	if (!wide_shape_ok(g, w, r, lds) || !w.v2c) return hipErrorInvalidValue; // (nbl_create_ems_wide refuses such shapes)
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_ems_wide_kernel<QQ>, (long long)r.B * g.M, EmsWide<QQ>::NT, lds, st, g, w, r, layers))
}

hipError_t nbl_launch_cn_ems_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const int layers = nbl_ems_layers(g.maxdc, r.nc);
	const size_t lds = nbl_ems_wide_lds_bytes(g.q, g.maxdc, r.nm, r.nc);
	if (!nbl_layer_range_ok(g, offset, count) || !wide_shape_ok(g, w, r, lds)) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_ems_wide_layered_kernel<QQ>, (long long)r.B * count, EmsWide<QQ>::NT, lds, st, g, w, r, ly, offset, count, layers))
}
