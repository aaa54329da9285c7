// nbldpc_amd/csrc/nbl_cn_bp_wide.hip -- exact log-domain QSPA check node for checks of degree up to NBL_BP_MAX_CHECK_DEGREE
// (nbl_create_bp_wide on a code with a check above degree 8, or any such decoder under nbl_debug_force_generic(dec, 3)): the programme of
// nbl_cn_bp_wide_core.h, one instantiation per q for every degree, under both schedules.  One check per workgroup of max(1, q / 64)
// waves.  The input formers are BpV2cInput and BpLayeredInput (nbl_cn_bp_inputs.h: per wave, one edge at a time); the one-buffer
// argument of the layered schedule (nbl_cn_bp_layered.hip) carries over with "wave" read as "workgroup" -- the checks of a layer share no
// variable, every input of a check is read before the workgroup's first barrier and C is first written after it
// (nbl_cn_bp_wide_core.h, Aliasing), an edge's v2c vector is read and written by the one wave that stages that edge.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_bp_wide_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q>
__global__ __launch_bounds__(BpWide<Q>::NT) void cn_bp_wide_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const BpV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	bp_wide_check_node<Q>(g, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer: one workgroup per (codeword, check)
template <int Q>
__global__ __launch_bounds__(BpWide<Q>::NT) void cn_bp_wide_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const BpLayeredInput<Q> input = {w.Lch + (size_t)k.b * g.N * Q, Cb, w.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), r.damp_old, r.damp_new};
	bp_wide_check_node<Q>(g, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

// [maxdc][q] inputs, one [q] output vector, two [q] XP blocks of 16 bytes, the reduction words
size_t nbl_bp_wide_lds_bytes(int q, int maxdc) { return ((size_t)maxdc + 5) * (size_t)q * 8 + NBL_BP_WIDE_RED_DOUBLES * 8; }

static bool wide_shape_ok(const NblGraphDev &g, const NblWork &w, size_t lds)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_BP_MAX_CHECK_DEGREE && lds <= NBL_MAX_LDS && w.c2v && w.v2c;
}

hipError_t nbl_launch_cn_bp_wide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_bp_wide_lds_bytes(g.q, g.maxdc);
	if (!wide_shape_ok(g, w, lds)) return hipErrorInvalidValue; // (nbl_create_bp_wide refuses such shapes)
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_bp_wide_kernel<QQ>, (long long)r.B * g.M, BpWide<QQ>::NT, lds, st, g, w, r))
}

hipError_t nbl_launch_cn_bp_wide_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_bp_wide_lds_bytes(g.q, g.maxdc);
	if (!nbl_layer_range_ok(g, offset, count) || !wide_shape_ok(g, w, lds) || !w.Lch) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_bp_wide_layered_kernel<QQ>, (long long)r.B * count, BpWide<QQ>::NT, lds, st, g, w, r, ly, offset, count))
}
