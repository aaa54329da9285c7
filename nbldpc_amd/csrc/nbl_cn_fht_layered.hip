// nbldpc_amd/csrc/nbl_cn_fht_layered.hip -- FHT sum-product decoding under the damped layered (check-serial) schedule of
// include/nbldpc.h (nbl_create_fht with NBL_FHT_LAYERED): nbl_cn_bp_layered.hip with the check-node programme of nbl_cn_fht_core.h in
// place of the exact one.  The input former is BpLayeredInput (nbl_cn_bp_inputs.h), and the argument for one c2v and one v2c buffer is
// that kernel's: every global read of a check's inputs happens in the programme's first step and is complete before its first c2v store
// in the last; the checks of a layer share no variable; an edge's v2c vector belongs to its check's wave alone; the launches of a stream
// order the layers.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_fht_core.h"
#include "nbl_cn_bp_inputs.h"

// the checks of one layer: one wave per (codeword, check)
template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const BpLayeredInput<Q> input = {w.Lch + (size_t)k.b * g.N * Q, Cb, w.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), r.damp_old, r.damp_new};
	fht_check_node<Q, BpLayeredInput<Q>, DCM>(g, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

hipError_t nbl_launch_cn_fht_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const size_t lds = nbl_fht_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (!nbl_layer_range_ok(g, offset, count) || g.maxdc > NBL_MAXDC || lds > NBL_LDS_OPT_IN || !w.v2c) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, {
		if (g.maxdc <= 4) return nbl_launch_checks(cn_fht_layered_kernel<QQ, 4>, blocks, 64, lds, st, g, w, r, ly, offset, count);
		return nbl_launch_checks(cn_fht_layered_kernel<QQ, NBL_MAXDC>, blocks, 64, lds, st, g, w, r, ly, offset, count);
	})
}
