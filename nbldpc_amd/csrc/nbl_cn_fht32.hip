// nbldpc_amd/csrc/nbl_cn_fht32.hip -- single-precision FHT sum-product check node (nbl_create_fht32): the programme of
// nbl_cn_fht32_core.h under the flooding schedule (one wave per (codeword, check), on the float v2c the variable-node pass of
// nbl_fht32.hip wrote) and under the damped layered schedule (the checks of one layer; each forms its inputs from Lf and the one float
// c2v buffer and damps them against the edge's float v2c, updated in place): the formers of nbl_cn_bp_inputs.h on float.  The launch
// shapes, and the argument for one c2v and one v2c buffer under the layered schedule, are those of nbl_cn_fht.hip /
// nbl_cn_fht_layered.hip.  q < 64 leaves lanes idle.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_fht32_core.h"
#include "nbl_cn_bp_inputs.h" // Bp32V2cInput, Bp32LayeredInput

template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht32_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const Bp32V2cInput<Q> in = {f.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	fht32_check_node<Q, Bp32V2cInput<Q>, DCM>(g, smem, k.c0, k.dc, f.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer: one wave per (codeword, check)
template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht32_layered_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	float *Cb = f.c2v + (size_t)k.b * g.E * Q;
	const Bp32LayeredInput<Q> input = {f.Lf + (size_t)k.b * g.N * Q, Cb, f.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), (float)r.damp_old, (float)r.damp_new};
	fht32_check_node<Q, Bp32LayeredInput<Q>, DCM>(g, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

hipError_t nbl_launch_cn_fht32(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st)
{
	// maxdc q 4 bytes: 8 KB at q = 256 and degree 8, the largest this programme runs (nbl_create_fht32 refuses a larger check)
	const size_t lds = nbl_fht32_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (g.maxdc > NBL_MAXDC || lds > NBL_LDS_OPT_IN || !f.v2c || !f.c2v) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, {
		if (g.maxdc <= 4) return nbl_launch_checks(cn_fht32_kernel<QQ, 4>, blocks, 64, lds, st, g, w, f, r);
		return nbl_launch_checks(cn_fht32_kernel<QQ, NBL_MAXDC>, blocks, 64, lds, st, g, w, f, r);
	})
}

hipError_t nbl_launch_cn_fht32_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                       hipStream_t st)
{
	const size_t lds = nbl_fht32_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * count;
	if (!nbl_layer_range_ok(g, offset, count) || g.maxdc > NBL_MAXDC || lds > NBL_LDS_OPT_IN || !f.v2c || !f.c2v || !f.Lf) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, {
		if (g.maxdc <= 4) return nbl_launch_checks(cn_fht32_layered_kernel<QQ, 4>, blocks, 64, lds, st, g, w, f, r, ly, offset, count);
		return nbl_launch_checks(cn_fht32_layered_kernel<QQ, NBL_MAXDC>, blocks, 64, lds, st, g, w, f, r, ly, offset, count);
	})
}
