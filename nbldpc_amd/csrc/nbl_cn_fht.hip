// nbldpc_amd/csrc/nbl_cn_fht.hip -- FHT sum-product check node under the flooding schedule (nbl_create_fht, flags 0): the programme of
// nbl_cn_fht_core.h (which the layered kernel, nbl_cn_fht_layered.hip, shares) on the v2c vectors the variable-node pass wrote.  The
// launch shape is that of nbl_cn_bp.hip: one wave per (codeword, check).  q < 64 leaves lanes idle, as the general kernels do.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_fht_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q, int DCM>
__global__ __launch_bounds__(64) void cn_fht_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const BpV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	fht_check_node<Q, BpV2cInput<Q>, DCM>(g, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

hipError_t nbl_launch_cn_fht(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	// maxdc q 8 bytes: 16 KB at q = 256 and degree 8, the largest this programme runs (a code with a larger check, up to
	// NBL_FHT_MAX_CHECK_DEGREE, takes nbl_cn_fht_wide.hip)
	const size_t lds = nbl_fht_lds_bytes(g.q, g.maxdc);
	const long long blocks = (long long)r.B * g.M;
	if (g.maxdc > NBL_MAXDC || lds > NBL_LDS_OPT_IN || !w.v2c) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, {
		if (g.maxdc <= 4) return nbl_launch_checks(cn_fht_kernel<QQ, 4>, blocks, 64, lds, st, g, w, r);
		return nbl_launch_checks(cn_fht_kernel<QQ, NBL_MAXDC>, blocks, 64, lds, st, g, w, r);
	})
}
