// nbldpc_amd/csrc/nbl_cn_bp.hip -- exact log-domain QSPA check node under the flooding schedule: the programme of nbl_cn_bp_core.h
// (which the layered kernel, nbl_cn_bp_layered.hip, shares) on the v2c vectors the variable-node pass wrote.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_bp_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q>
__global__ __launch_bounds__(64) void cn_bp_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const BpV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	bp_check_node<Q>(g, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

hipError_t nbl_launch_cn_bp(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_bp_lds_bytes(g.q, g.maxdc);
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_bp_kernel<QQ>, (long long)r.B * g.M, 64, lds, st, g, w, r))
}
