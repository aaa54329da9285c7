// nbldpc_amd/csrc/nbl_cn_tems.hip -- trellis-EMS check node (NBLDPC.cpp:1055-1130, helpers :1789-1944) of the flooding schedule.
//
// One wave per (codeword, check).  The check-node programmes -- the general one for any nc and the fast one for nc <= 3 -- live in
// nbl_cn_tems_core.h, which the layered kernel (nbl_cn_tems_layered.hip) shares; here their inputs are the v2c vectors the
// variable-node pass wrote, read through c_epos.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_tems_core.h"
#include <cstdlib>

template <int Q>
__global__ __launch_bounds__(64) void cn_tems_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const TemsV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	tems_check_node<Q>(g, r, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// fast variant (nc <= 3)
template <int Q>
__global__ __launch_bounds__(64) void cn_tems_fast_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const TemsV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	tems_fast_check_node<Q>(g, r, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

bool nbl_tems_use_fast(int nc) { return nc <= 3 && !getenv("NBL_TEMS_GENERIC"); }

hipError_t nbl_launch_cn_tems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const size_t lds = nbl_tems_lds_bytes(g.q, g.maxdc, r.nc);
	if (lds > NBL_MAX_LDS) return hipErrorInvalidValue;
	if ((double)g.p * g.maxdc > 32.0) return hipErrorInvalidValue; // path code must fit 32 bits
	const long long blocks = (long long)r.B * g.M;
	if (nbl_tems_use_fast(r.nc)) {
		const size_t fl = nbl_tems_fast_lds_bytes(g.q, g.maxdc);
		NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_tems_fast_kernel<QQ>, blocks, 64, fl, st, g, w, r))
	}
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_tems_kernel<QQ>, blocks, 64, lds, st, g, w, r))
}
