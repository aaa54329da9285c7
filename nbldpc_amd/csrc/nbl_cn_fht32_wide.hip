// nbldpc_amd/csrc/nbl_cn_fht32_wide.hip -- single-precision FHT sum-product check node for checks of degree up to
// NBL_FHT32_MAX_CHECK_DEGREE (nbl_create_fht32_wide on a code with a check above degree 8, or any such decoder under
// nbl_debug_force_generic(dec, 3)): the programme of nbl_cn_fht32_wide_core.h, one instantiation per q for every degree, under both
// schedules.  The launch shapes and the input formers (nbl_cn_bp_inputs.h on float) are those of nbl_cn_fht32.hip: one wave per
// (codeword, check); every global read of a check's inputs happens in the programme's first step; between that step and a c2v region's
// final store the region holds the check's forward product, which only the owning wave reads -- the checks of a layer share no variable,
// and the launches of a stream order everything else.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_fht32_wide_core.h"
#include "nbl_cn_bp_inputs.h"

template <int Q>
__global__ __launch_bounds__(64) void cn_fht32_wide_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const Bp32V2cInput<Q> in = {f.v2c + (size_t)k.b * g.E * Q, g.c_epos + k.c0, lane_id()};
	fht32_wide_check_node<Q, Bp32V2cInput<Q>>(g, smem, k.c0, k.dc, f.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// the checks of one layer
template <int Q>
__global__ __launch_bounds__(64) void cn_fht32_wide_layered_kernel(NblGraphDev g, NblWork w, NblWork32 f, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	float *Cb = f.c2v + (size_t)k.b * g.E * Q;
	const Bp32LayeredInput<Q> input = {f.Lf + (size_t)k.b * g.N * Q, Cb, f.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), (float)r.damp_old, (float)r.damp_new};
	fht32_wide_check_node<Q, Bp32LayeredInput<Q>>(g, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

// maxdc q 4 bytes of LDS: 32 KB at q = 256 and degree 32, the largest nbl_create_fht32_wide accepts
static bool wide32_shape_ok(const NblGraphDev &g, const NblWork32 &f)
{
	return g.maxdc >= 2 && g.maxdc <= NBL_FHT32_MAX_CHECK_DEGREE && nbl_fht32_wide_lds_bytes(g.q, g.maxdc) <= NBL_LDS_OPT_IN && f.v2c && f.c2v;
}

hipError_t nbl_launch_cn_fht32_wide(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, hipStream_t st)
{
	if (!wide32_shape_ok(g, f)) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_fht32_wide_kernel<QQ>, (long long)r.B * g.M, 64, nbl_fht32_wide_lds_bytes(g.q, g.maxdc), st, g, w, f, r))
}

hipError_t nbl_launch_cn_fht32_wide_layered(const NblGraphDev &g, const NblWork &w, const NblWork32 &f, const NblRun &r, const NblLayerDev &ly, int offset, int count,
                                            hipStream_t st)
{
	if (!nbl_layer_range_ok(g, offset, count) || !wide32_shape_ok(g, f) || !f.Lf) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_fht32_wide_layered_kernel<QQ>, (long long)r.B * count, 64, nbl_fht32_wide_lds_bytes(g.q, g.maxdc), st, g, w, f, r, ly, offset, count))
}
