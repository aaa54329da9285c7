// nbldpc_amd/csrc/nbl_cn_bp_layered.hip -- log-QSPA under the damped layered (check-serial) schedule of include/nbldpc.h
// (nbl_create_layered_bp).
//
// One iteration is: vn_decide_kernel and syn_kernel (as for layered EMS and T-EMS), then ONE launch of cn_bp_layered_kernel per layer.
// A check of layer l forms the raw input of each of its edges from L_ch and the c2v buffer as the layers before it left it, damps it
// against the edge's stored v2c vector (the reference's per-edge damping, NBLDPC.cpp:730-741: where the hard decisions of the two
// differ, 0.5 old + 0.5 new), stores the result back as the edge's v2c, runs the log-QSPA check-node programme of the general kernel
// (nbl_cn_bp_core.h: the same device code) on it and writes its c2v vectors back into the same buffer.
//
// What makes one c2v and one v2c buffer enough:
//   * every global read of a check's inputs (L_ch, the neighbours' c2v, its own c2v, its stored v2c) happens in the first step of the
//     programme, which moves all dc inputs into LDS before its first convolution, and is complete before the check's first c2v store
//     in the programme's last step;
//   * the checks of a layer share no variable, so no wave of a launch reads a c2v vector that another wave of that launch writes;
//   * an edge belongs to one check, so its v2c vector is read and written by that check's wave alone;
//   * the launches of one stream order the layers.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_bp_core.h"
#include "nbl_cn_bp_inputs.h"

// the checks of one layer: one wave per (codeword, check)
template <int Q>
__global__ __launch_bounds__(64) void cn_bp_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const BpLayeredInput<Q> input = {w.Lch + (size_t)k.b * g.N * Q, Cb, w.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), r.damp_old, r.damp_new};
	bp_check_node<Q>(g, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

hipError_t nbl_launch_cn_bp_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	// (3 maxdc + 5) q 8 bytes: 59,392 B at q = 256 and degree 8, the largest the ABI accepts -- below the 64 KB a kernel has unasked
	const size_t lds = nbl_bp_lds_bytes(g.q, g.maxdc);
	if (!nbl_layer_range_ok(g, offset, count) || lds > NBL_LDS_OPT_IN || !w.v2c) return hipErrorInvalidValue;
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_bp_layered_kernel<QQ>, (long long)r.B * count, 64, lds, st, g, w, r, ly, offset, count))
}
