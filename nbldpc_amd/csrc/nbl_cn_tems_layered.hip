// nbldpc_amd/csrc/nbl_cn_tems_layered.hip -- T-EMS under the damped layered (check-serial) schedule of include/nbldpc.h
// (nbl_create_layered_ex with NBL_LAYERED_DAMPED).
//
// One iteration is: vn_decide_kernel and syn_kernel (as for layered EMS), then ONE launch of cn_tems_layered_kernel per layer.  A
// check of layer l forms the raw input of each of its edges from L_ch and the c2v buffer as the layers before it left it, damps it
// against the edge's stored v2c vector (the reference's per-edge damping, NBLDPC.cpp:1029-1052: where the hard decisions of the two
// differ, 0.25 old + 0.75 new), stores the result back as the edge's v2c (BpLayeredInput, nbl_cn_bp_inputs.h), runs the T-EMS
// check-node programme of the general kernels (nbl_cn_tems_core.h: the same device code) on it and writes its c2v vectors back into
// the same buffer.
//
// What makes one c2v and one v2c buffer enough:
//   * every global read of a check's inputs (L_ch, the neighbours' c2v, its own c2v, its stored v2c) happens in step 1 of the
//     programme and is complete, in registers or LDS, before the check's first c2v store in step 4;
//   * the checks of a layer share no variable, so no wave of a launch reads a c2v vector that another wave of that launch writes;
//   * an edge belongs to one check, so its v2c vector is read and written by that check's wave alone;
//   * the launches of one stream order the layers.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_tems_core.h"
#include "nbl_cn_bp_inputs.h"

// the checks of one layer: one wave per (codeword, check)
template <int Q, bool FAST>
__global__ __launch_bounds__(64) void cn_tems_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const BpLayeredInput<Q> input = {w.Lch + (size_t)k.b * g.N * Q, Cb, w.v2c + (size_t)k.b * g.E * Q, ly.nbr, g.c_epos, k.c0, lane_id(), r.damp_old, r.damp_new};
	if (FAST) tems_fast_check_node<Q>(g, r, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
	else tems_check_node<Q>(g, r, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, input);
}

size_t nbl_tems_layered_lds_bytes(int q, int maxdc, int nc)
{
	// (the general programme's size decides what is refused; the fast programme, taken for nc <= 3, must fit as well)
	const size_t gen = nbl_tems_lds_bytes((size_t)q, (size_t)maxdc, nc), fast = nc <= 3 ? nbl_tems_fast_lds_bytes((size_t)q, (size_t)maxdc) : 0;
	return gen > fast ? gen : fast;
}

hipError_t nbl_launch_cn_tems_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const bool fast = nbl_tems_use_fast(r.nc);
	const size_t lds = fast ? nbl_tems_fast_lds_bytes(g.q, g.maxdc) : nbl_tems_lds_bytes(g.q, g.maxdc, r.nc);
	if (!nbl_layer_range_ok(g, offset, count) || lds > NBL_MAX_LDS) return hipErrorInvalidValue; // (nbl_create_layered_ex refuses such shapes)
	if ((double)g.p * g.maxdc > 32.0) return hipErrorInvalidValue; // path code must fit 32 bits (refused at creation)
	if (!w.v2c) return hipErrorInvalidValue;
	const long long blocks = (long long)r.B * count;
	if (fast) { NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_tems_layered_kernel<QQ, true>, blocks, 64, lds, st, g, w, r, ly, offset, count)) }
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_tems_layered_kernel<QQ, false>, blocks, 64, lds, st, g, w, r, ly, offset, count))
}
