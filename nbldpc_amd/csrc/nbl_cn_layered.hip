// nbldpc_amd/csrc/nbl_cn_layered.hip -- EMS under the layered (check-serial) schedule of include/nbldpc.h (nbl_create_layered).
//
// One iteration is: vn_decide_kernel (a-posteriori sum and hard decision of every variable; no v2c is written), syn_kernel
// (nbl_kernels.hip, unchanged), then ONE launch of cn_ems_layered_kernel per layer.  A check of layer l forms its own inputs from
// L_ch and the c2v buffer as the layers before it left it, runs the EMS check-node programme of the general kernel
// (nbl_cn_ems_core.h: the same device code) and writes its c2v vectors back into the same buffer.  The checks of a layer share no
// variable, so no wave of a launch reads what another wave of that launch writes; the launches of one stream order the layers.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_ems_core.h"

// ---------------------------------------------------------------------------------------------------------
// tentative decision: L_post = L_ch + c2v_0 + c2v_1 ... in the variable's edge order, DecideLLRVector (NBLDPC.cpp:808-823); the
// variable-node pass of nbl_kernels.hip without its v2c half.  One wave per (codeword, variable).
// ---------------------------------------------------------------------------------------------------------
template <int Q>
__global__ __launch_bounds__(256) void vn_decide_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	const long long node = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (node >= (long long)r.B * g.N) return;
	const int b = nbl_codeword(w, r, (int)(node / g.N)), n = (int)(node % g.N);
	if (b < 0) return;
	if (!r.fixed_iters && w.done[b]) return;

	const int e0 = g.voff[n], dv = g.voff[n + 1] - e0;
	const double *L = w.Lch + ((size_t)b * g.N + n) * Q;
	const double *C = w.c2v + (size_t)b * g.E * Q;
	double post[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) {
		int a = lane + 64 * i;
		post[i] = (a < Q) ? L[a] : 0.0;
	}
	for (int d = 0; d < dv; d++) {
		const double *Cd = C + (size_t)g.v_cpos[e0 + d] * Q;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) post[i] = post[i] + Cd[a];
		}
	}
	int dec = wave_decide<NS>(post, lane, Q);
	if (lane == 0) w.dec[(size_t)b * g.N + n] = dec;
	if (w.post) {
		double *P = w.post + ((size_t)b * g.N + n) * Q;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) P[a] = post[i];
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// the checks of one layer: one wave per (codeword, check); grid = count * (codeword slots)
// ---------------------------------------------------------------------------------------------------------
template <int Q>
__global__ __launch_bounds__(64) void cn_ems_layered_kernel(NblGraphDev g, NblWork w, NblRun r, NblLayerDev ly, int offset, int count, int layers)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_layer_codeword(w, r, count);
	if (b < 0) return;
	const NblCheck k = nbl_layer_check(g, ly, offset, count, b);
	double *Cb = w.c2v + (size_t)k.b * g.E * Q;
	const EmsLayeredInput<Q> in = {w.Lch + (size_t)k.b * g.N * Q, Cb, ly.nbr, k.c0}; // (nbl_cn_shell.h)
	ems_check_node<Q>(g, w, r, layers, smem, k.c0, k.dc, Cb + (size_t)k.c0 * Q, in);
}

hipError_t nbl_launch_vn_decide(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const long long nodes = (long long)r.B * g.N;
	dim3 grid((unsigned)((nodes + 3) / 4)), block(256);
	NBL_DISPATCH_Q(g.q, vn_decide_kernel<QQ><<<grid, block, 0, st>>>(g, w, r))
	return hipGetLastError();
}

hipError_t nbl_launch_cn_ems_layered(const NblGraphDev &g, const NblWork &w, const NblRun &r, const NblLayerDev &ly, int offset, int count, hipStream_t st)
{
	const int layers = nbl_ems_layers(g.maxdc, r.nc);
	const size_t lds = nbl_ems_lds_bytes(g.q, g.maxdc, r.nm, r.nc);
	if (!nbl_layer_range_ok(g, offset, count) || lds > NBL_MAX_LDS) return hipErrorInvalidValue; // (nbl_create_layered refuses such shapes)
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_ems_layered_kernel<QQ>, (long long)r.B * count, 64, lds, st, g, w, r, ly, offset, count, layers))
}
