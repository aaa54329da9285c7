// nbldpc_amd/csrc/nbl_cn_shell.h -- what the per-check check-node kernels share around their programmes ("the
// shell"): which check a workgroup runs, the undamped EMS-shaped input formers, and on the host the range checks and the launch.  A
// family writes its programme (nbl_cn_*_core.h), its shape_ok and its LDS size; the rest is here, in nbl_cn_bp_inputs.h (the damped
// formers) and in nbl_kernels.h (NBL_DISPATCH_Q, the LDS constants).  The fused kernels (XCD-aware slots) have prologues of their own.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_kernels.h"

// ---------------------------------------------------------------------------------------------------------
// device: the check of this workgroup, in two steps.  First the codeword: -1 = nothing to do (a slot beyond the batch or the active
// list, or a codeword that stopped early) and the kernel returns, as a whole workgroup, before its first barrier.  Then the check's
// edges.  Two steps, not one call that hands back both: a helper that also loads c0 and dc on its live path leaves the kernel a join
// that carries loaded values in front of its return, and hipcc does not thread that join away -- cn_ems_wide_kernel<64> measured 1.7 %
// slower that way at equal registers, cn_bstems_kernel grew by a sixth.  This form compiles to the prologue as each kernel used to
// write it out: the same order of loads and exits, the same registers.
// ---------------------------------------------------------------------------------------------------------
struct NblCheck { int b, c0, dc; }; // codeword; first check-major edge and degree of the check

__device__ __forceinline__ int nbl_live_codeword(const NblWork &w, const NblRun &r, int slot)
{
	const int b = nbl_codeword(w, r, slot);
	if (b < 0) return -1;
	if (!r.fixed_iters && w.done[b]) return -1;
	return b;
}
__device__ __forceinline__ NblCheck nbl_check_at(const NblGraphDev &g, int b, int m)
{
	const int c0 = g.coff[m];
	return {b, c0, g.coff[m + 1] - c0};
}
// flooding: grid = M * (codeword slots)
__device__ __forceinline__ int nbl_flooding_codeword(const NblGraphDev &g, const NblWork &w, const NblRun &r) { return nbl_live_codeword(w, r, blockIdx.x / g.M); }
__device__ __forceinline__ NblCheck nbl_flooding_check(const NblGraphDev &g, int b) { return nbl_check_at(g, b, blockIdx.x % g.M); }
// the checks chk[offset] .. chk[offset + count - 1] of one layer: grid = count * (codeword slots)
__device__ __forceinline__ int nbl_layer_codeword(const NblWork &w, const NblRun &r, int count) { return nbl_live_codeword(w, r, blockIdx.x / count); }
__device__ __forceinline__ NblCheck nbl_layer_check(const NblGraphDev &g, const NblLayerDev &ly, int offset, int count, int b)
{
	return nbl_check_at(g, b, ly.chk[offset + blockIdx.x % count]);
}

// ---------------------------------------------------------------------------------------------------------
// device: the input formers of the EMS-shaped programmes (ems_check_node, ems_wide_check_node, minmax_check_node): input(j) returns
// the callable a -> entry a of edge j's incoming vector
// ---------------------------------------------------------------------------------------------------------
// flooding: the v2c vector the variable-node pass wrote
template <int Q> struct EmsV2cInput {
	const double *V; // the codeword's v2c block
	const int *epos; // NblGraphDev::c_epos
	int c0;
	__device__ __forceinline__ auto operator()(int j) const
	{
		const double *Vj = V + (size_t)epos[c0 + j] * Q;
		return [=](int a) { return Vj[a]; };
	}
};

// layered (include/nbldpc.h): input of edge j, variable n: P = L_ch[n], then + c2v of each of n's edges in n's order (the CURRENT
// values), then - c2v of this edge; the row gives every address after one index load
template <int Q> struct EmsLayeredInput {
	const double *L;  // the codeword's L_ch block
	const double *Cb; // the codeword's c2v block (the one buffer of the layered schedule)
	const int *nbr;   // NblLayerDev::nbr
	int c0;
	__device__ __forceinline__ auto operator()(int j) const
	{
		const int *row = nbr + (size_t)(c0 + j) * NBL_LAYER_ROW;
		const int dv = row[1];
		const double *Ln = L + (size_t)row[0] * Q;
		const double *own = Cb + (size_t)(c0 + j) * Q;
		const double *nb[NBL_MAXDV];
#pragma unroll
		for (int d = 0; d < NBL_MAXDV; d++) nb[d] = Cb + (size_t)row[4 + (d < dv ? d : 0)] * Q;
		return [=](int a) {
			double P = Ln[a];
#pragma unroll
			for (int d = 0; d < NBL_MAXDV; d++)
				if (d < dv) P = P + nb[d][a];
			return P - own[a];
		};
	}
};

// ---------------------------------------------------------------------------------------------------------
// host: the layer range; the launch (one instantiation per q: NBL_DISPATCH_Q of nbl_kernels.h)
// ---------------------------------------------------------------------------------------------------------
inline bool nbl_layer_range_ok(const NblGraphDev &g, int offset, int count) { return count >= 1 && offset >= 0 && offset + count <= g.M; }

// `blocks` workgroups of `threads` with `lds` bytes of dynamic LDS (the caller has refused lds > NBL_MAX_LDS)
template <typename... Params, typename... Args>
inline hipError_t nbl_launch_checks(void (*kernel)(Params...), long long blocks, int threads, size_t lds, hipStream_t st, const Args &...args)
{
	if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
	if (lds > NBL_LDS_OPT_IN) (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	kernel<<<dim3((unsigned)blocks), dim3(threads), lds, st>>>(args...);
	return hipGetLastError();
}
