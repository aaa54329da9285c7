// nbldpc_amd/csrc/nbl_cn_bp_inputs.h -- the input formers of the sum-product check-node programmes (bp_check_node of nbl_cn_bp_core.h,
// fht_check_node of nbl_cn_fht_core.h).  A former fills v[i] with entry lane + 64 i of edge d's incoming vector; the programmes call it
// once per edge, in edge order, by the whole wave, in their first step only.  One former per schedule, shared by the exact and the FHT
// kernels of that schedule: the same device code in both.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"

// flooding: entry lane + 64 i of edge d's v2c vector, as the variable-node pass wrote it
template <int Q> struct BpV2cInput {
	const double *V; // the codeword's v2c block
	const int *epos; // the check's row of c_epos
	int lane;
	__device__ __forceinline__ void operator()(int d, double (&v)[Fld<Q>::NS]) const
	{
		const double *Vd = V + (size_t)epos[d] * Q;
#pragma unroll
		for (int i = 0; i < Fld<Q>::NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Vd[a] : 0.0;
		}
	}
};

// damped layered schedule (include/nbldpc.h, nbl_create_layered_bp): input of edge j, variable n: P = L_ch[n], then + c2v of each of n's
// edges in n's order (the CURRENT values); raw = P - c2v of this edge; damped against the stored v2c of this edge where the two decide
// differently; stored back as the edge's v2c
template <int Q> struct BpLayeredInput {
	const double *L;  // the codeword's L_ch block
	const double *Cb; // the codeword's c2v block (the one buffer of the layered schedule)
	double *Vb;       // the codeword's v2c block
	const int *nbr;   // NblLayerDev::nbr
	const int *epos;  // NblGraphDev::c_epos
	int c0, lane;
	double damp_old, damp_new;
	__device__ __forceinline__ void operator()(int j, double (&v)[Fld<Q>::NS]) const
	{
		constexpr int NS = Fld<Q>::NS;
		const int *row = nbr + (size_t)(c0 + j) * NBL_LAYER_ROW;
		const int dv = row[1];
		const double *Ln = L + (size_t)row[0] * Q;
		const double *own = Cb + (size_t)(c0 + j) * Q;
		double *Vd = Vb + (size_t)epos[c0 + j] * Q;
		double ov[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Ln[a] : 0.0;
			ov[i] = (a < Q) ? Vd[a] : 0.0;
		}
		for (int d = 0; d < dv; d++) {
			const double *Cd = Cb + (size_t)row[4 + d] * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				if (a < Q) v[i] = v[i] + Cd[a];
			}
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) v[i] = v[i] - own[a];
		}
		const int before = wave_decide<NS>(ov, lane, Q);
		const int after = wave_decide<NS>(v, lane, Q);
		if (before != after) {
#pragma unroll
			for (int i = 0; i < NS; i++) v[i] = __dadd_rn(__dmul_rn(damp_old, ov[i]), __dmul_rn(damp_new, v[i]));
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a == 0) v[i] = 0.0;
			if (a < Q) Vd[a] = v[i];
		}
	}
};
