// nbldpc_amd/csrc/nbl_cn_fht32_inputs.h -- how a check of the single-precision FHT decoders forms its inputs, shared by the register
// programme (nbl_cn_fht32.hip) and the wide one (nbl_cn_fht32_wide.hip): the two formers of nbl_cn_bp_inputs.h on the float state.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_cn_fht32_core.h"

// flooding: entry lane + 64 i of edge d's v2c vector (BpV2cInput of nbl_cn_bp_inputs.h on floats)
template <int Q> struct Bp32V2cInput {
	const float *V;  // the codeword's v2c block
	const int *epos; // the check's row of c_epos
	int lane;
	__device__ __forceinline__ void operator()(int d, float (&v)[Fld<Q>::NS]) const
	{
		const float *Vd = V + (size_t)epos[d] * Q;
#pragma unroll
		for (int i = 0; i < Fld<Q>::NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Vd[a] : 0.0f;
		}
	}
};

// damped layered schedule (BpLayeredInput on floats): input of edge j, variable n: P = Lf[n], then + c2v of each of n's edges in n's
// order (the CURRENT values); raw = P - c2v of this edge; damped 0.5 / 0.5 against the stored v2c of this edge where the two decide
// differently; stored back as the edge's v2c.  Every operation in binary32.
template <int Q> struct Bp32LayeredInput {
	const float *L;  // the codeword's Lf block
	const float *Cb; // the codeword's c2v block
	float *Vb;       // the codeword's v2c block
	const int *nbr;  // NblLayerDev::nbr
	const int *epos; // NblGraphDev::c_epos
	int c0, lane;
	float damp_old, damp_new;
	__device__ __forceinline__ void operator()(int j, float (&v)[Fld<Q>::NS]) const
	{
		constexpr int NS = Fld<Q>::NS;
		const int *row = nbr + (size_t)(c0 + j) * NBL_LAYER_ROW;
		const int dv = row[1];
		const float *Ln = L + (size_t)row[0] * Q;
		const float *own = Cb + (size_t)(c0 + j) * Q;
		float *Vd = Vb + (size_t)epos[c0 + j] * Q;
		float ov[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Ln[a] : 0.0f;
			ov[i] = (a < Q) ? Vd[a] : 0.0f;
		}
		for (int d = 0; d < dv; d++) {
			const float *Cd = Cb + (size_t)row[4 + d] * Q;
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
		const int before = wave_decide32<NS>(ov, lane, Q);
		const int after = wave_decide32<NS>(v, lane, Q);
		if (before != after) {
#pragma unroll
			for (int i = 0; i < NS; i++) v[i] = __fadd_rn(__fmul_rn(damp_old, ov[i]), __fmul_rn(damp_new, v[i]));
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a == 0) v[i] = 0.0f;
			if (a < Q) Vd[a] = v[i];
		}
	}
};
