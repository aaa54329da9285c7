// nbldpc_amd/csrc/nbl_cn_bp_inputs.h -- the input formers of the sum-product check-node programmes (bp_check_node of nbl_cn_bp_core.h,
// fht_check_node of nbl_cn_fht_core.h and their wide and single-precision forms) and, under the damped layered schedule, of the T-EMS
// programmes.  A former fills v[i] with entry lane + 64 i of edge d's incoming vector; the programmes call it once per edge, in edge
// order, by one whole wave, in their first step only.  One former per schedule, on the scalar type T of the message state: double
// (NblWork) or float (NblWork32, every operation in binary32).
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"

// the hard decision and the damping step of a scalar type; each product and the sum rounded on its own
template <int NS> __device__ __forceinline__ int input_decide(const double (&v)[NS], int lane, int q) { return wave_decide<NS>(v, lane, q); }
template <int NS> __device__ __forceinline__ int input_decide(const float (&v)[NS], int lane, int q) { return wave_decide32<NS>(v, lane, q); }
__device__ __forceinline__ double input_damp(double wo, double o, double wn, double n) { return __dadd_rn(__dmul_rn(wo, o), __dmul_rn(wn, n)); }
__device__ __forceinline__ float input_damp(float wo, float o, float wn, float n) { return __fadd_rn(__fmul_rn(wo, o), __fmul_rn(wn, n)); }

// flooding: entry lane + 64 i of edge d's v2c vector, as the variable-node pass wrote it
template <int Q, typename T = double> struct BpV2cInput {
	const T *V;      // the codeword's v2c block
	const int *epos; // the check's row of c_epos
	int lane;
	__device__ __forceinline__ void operator()(int d, T (&v)[Fld<Q>::NS]) const
	{
		const T *Vd = V + (size_t)epos[d] * Q;
#pragma unroll
		for (int i = 0; i < Fld<Q>::NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Vd[a] : T(0);
		}
	}
};

// damped layered schedule (include/nbldpc.h, nbl_create_layered_bp): input of edge j, variable n: P = L_ch[n], then + c2v of each of n's
// edges in n's order (the CURRENT values); raw = P - c2v of this edge; damped against the stored v2c of this edge where the two decide
// differently; stored back as the edge's v2c
template <int Q, typename T = double> struct BpLayeredInput {
	const T *L;      // the codeword's L_ch block
	const T *Cb;     // the codeword's c2v block (the one buffer of the layered schedule)
	T *Vb;           // the codeword's v2c block
	const int *nbr;  // NblLayerDev::nbr
	const int *epos; // NblGraphDev::c_epos
	int c0, lane;
	T damp_old, damp_new;
	__device__ __forceinline__ void operator()(int j, T (&v)[Fld<Q>::NS]) const
	{
		constexpr int NS = Fld<Q>::NS;
		const int *row = nbr + (size_t)(c0 + j) * NBL_LAYER_ROW;
		const int dv = row[1];
		const T *Ln = L + (size_t)row[0] * Q;
		const T *own = Cb + (size_t)(c0 + j) * Q;
		T *Vd = Vb + (size_t)epos[c0 + j] * Q;
		T ov[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q) ? Ln[a] : T(0);
			ov[i] = (a < Q) ? Vd[a] : T(0);
		}
		for (int d = 0; d < dv; d++) {
			const T *Cd = Cb + (size_t)row[4 + d] * Q;
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
		const int before = input_decide<NS>(ov, lane, Q);
		const int after = input_decide<NS>(v, lane, Q);
		if (before != after) {
#pragma unroll
			for (int i = 0; i < NS; i++) v[i] = input_damp(damp_old, ov[i], damp_new, v[i]);
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a == 0) v[i] = T(0);
			if (a < Q) Vd[a] = v[i];
		}
	}
};

// the formers of the single-precision FHT decoders (nbl_cn_fht32.hip, nbl_cn_fht32_wide.hip)
template <int Q> using Bp32V2cInput = BpV2cInput<Q, float>;
template <int Q> using Bp32LayeredInput = BpLayeredInput<Q, float>;
