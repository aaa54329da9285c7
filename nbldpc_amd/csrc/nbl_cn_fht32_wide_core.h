// nbldpc_amd/csrc/nbl_cn_fht32_wide_core.h -- the single-precision FHT sum-product check-node programme of include/nbldpc.h
// (nbl_create_fht32_wide) for checks of degree 9 .. NBL_FHT32_MAX_CHECK_DEGREE, shared by the flooding and the layered kernel of
// nbl_cn_fht32_wide.hip: one wave per check, the same device code in both.
//
// It is the programme of nbl_cn_fht32_core.h operation for operation -- the same transforms (fht32<Q>), the same products in the same
// order, the same floor, the same device expf / logf -- with ONE step added, and in the storage scheme of nbl_cn_fht_wide_core.h.
//
// Step 3a (range).  |U_d[y]| <= U_d[0] <= q, so a product of 31 transformed vectors can reach q^31 = 2^248 at GF(256), and a flat input
// (the all-zero channel vector of a punctured symbol) makes U_d[0] = q exactly: unscaled, degree 32 leaves binary32's range in the
// ordinary case.  U_d[0] = sum_y u_d[y] >= 1 (one u is exactly 1, none is negative), so there is an integer e_d in 0 .. log2 q with
// 2^e_d <= U_d[0] < 2^(e_d+1); every slot of U_d is multiplied by 2^-e_d.  Then |U_d[y]| < 2, a product of up to 31 stays below 2^31,
// its transform below 2^39, and t >= 1: sum_y v_d[y] = q V_d[0], so the largest v_d is at least V_d[0], a product of slot 0s in [1, 2).
// The scale is a power of two: exact unless a value is subnormal; it multiplies every v_d by one factor, which the difference of logs in
// step 7 removes, and the floor of step 6 is relative to the vector's own largest.  A scaled and an unscaled evaluation of one check
// differ only in how logf rounds a scaled argument, so this programme and the register programme are not bit-identical on a code both
// run; each carries the parity statement against its own restatement (tests/fht32_wide_ref.py, tests/fht32_ref.py).
//
// Storage (that of nbl_cn_fht_wide_core.h, on floats).  A lane holds three q-vectors' worth of slots (U_d, the running forward or
// backward product, V_d); the edge loops are run-time loops:
//   U_d    in LDS, region d of the ONE [maxdc][Q] float block: region d takes the permuted input (step 1), is read back by own slots, and
//          is overwritten by the same lanes at the same addresses with the scaled U_d; in the last pass it carries c_d for the permutation
//          out.
//   Fwd_d  in the check's own float c2v region C[d] (d >= 1).  After step 1 every read input() makes is complete and that region is dead
//          until its final store; a lane reads back exactly the addresses it wrote (slots lane + 64 i) and later stores the final c2v
//          entries lane + 64 i over them, so program order is all the ordering the scratch use needs.
// LDS is maxdc q 4 bytes (nbl_fht32_wide_lds_bytes): 32 KB at q = 256 and degree 32.  DESIGN.md section 5r has the compiler's resource
// report.
//
// Contract (that of fht_wide_check_node): input(d, v) is called once per edge, in edge order, by the whole wave, and ONLY in step 1,
// before the first barrier; C ([dc][Q]) receives its final values last -- region d in the pass of edge d, after which nothing of this
// programme touches it again -- and is written by no one else meanwhile (the caller's schedule: one wave per check, the checks of a layer
// share no variable), so C may alias what input() reads.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_cn_fht32_core.h"

inline size_t nbl_fht32_wide_lds_bytes(size_t q, size_t mdc) { return mdc * q * 4; }

// 2^-e for the e with 2^e <= x < 2^(e+1); x normal and in [1, 2^127) (here [1, q]): both exponents taken and made as bits
__device__ __forceinline__ float fht32_pow2_below_inv(float x)
{
	const unsigned biased = (__float_as_uint(x) >> 23) & 0xffu; // 127 + e
	return __uint_as_float((254u - biased) << 23);              // 127 - e
}

template <int Q, class Input>
__device__ __forceinline__ void fht32_wide_check_node(const NblGraphDev &g, char *smem, int c0, int dc, float *C, Input input)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	float *S = (float *)smem; // [maxdc][Q]

	// 1. the check domain: p_d[h_d a] = in_d[a]
	for (int d = 0; d < dc; d++) {
		float v[NS];
		input(d, v);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) S[d * Q + mh.at_slot(i)] = (a == 0) ? 0.0f : v[i];
		}
	}
	__syncthreads();
	// 2., 3. u_d = exp(p_d - max p_d), U_d = WHT(u_d); 3a. U_d <- U_d 2^-e_d, back into region d (own slots); 4. Fwd_d into C[d],
	// Fwd_{d+1} = Fwd_d U_d
	{
		float F[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) F[i] = 0.0f;
#pragma unroll 1
		for (int d = 0; d < dc; d++) {
			float U[NS];
			float m = NBL_NEG_INF_F;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				U[i] = (y < Q) ? S[d * Q + y] : NBL_NEG_INF_F;
				m = fmax32(m, U[i]);
			}
			m = wave_fmax32(m);
#pragma unroll
			for (int i = 0; i < NS; i++) U[i] = (lane + 64 * i < Q) ? expf(U[i] - m) : 0.0f;
			fht32<Q>(U, lane);
			const float sc = fht32_pow2_below_inv(read_lane_f32(U[0], 0)); // slot 0 of U_d: U[0] in lane 0
			float *Cd = C + (size_t)d * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				U[i] = U[i] * sc;
				if (y < Q) {
					S[d * Q + y] = U[i];              // U_d
					if (d > 0) Cd[y] = F[i];          // Fwd_d
				}
				F[i] = (d == 0) ? U[i] : F[i] * U[i]; // Fwd_{d+1}
			}
		}
	}
	// 4.-7. from the last edge down, with the running backward product
	float Bw[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) Bw[i] = 0.0f;
#pragma unroll 1
	for (int d = dc - 1; d >= 0; d--) {
		float *Cd = C + (size_t)d * Q;
		float v[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int y = lane + 64 * i;
			const float f = (y < Q && d > 0) ? Cd[y] : 0.0f;
			const float u = (y < Q) ? S[d * Q + y] : 0.0f;
			v[i] = (d == dc - 1) ? f : (d == 0) ? Bw[i] : f * Bw[i]; // V_d
			Bw[i] = (d == dc - 1) ? u : Bw[i] * u;                   // Bwd_{d-1}: Bwd_{dc-2} = U_{dc-1}, Bwd_{k-1} = Bwd_k U_k
		}
		fht32<Q>(v, lane); // 5.
		float t = NBL_NEG_INF_F;
#pragma unroll
		for (int i = 0; i < NS; i++)
			if (lane + 64 * i < Q) t = fmax32(t, v[i]);
		t = wave_fmax32(t);
		const float fl = t * (1.0f / (float)(1u << NBL_FHT32_FLOOR_LOG2)); // 6. (a power of two: exact)
#pragma unroll
		for (int i = 0; i < NS; i++) v[i] = logf(fmax32(v[i], fl));
		const float l0 = read_lane_f32(v[0], 0); // 7.
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int y = lane + 64 * i;
			if (y < Q) S[d * Q + y] = v[i] - l0;
		}
		__syncthreads();
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) Cd[a] = (a == 0) ? 0.0f : S[d * Q + mh.at_slot(i)];
		}
	}
}
