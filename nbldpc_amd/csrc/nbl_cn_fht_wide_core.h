// nbldpc_amd/csrc/nbl_cn_fht_wide_core.h -- the FHT sum-product check-node programme of include/nbldpc.h (nbl_create_fht) in a layout
// whose register use does not grow with the check degree: what runs checks of degree 9 .. NBL_FHT_MAX_CHECK_DEGREE (nbl_cn_fht_wide.hip,
// flooding and layered).  The programme is that of nbl_cn_fht_core.h operation for operation -- the same transforms (fht<Q>), the same
// products in the same order, the same floor, the same device exp / log -- so on a check both layouts can run the two are bit-identical
// (tests/test_gpu_fht_wide.py holds them to that).  Only where U_k and Fwd_k live differs.
//
// Storage.  The register programme keeps every U_k in registers (DCM x NS doubles per lane, edge loops unrolled over DCM); here a lane
// holds three q-vectors' worth of slots (U_d, the running forward or backward product, V_d), and the edge loops are run-time loops:
//   U_d    in LDS, region d of the ONE [maxdc][Q] block: region d takes the permuted input (step 1), is read back by own slots, and is
//          overwritten by the same lanes at the same addresses with U_d; in the last pass it carries c_d for the permutation out.
//   Fwd_d  in the check's own c2v region C[d] (d >= 1).  After step 1 every read input() makes is complete and that region is dead until
//          its final store; a lane reads back exactly the addresses it wrote (slots lane + 64 i) and later stores the final c2v entries
//          lane + 64 i over them, so program order is all the ordering the scratch use needs.
// LDS is maxdc q 8 bytes as before: 64 KB at q = 256 and degree 32, what a launch gets without opting in.  DESIGN.md section 5m has the
// compiler's resource report.
//
// Contract (that of bp_check_node and fht_check_node): input(d, v) is called once per edge, in edge order, by the whole wave, and ONLY in
// step 1, before the first barrier; C ([dc][Q]) receives its final values last -- region d in the pass of edge d, after which nothing of
// this programme touches it again -- and is written by no one else meanwhile (the caller's schedule: one wave per check, the checks of a
// layer share no variable), so C may alias what input() reads.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"
#include "nbl_cn_fht_core.h"

template <int Q, class Input>
__device__ __forceinline__ void fht_wide_check_node(const NblGraphDev &g, char *smem, int c0, int dc, double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	double *S = (double *)smem; // [maxdc][Q]

	// 1. the check domain: p_d[h_d a] = in_d[a]
	for (int d = 0; d < dc; d++) {
		double v[NS];
		input(d, v);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + d], g.poly, lane);
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) S[d * Q + mh.at_slot(i)] = (a == 0) ? 0.0 : v[i];
		}
	}
	__syncthreads();
	// 2., 3. u_d = exp(p_d - max p_d), U_d = WHT(u_d) back into region d (own slots); 4. Fwd_d into C[d], Fwd_{d+1} = Fwd_d U_d
	{
		double F[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) F[i] = 0.0;
#pragma unroll 1
		for (int d = 0; d < dc; d++) {
			double U[NS];
			double m = NBL_NEG_INF;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				U[i] = (y < Q) ? S[d * Q + y] : NBL_NEG_INF;
				m = dmax(m, U[i]);
			}
			m = wave_fmax(m);
#pragma unroll
			for (int i = 0; i < NS; i++) U[i] = (lane + 64 * i < Q) ? exp(U[i] - m) : 0.0;
			fht<Q>(U, lane);
			double *Cd = C + (size_t)d * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int y = lane + 64 * i;
				if (y < Q) {
					S[d * Q + y] = U[i];              // U_d
					if (d > 0) Cd[y] = F[i];          // Fwd_d
				}
				F[i] = (d == 0) ? U[i] : F[i] * U[i]; // Fwd_{d+1}
			}
		}
	}
	// 4.-7. from the last edge down, with the running backward product
	double Bw[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) Bw[i] = 0.0;
#pragma unroll 1
	for (int d = dc - 1; d >= 0; d--) {
		double *Cd = C + (size_t)d * Q;
		double v[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int y = lane + 64 * i;
			const double f = (y < Q && d > 0) ? Cd[y] : 0.0;
			const double u = (y < Q) ? S[d * Q + y] : 0.0;
			v[i] = (d == dc - 1) ? f : (d == 0) ? Bw[i] : f * Bw[i]; // V_d
			Bw[i] = (d == dc - 1) ? u : Bw[i] * u;                   // Bwd_{d-1}: Bwd_{dc-2} = U_{dc-1}, Bwd_{k-1} = Bwd_k U_k
		}
		fht<Q>(v, lane); // 5.
		double t = NBL_NEG_INF;
#pragma unroll
		for (int i = 0; i < NS; i++)
			if (lane + 64 * i < Q) t = dmax(t, v[i]);
		t = wave_fmax(t);
		const double fl = t * (1.0 / (double)(1ull << NBL_FHT_FLOOR_LOG2)); // 6. (a power of two: exact)
#pragma unroll
		for (int i = 0; i < NS; i++) v[i] = log(dmax(v[i], fl));
		const double l0 = read_lane_f64(v[0], 0); // 7.
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
			if (a < Q) Cd[a] = (a == 0) ? 0.0 : S[d * Q + mh.at_slot(i)];
		}
	}
}
