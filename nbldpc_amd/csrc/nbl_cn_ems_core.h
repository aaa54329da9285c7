// nbldpc_amd/csrc/nbl_cn_ems_core.h -- the EMS check-node programme of the general kernel, shared by the flooding kernel
// (nbl_kernels.hip, inputs = the v2c vectors the variable-node pass wrote) and the layered kernel (nbl_cn_layered.hip, inputs formed
// from L_ch and the in-place c2v): one wave per check, the same device code in both.
#pragma once
#include <hip/hip_runtime.h>
#include "nbl_device.h"

// ---------------------------------------------------------------------------------------------------------
// EMS check node (NBLDPC.cpp:859-917 with SortLLRVector :1715-1746 and ConstructConf :1748-1786)
//
// The reference enumerates conf(q,1) U conf(nm,nc) by recursion for every output edge.  Here the same maximum
// over the same configuration set is computed by max-plus dynamic programming over the other edges in index
// order, so every candidate value is the same left-to-right sum ((x1+x2)+x3).. (x -> fl(x+c) is monotone, so
// max and the rounded add commute).  What is NOT reproduced is the reference's running add-then-subtract
// residue.
// ---------------------------------------------------------------------------------------------------------

// Top-nm selection under SortLLRVector's order: value descending, among equal values the HIGHER symbol first.
// Wave-level quickselect on ballots: candidate sets live in scalar registers.  Returns member masks per slot and
// the rank-0 element (value + symbol).
template <int NS>
__device__ __forceinline__ void select_top(const double (&v)[NS], int lane, int q, int nm, uint64_t (&member)[NS],
                                           double &top_v, int &top_a)
{
	uint64_t valid[NS], cand[NS];
#pragma unroll
	for (int i = 0; i < NS; i++) {
		valid[i] = __ballot(lane + 64 * i < q);
		cand[i] = valid[i];
		member[i] = valid[i];
	}
	if (nm < q) {
		for (int guard = 0; guard < 4 * 64 + 8; guard++) {
			// pivot: first remaining candidate
			double pv = 0.0;
			int pa = 0;
			bool found = false;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				if (!found && cand[i]) {
					int pl = __builtin_ctzll(cand[i]);
					pv = read_lane_f64(v[i], pl);
					pa = pl + 64 * i;
					found = true;
				}
			}
			if (!found) break; // cannot happen: the nm-th element is always a candidate
			uint64_t gt[NS];
			int G = 1;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				gt[i] = __ballot(a < q && (v[i] > pv || (v[i] == pv && a > pa)));
				G += __popcll(gt[i]);
			}
			const int ps = pa >> 6;
			const uint64_t pbit = 1ull << (pa & 63);
			if (G == nm) {
#pragma unroll
				for (int i = 0; i < NS; i++) member[i] = gt[i] | ((i == ps) ? pbit : 0ull);
				break;
			}
			if (G > nm) {
#pragma unroll
				for (int i = 0; i < NS; i++) cand[i] &= gt[i];
			} else {
#pragma unroll
				for (int i = 0; i < NS; i++) cand[i] &= ~gt[i] & ~((i == ps) ? pbit : 0ull);
			}
		}
	}
	// rank 0: maximum under the same order
	double bv = -__builtin_huge_val();
	int ba = -1;
#pragma unroll
	for (int i = 0; i < NS; i++) {
		int a = lane + 64 * i;
		if (a < q && (v[i] > bv || (v[i] == bv && a > ba))) { bv = v[i]; ba = a; }
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		double ob = __shfl_xor(bv, off, 64);
		int oa = __shfl_xor(ba, off, 64);
		if (ob > bv || (ob == bv && oa > ba)) { bv = ob; ba = oa; }
	}
	top_v = uniform_f64(bv);
	top_a = uniform(ba);
}

struct EmsLds {
	double *U;   // [dc][Q]   check-domain input vectors: U[j][h_j*a] = v2c_j[a], U[j][0] = 0
	double *lv;  // [dc][nm]  values of the nm most reliable entries (rank 0 first)
	int *lt;     // [dc][nm]  their check-domain symbols
	double *A;   // [layers][Q] DP ping
	double *Bq;  // [layers][Q] DP pong
	double *Sv;  // [Q]       final configuration-set maxima of the current output edge
};

// One check of `dc` edges starting at check-major edge c0, by the calling wave (a workgroup of one wave; `smem` is its dynamic LDS,
// nbl_ems_lds_bytes).  input(j) returns a callable a -> v2c_j[a] for the symbols 1 .. Q-1 of edge j's incoming vector (slot 0 is
// taken as 0.0 and never asked for); C is where the dc outgoing vectors go, [dc][Q].  Every input is read before the first output
// is written, so C may alias what input() reads.
template <int Q, class Input>
__device__ __forceinline__ void ems_check_node(const NblGraphDev &g, const NblWork &w, const NblRun &r, int layers, char *smem, int c0, int dc,
                                               double *C, Input input)
{
	constexpr int NS = Fld<Q>::NS;
	const int lane = lane_id();
	const int nm = r.nm;
	// debug stamps (diagnostic runs only): cycles per section, summed over sampled blocks
	unsigned long long st_t0 = 0, st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	const bool st_on = (w.stamps != nullptr) && ((blockIdx.x & 63) == 0);
#define STAMP(i) do { if (st_on) { unsigned long long t1_ = clock64(); st_acc[i] += t1_ - st_t0; st_t0 = t1_; } } while (0)
	if (st_on) st_t0 = clock64();

	EmsLds s;
	s.U = (double *)smem;
	s.A = s.U + g.maxdc * Q;
	s.Bq = s.A + layers * Q;
	s.Sv = s.Bq + layers * Q;
	s.lv = s.Sv + Q;
	s.lt = (int *)(s.lv + g.maxdc * nm);

	// ---- stage the dc incoming vectors: permute into the check domain, select the nm best -----------------
	for (int j = 0; j < dc; j++) {
		const auto vj = input(j);
		GfMul<Q> mh;
		mh.init(g.c_h[c0 + j], g.poly, lane);
		double v[NS];
		int t[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			v[i] = (a < Q && a > 0) ? vj(a) : 0.0;
			t[i] = mh.at_slot(i);
			if (a < Q) s.U[j * Q + t[i]] = v[i];
		}
		uint64_t member[NS];
		double top_v;
		int top_a;
		STAMP(0);
		select_top<NS>(v, lane, Q, nm, member, top_v, top_a);
		STAMP(1);
		// compact the members into the list, rank 0 swapped to the front
		int base = 0, p0 = 0;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			if (i == (top_a >> 6)) p0 = base + __popcll(member[i] & ((1ull << (top_a & 63)) - 1ull));
			base += __popcll(member[i]);
		}
		base = 0;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if ((member[i] >> lane) & 1ull) {
				int pos = base + prefix_count(member[i]);
				if (a == top_a) pos = 0;
				else if (pos == 0) pos = p0;
				s.lv[j * nm + pos] = v[i];
				s.lt[j * nm + pos] = t[i];
			}
			base += __popcll(member[i]);
		}
		STAMP(2);
	}
	__syncthreads();

	// ---- one output edge at a time ---------------------------------------------------------------------------
	for (int x = 0; x < dc; x++) {
		// the other edges in index order: OTH(l) = l-th edge != x
#define OTH(l) ((l) + ((l) >= x ? 1 : 0))
		const int rn = dc - 1;
		int zall = 0;
		for (int l = 0; l < rn; l++) zall ^= s.lt[OTH(l) * nm];

		double S[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) S[i] = -NBL_DBL_MAX;

		// conf(q,1): at most one edge deviates, to ANY symbol (:894)
		for (int pi = 0; pi < rn; pi++) {
			const int jd = OTH(pi);
			const int shift = zall ^ s.lt[jd * nm];
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int sym = lane + 64 * i;
				if (sym < Q) {
					double u = s.U[jd * Q + (sym ^ shift)];
					double acc = 0.0;
					for (int l = 0; l < rn; l++) acc = acc + ((l == pi) ? u : s.lv[OTH(l) * nm]);
					S[i] = dmax(S[i], acc);
				}
			}
		}

		STAMP(3);
		// conf(nm,nc): at most nc edges deviate, each inside its nm best (:897); conf(nm,0) is the all-rank-0 configuration alone,
		// which conf(q,1) already holds
		if (r.nc < 1) {
		} else if (layers == 1) {
			// nc >= dc-1: no deviation counting needed -> plain truncated max-plus convolution
			double *A = s.A, *Bq = s.Bq;
			__syncthreads();
			for (int sidx = lane; sidx < Q; sidx += 64) A[sidx] = NBL_NEG_INF;
			__syncthreads();
			if (rn == 1) {
				const int j1 = OTH(0);
				for (int k = lane; k < nm; k += 64) A[s.lt[j1 * nm + k]] = 0.0 + s.lv[j1 * nm + k];
			} else {
				const int j1 = OTH(0), j2 = OTH(1);
				for (int idx = lane; idx < nm * nm; idx += 64) {
					int k1 = idx / nm, k2 = idx - k1 * nm;
					double val = (0.0 + s.lv[j1 * nm + k1]) + s.lv[j2 * nm + k2];
					__hip_atomic_fetch_max(&A[s.lt[j1 * nm + k1] ^ s.lt[j2 * nm + k2]], val, __ATOMIC_RELAXED,
					                       __HIP_MEMORY_SCOPE_WORKGROUP);
				}
			}
			__syncthreads();
			STAMP(4);
			for (int l = 2; l < rn; l++) {
				const int jl = OTH(l);
				double acc[NS];
#pragma unroll
				for (int i = 0; i < NS; i++) acc[i] = NBL_NEG_INF;
				for (int k = 0; k < nm; k++) {
					const int tk = uniform(s.lt[jl * nm + k]);
					const double vk = s.lv[jl * nm + k];
#pragma unroll
					for (int i = 0; i < NS; i++) {
						int sym = lane + 64 * i;
						if (sym < Q) acc[i] = dmax(acc[i], A[sym ^ tk] + vk);
					}
				}
				if (l == rn - 1) {
#pragma unroll
					for (int i = 0; i < NS; i++) S[i] = dmax(S[i], acc[i]);
				} else {
#pragma unroll
					for (int i = 0; i < NS; i++) {
						int sym = lane + 64 * i;
						if (sym < Q) Bq[sym] = acc[i];
					}
					__syncthreads();
					double *T = A; A = Bq; Bq = T;
				}
			}
			if (rn <= 2) {
#pragma unroll
				for (int i = 0; i < NS; i++) {
					int sym = lane + 64 * i;
					if (sym < Q) S[i] = dmax(S[i], A[sym]);
				}
			}
		} else {
			// layered DP: A[d][s] = best value reaching check sum s with exactly d deviations
			double *A = s.A, *Bq = s.Bq;
			__syncthreads();
			for (int idx = lane; idx < layers * Q; idx += 64) A[idx] = (idx == 0) ? 0.0 : NBL_NEG_INF;
			__syncthreads();
			for (int l = 0; l < rn; l++) {
				const int jl = OTH(l);
				const int z = s.lt[jl * nm];
				const double mz = s.lv[jl * nm];
				for (int d = 0; d < layers; d++) {
					double acc[NS];
#pragma unroll
					for (int i = 0; i < NS; i++) {
						int sym = lane + 64 * i;
						acc[i] = (sym < Q) ? A[d * Q + (sym ^ z)] + mz : NBL_NEG_INF;
					}
					if (d >= 1) {
						for (int k = 1; k < nm; k++) {
							const int tk = uniform(s.lt[jl * nm + k]);
							const double vk = s.lv[jl * nm + k];
#pragma unroll
							for (int i = 0; i < NS; i++) {
								int sym = lane + 64 * i;
								if (sym < Q) acc[i] = dmax(acc[i], A[(d - 1) * Q + (sym ^ tk)] + vk);
							}
						}
					}
#pragma unroll
					for (int i = 0; i < NS; i++) {
						int sym = lane + 64 * i;
						if (sym < Q) Bq[d * Q + sym] = acc[i];
					}
				}
				__syncthreads();
				double *T = A; A = Bq; Bq = T;
			}
			for (int d = 0; d < layers; d++) {
#pragma unroll
				for (int i = 0; i < NS; i++) {
					int sym = lane + 64 * i;
					if (sym < Q) S[i] = dmax(S[i], A[d * Q + sym]);
				}
			}
		}

		STAMP(5);
		// ---- output: c2v[a] = shape(S[h_x a] - S[0]) (:899-916) ----------------------------------------------
		double *Sv = s.Sv;
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int sym = lane + 64 * i;
			if (sym < Q) Sv[sym] = S[i];
		}
		__syncthreads();
		{
			GfMul<Q> mh;
			mh.init(g.c_h[c0 + x], g.poly, lane);
			const double s0 = Sv[0];
			double *Cx = C + (size_t)x * Q;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				if (a < Q) Cx[a] = (a == 0) ? 0.0 : shape_llr(Sv[mh.at_slot(i)] - s0, r.factor, r.offset);
			}
		}
#undef OTH
		STAMP(6);
	}
	if (st_on && lane == 0) {
		for (int i = 0; i < 8; i++) atomicAdd(&w.stamps[i], st_acc[i]);
		atomicAdd(&w.stamps[15], 1ull);
	}
#undef STAMP
}
