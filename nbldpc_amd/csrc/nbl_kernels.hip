// nbldpc_amd/csrc/nbl_kernels.hip -- HIP kernels of the NB-LDPC message-passing iteration for gfx950.
//
// One iteration of the reference's flooding schedule (NBLDPC.cpp:673-768 / 805-919 / 973-1131) is three launches:
//   vn_kernel   one wave per (codeword, variable): a-posteriori sum, hard decision, variable-to-check messages
//   syn_kernel  one wave per codeword: syndrome over GF(q), first-zero-syndrome freeze of the output
//   cn_*_kernel one wave per (codeword, check): check-node update (EMS / T-EMS / log-QSPA)
// Everything is FP64 and every floating-point expression keeps the reference's association order; the file
// is compiled with -ffp-contract=off so no multiply-add is fused.
#include <hip/hip_runtime.h>
#include "nbl_cn_shell.h"
#include "nbl_cn_ems_core.h"

// ---------------------------------------------------------------------------------------------------------
// init: host/API layout [B][N][q-1] -> padded [B][N][q] with slot 0 = 0.0; clear c2v; v2c = L_ch
// (NBLDPC.cpp:649-662 / 781-794 / 934-969)
// ---------------------------------------------------------------------------------------------------------
// write_v2c bit 0: also v2c = L_ch (damped methods read it); bit 1: leave c2v alone (fused iterations read the zeros of
// iteration 0 from a buffer of their own); bit 2: L_ch is already padded (init_rows_kernel)
__global__ void init_kernel(const double *__restrict__ Lin, NblGraphDev g, NblWork w, int B, int write_v2c)
{
	const int q = g.q;
	long long total = (long long)B * g.N * q;
	if (Lin && !(write_v2c & 4)) // else: demod_kernel or init_rows_kernel has already filled Lch
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
			int a = (int)(i % q);
			long long bn = i / q;
			w.Lch[i] = a ? Lin[bn * (q - 1) + (a - 1)] : 0.0;
		}
	long long etotal = (long long)B * g.E * q;
	if (!(write_v2c & 2))
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < etotal; i += (long long)gridDim.x * blockDim.x)
			w.c2v[i] = 0.0;
	if (write_v2c & 1) {
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < etotal; i += (long long)gridDim.x * blockDim.x) {
			int a = (int)(i % q);
			long long be = i / q;
			int e = (int)(be % g.E);
			long long b = be / g.E;
			// variable of edge e: binary search in voff
			int lo = 0, hi = g.N;
			while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (g.voff[mid] <= e) lo = mid; else hi = mid; }
			w.v2c[i] = a ? (Lin ? Lin[(b * g.N + lo) * (q - 1) + (a - 1)] : w.Lch[(b * g.N + lo) * q + a]) : 0.0;
		}
	}
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (long long)gridDim.x * blockDim.x) {
		w.done[i] = 0;
		w.iters[i] = 0;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) *w.n_done = 0;
}

// The L_ch part of init for q >= 64, row by row: Q / 2 lanes (at most a wave) take one (codeword, variable) row, each lane two
// neighbouring symbols per pass -- 8-byte loads (a [q-1] row is only 8-byte aligned), one 16-byte store, slot 0 = 0.0 -- and a wave
// carries ROWS such row groups with every load issued before the first store.  No division per element: the row comes from the wave's
// index.  flags: 1 = also done / iters / n_done (then init_kernel has nothing left to do on the fused undamped path).
template <int Q, int ROWS>
__global__ __launch_bounds__(256) void init_rows_kernel(const double *__restrict__ Lin, double *__restrict__ Lch, long long rows, NblWork w, int B, int flags)
{
	constexpr int LPR = (Q / 2 < 64) ? Q / 2 : 64; // lanes per row
	constexpr int RPW = 64 / LPR;                  // rows side by side in a wave
	constexpr int P = Q / (2 * LPR);               // passes over a row
	const int lane = lane_id(), sub = lane / LPR, ll = lane % LPR;
	const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const long long row0 = wave * (ROWS * RPW) + sub;
	double2 val[ROWS][P];
#pragma unroll
	for (int k = 0; k < ROWS; k++) {
		const long long row = row0 + (long long)k * RPW;
		if (row < rows) {
			const double *src = Lin + (size_t)row * (Q - 1);
#pragma unroll
			for (int p = 0; p < P; p++) {
				const int a = 2 * ll + 2 * LPR * p; // symbols a, a + 1 <= Q - 1
				val[k][p].x = a ? src[a - 1] : 0.0;
				val[k][p].y = src[a];
			}
		}
	}
#pragma unroll
	for (int k = 0; k < ROWS; k++) {
		const long long row = row0 + (long long)k * RPW;
		if (row < rows) {
			double2 *dst = (double2 *)(Lch + (size_t)row * Q);
#pragma unroll
			for (int p = 0; p < P; p++) dst[ll + LPR * p] = val[k][p];
		}
	}
	if (flags & 1) {
		for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < B; i += (long long)gridDim.x * blockDim.x) {
			w.done[i] = 0;
			w.iters[i] = 0;
		}
		if (blockIdx.x == 0 && threadIdx.x == 0) *w.n_done = 0;
	}
}

// ---------------------------------------------------------------------------------------------------------
// soft demodulator: received samples -> symbol LLRs, written straight into the padded Lch layout.
// Expression order is CComm::Demodulate's (Comm.cpp:356, :364-378 for BPSK; :394-395 for q-ary constellations).
// ---------------------------------------------------------------------------------------------------------
// GAIN (include/nbldpc.h, "demodulators with gains"): gain [B][L][2], BPSK takes z = hr re + hi im in place of re,
// the q-ary path the faded points of its sample in place of the table's.  The instance without GAIN is the kernel the gain-less calls
// have always launched.
template <bool GAIN>
__global__ __launch_bounds__(256) void demod_kernel(const double *__restrict__ rx, int L, double sigma_n, int mod_order, int p,
                                                    const double *__restrict__ cons, const int *__restrict__ src, NblGraphDev g,
                                                    NblWork w, int B, const double *__restrict__ gain)
{
	const int lane = lane_id();
	const long long node = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (node >= (long long)B * g.N) return;
	const int b = (int)(node / g.N), n = (int)(node % g.N), q = g.q;
	double *dst = w.Lch + ((size_t)b * g.N + n) * q;
	const double *r = rx + (size_t)b * L * 2;
	const double *h = GAIN ? gain + (size_t)b * L * 2 : nullptr;
	if (mod_order == 2) {
		double bl[8];
		for (int k = 0; k < 8; k++) {
			const int sidx = (k < p) ? src[n * p + k] : -1;
			if constexpr (GAIN) {
				const double z = (sidx < 0) ? 0.0 : h[2 * sidx] * r[2 * sidx] + h[2 * sidx + 1] * r[2 * sidx + 1];
				bl[k] = (sidx < 0) ? 0.0 : -2 * z / (sigma_n * sigma_n);
			} else {
				bl[k] = (sidx < 0) ? 0.0 : -2 * r[2 * sidx] / (sigma_n * sigma_n);
			}
		}
		for (int a = lane; a < q; a += 64) {
			double acc = 0;
#pragma unroll
			for (int k = 0; k < 8; k++)
				if (k < p && (a & (1 << k)) != 0) acc += bl[k];
			dst[a] = a ? acc : 0.0;
		}
	} else {
		const int sidx = src[n];
		double c0r = cons[0], c0i = cons[1];
		const double re = sidx < 0 ? 0.0 : r[2 * sidx], im = sidx < 0 ? 0.0 : r[2 * sidx + 1];
		double hr = 0.0, hi = 0.0;
		if constexpr (GAIN) {
			hr = sidx < 0 ? 0.0 : h[2 * sidx];
			hi = sidx < 0 ? 0.0 : h[2 * sidx + 1];
			const double p0r = hr * c0r - hi * c0i, p0i = hr * c0i + hi * c0r;
			c0r = p0r;
			c0i = p0i;
		}
		for (int a = lane; a < q; a += 64) {
			double cr = cons[2 * a], ci = cons[2 * a + 1];
			if constexpr (GAIN) {
				const double par = hr * cr - hi * ci, pai = hr * ci + hi * cr;
				cr = par;
				ci = pai;
			}
			const double num = (2 * re - c0r - cr) * (cr - c0r) + (2 * im - c0i - ci) * (ci - c0i);
			dst[a] = (a == 0 || sidx < 0) ? 0.0 : num / (2 * sigma_n * sigma_n);
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// variable node: L_post = L_ch + c2v_0 + c2v_1 ... (in that order), decision, v2c = L_post - c2v (+ damping)
// (NBLDPC.cpp:676-691, 718-744 | 808-823, 848-857 | 977-992, 1029-1052)
// ---------------------------------------------------------------------------------------------------------
template <int Q, bool DAMP>
__global__ __launch_bounds__(256) void vn_kernel(NblGraphDev g, NblWork w, NblRun r)
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
	double *V = w.v2c + ((size_t)b * g.E + e0) * Q;

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
	for (int d = 0; d < dv; d++) {
		const double *Cd = C + (size_t)g.v_cpos[e0 + d] * Q;
		double *Vd = V + (size_t)d * Q;
		double nv[NS];
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			nv[i] = (a < Q) ? post[i] - Cd[a] : 0.0;
		}
		if (DAMP) {
			double ov[NS];
#pragma unroll
			for (int i = 0; i < NS; i++) {
				int a = lane + 64 * i;
				ov[i] = (a < Q) ? Vd[a] : 0.0;
			}
			int before = wave_decide<NS>(ov, lane, Q);
			int after = wave_decide<NS>(nv, lane, Q);
			if (before != after) {
#pragma unroll
				for (int i = 0; i < NS; i++) nv[i] = __dadd_rn(__dmul_rn(r.damp_old, ov[i]), __dmul_rn(r.damp_new, nv[i]));
			}
		}
#pragma unroll
		for (int i = 0; i < NS; i++) {
			int a = lane + 64 * i;
			if (a < Q) Vd[a] = (a == 0) ? 0.0 : nv[i];
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// The same variable-node pass for small fields (q <= 32): 64 / q variables per wave, lane = (variable of the wave, symbol).
// One variable per wave leaves 48 of 64 lanes idle at q = 16 and makes the launch a million tiny waves; the arithmetic per
// variable is unchanged (same sums in the same order, same decision rule), only the reductions run inside groups of q lanes.
// ---------------------------------------------------------------------------------------------------------
template <int Q> __device__ __forceinline__ double group_max(double v)
{
#pragma unroll
	for (int mk = 1; mk < Q; mk <<= 1) v = dmax(v, __shfl_xor(v, mk, 64));
	return v;
}
// DecideLLRVector (:1542-1562) inside a group of Q lanes: lowest symbol among the maxima of {0, v}; v of symbol 0 must be <= 0
template <int Q> __device__ __forceinline__ int group_decide(double v, int sub)
{
	const double mx = dmax(group_max<Q>(v), 0.0);
	const uint64_t hit = __ballot(v == mx);
	const unsigned grp = (unsigned)((hit >> (sub * Q)) & ((Q == 32) ? 0xffffffffull : ((1ull << Q) - 1)));
	return (mx > 0.0 && grp) ? __builtin_ctz(grp) : 0;
}

template <int Q, bool DAMP>
__global__ __launch_bounds__(256) void vn_packed_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	constexpr int G = 64 / Q;
	const int lane = lane_id(), sub = lane / Q, a = lane % Q;
	const long long node = ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * G + sub;
	int b = -1, n = 0;
	if (node < (long long)r.B * g.N) {
		b = nbl_codeword(w, r, (int)(node / g.N));
		n = (int)(node % g.N);
		if (b >= 0 && !r.fixed_iters && w.done[b]) b = -1;
	}
	const bool live = b >= 0;
	const int bb = live ? b : 0; // idle groups compute on codeword 0 / variable 0 and store nothing
	const int e0 = g.voff[live ? n : 0], dv = live ? g.voff[n + 1] - e0 : 0;
	const double *L = w.Lch + ((size_t)bb * g.N + (live ? n : 0)) * Q;
	const double *C = w.c2v + (size_t)bb * g.E * Q;
	double *V = w.v2c + ((size_t)bb * g.E + e0) * Q;

	double post = L[a];
	for (int d = 0; d < g.maxdv; d++)
		if (d < dv) post = post + C[(size_t)g.v_cpos[e0 + d] * Q + a];
	const int dec = group_decide<Q>(post, sub);
	if (live && a == 0) w.dec[(size_t)b * g.N + n] = dec;
	if (live && w.post) w.post[((size_t)b * g.N + n) * Q + a] = post;
	for (int d = 0; d < g.maxdv; d++) {
		const bool on = d < dv; // (the group reductions below need every lane of the wave, so the loop bound is the wave's)
		const size_t co = on ? (size_t)g.v_cpos[e0 + d] * Q + a : (size_t)a;
		double nv = post - C[co];
		if (DAMP) {
			const double ov = on ? V[(size_t)d * Q + a] : 0.0;
			const int before = group_decide<Q>(ov, sub), after = group_decide<Q>(nv, sub);
			const double blend = __dadd_rn(__dmul_rn(r.damp_old, ov), __dmul_rn(r.damp_new, nv));
			nv = (before != after) ? blend : nv;
		}
		if (on) V[(size_t)d * Q + a] = (a == 0) ? 0.0 : nv;
	}
}

// ---------------------------------------------------------------------------------------------------------
// syndrome + output freeze: one wave per codeword, lanes over checks (NBLDPC.cpp:693-715 / 826-846 / 999-1026)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void syn_kernel(NblGraphDev g, NblWork w, NblRun r)
{
	const int lane = lane_id();
	const int b = nbl_codeword(w, r, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
	if (b < 0) return;
	const int frozen = w.done[b];
	if (frozen) return;
	const int *dec = w.dec + (size_t)b * g.N;
	int bad = 0;
	for (int m = lane; m < g.M; m += 64) {
		int s = 0;
		for (int ce = g.coff[m]; ce < g.coff[m + 1]; ce++) s ^= g.mul[g.c_h[ce] * g.q + dec[g.c_var[ce]]];
		bad |= (s != 0);
	}
	const int ok = (__ballot(bad) == 0ull);
	int *out = w.out + (size_t)b * g.N;
	for (int n = lane; n < g.N; n += 64) out[n] = dec[n];
	if (lane == 0) {
		if (ok) {
			w.done[b] = 1;
			w.iters[b] = r.iter;
			atomicAdd(w.n_done, 1);
		} else {
			w.iters[b] = r.iter;
		}
	}
}

// ---------------------------------------------------------------------------------------------------------
// EMS check node: the programme itself is in nbl_cn_ems_core.h (shared with the layered kernel, nbl_cn_layered.hip)
// ---------------------------------------------------------------------------------------------------------
template <int Q>
__global__ __launch_bounds__(64) void cn_ems_kernel(NblGraphDev g, NblWork w, NblRun r, int layers)
{
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int b = nbl_flooding_codeword(g, w, r);
	if (b < 0) return;
	const NblCheck k = nbl_flooding_check(g, b);
	const EmsV2cInput<Q> in = {w.v2c + (size_t)k.b * g.E * Q, g.c_epos, k.c0}; // (nbl_cn_shell.h)
	ems_check_node<Q>(g, w, r, layers, smem, k.c0, k.dc, w.c2v + ((size_t)k.b * g.E + k.c0) * Q, in);
}

// ---------------------------------------------------------------------------------------------------------
// state read-back (parity tests): padded device layout -> [.][q-1]
// ---------------------------------------------------------------------------------------------------------
__global__ void unpad_kernel(const double *__restrict__ src, double *__restrict__ dst, const int *__restrict__ map,
                             int rows, int q)
{
	long long total = (long long)rows * (q - 1);
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		int a = (int)(i % (q - 1)) + 1;
		int row = (int)(i / (q - 1));
		int srow = map ? map[row] : row;
		dst[i] = src[(size_t)srow * q + a];
	}
}

// ---------------------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------------------
hipError_t nbl_launch_init(const double *d_Lin, const NblGraphDev &g, const NblWork &w, int B, int write_v2c, hipStream_t st)
{
	if (d_Lin && g.q >= 64 && B > 0) {
		// the re-pad at copy speed; with nothing else to initialise but the flags (fused undamped iterations) that is the whole init
		constexpr int ROWS = 4;
		const long long rows = (long long)B * g.N;
		const int rpw = g.q >= 128 ? 1 : 128 / g.q;
		const long long waves = (rows + ROWS * rpw - 1) / (ROWS * rpw), rblocks = (waves + 3) / 4;
		if (rblocks > 0x7fffffffLL) return hipErrorInvalidValue;
		const bool whole = write_v2c == 2;
		dim3 rgrid((unsigned)rblocks), rblock(256);
		switch (g.q) {
		case 64: init_rows_kernel<64, ROWS><<<rgrid, rblock, 0, st>>>(d_Lin, w.Lch, rows, w, B, whole ? 1 : 0); break;
		case 128: init_rows_kernel<128, ROWS><<<rgrid, rblock, 0, st>>>(d_Lin, w.Lch, rows, w, B, whole ? 1 : 0); break;
		case 256: init_rows_kernel<256, ROWS><<<rgrid, rblock, 0, st>>>(d_Lin, w.Lch, rows, w, B, whole ? 1 : 0); break;
		default: return hipErrorInvalidValue;
		}
		if (whole) return hipGetLastError();
		write_v2c |= 4;
	}
	long long total = (long long)B * g.E * g.q;
	int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
	if (blocks < 1) blocks = 1;
	hipLaunchKernelGGL(init_kernel, dim3(blocks), dim3(256), 0, st, d_Lin, g, w, B, write_v2c);
	return hipGetLastError();
}

hipError_t nbl_launch_demod(const double *d_rx, int L, double sigma, int mod_order, const double *d_cons, const int *d_src,
                            const NblGraphDev &g, const NblWork &w, int B, hipStream_t st, const double *d_gain)
{
	long long nodes = (long long)B * g.N;
	dim3 grid((unsigned)((nodes + 3) / 4)), block(256);
	if (d_gain) demod_kernel<true><<<grid, block, 0, st>>>(d_rx, L, sigma, mod_order, g.p, d_cons, d_src, g, w, B, d_gain);
	else demod_kernel<false><<<grid, block, 0, st>>>(d_rx, L, sigma, mod_order, g.p, d_cons, d_src, g, w, B, nullptr);
	return hipGetLastError();
}

hipError_t nbl_launch_vn(const NblGraphDev &g, const NblWork &w, const NblRun &r, bool damp, hipStream_t st)
{
	long long nodes = (long long)r.B * g.N;
	dim3 block(256);
	if (g.q <= 32 && !getenv("NBL_VN_UNPACKED")) { // small fields: 64 / q variables per wave
		const long long waves = (nodes + (64 / g.q) - 1) / (64 / g.q);
		dim3 pgrid((unsigned)((waves + 3) / 4));
#define NBL_VNP(QQ) { if (damp) vn_packed_kernel<QQ, true><<<pgrid, block, 0, st>>>(g, w, r); else vn_packed_kernel<QQ, false><<<pgrid, block, 0, st>>>(g, w, r); }
		switch (g.q) {
		case 4: NBL_VNP(4) break;
		case 8: NBL_VNP(8) break;
		case 16: NBL_VNP(16) break;
		case 32: NBL_VNP(32) break;
		default: return hipErrorInvalidValue;
		}
#undef NBL_VNP
		return hipGetLastError();
	}
	dim3 grid((unsigned)((nodes + 3) / 4));
	if (damp) { NBL_DISPATCH_Q(g.q, vn_kernel<QQ, true><<<grid, block, 0, st>>>(g, w, r)) }
	else { NBL_DISPATCH_Q(g.q, vn_kernel<QQ, false><<<grid, block, 0, st>>>(g, w, r)) }
	return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// early exit on large batches: the list of codewords that are still iterating, ascending (one workgroup; B is a few
// thousand).  Grids of the next window of iterations cover this list instead of the whole batch.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void compact_kernel(const uint8_t *__restrict__ done, int B, int *__restrict__ active, int *__restrict__ n_act)
{
	__shared__ int wsum[16];
	__shared__ int base;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	if (threadIdx.x == 0) base = 0;
	__syncthreads();
	for (int b0 = 0; b0 < B; b0 += 1024) {
		const int b = b0 + (int)threadIdx.x;
		const bool live = b < B && !done[b];
		const uint64_t m = __ballot(live);
		if (lane == 0) wsum[wv] = __builtin_popcountll(m);
		__syncthreads();
		int before = base;
		for (int k = 0; k < wv; k++) before += wsum[k];
		if (live) active[before + prefix_count(m)] = b;
		__syncthreads();
		if (threadIdx.x == 0) {
			int t = 0;
			for (int k = 0; k < 16; k++) t += wsum[k];
			base += t;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) *n_act = base;
}

hipError_t nbl_launch_compact(const uint8_t *done, int B, int *active, int *n_act, hipStream_t st)
{
	hipLaunchKernelGGL(compact_kernel, dim3(1), dim3(1024), 0, st, done, B, active, n_act);
	return hipGetLastError();
}

hipError_t nbl_launch_syn(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	dim3 grid((unsigned)((r.B + 3) / 4)), block(256);
	hipLaunchKernelGGL(syn_kernel, grid, block, 0, st, g, w, r);
	return hipGetLastError();
}

int nbl_ems_layers(int maxdc, int nc)
{
	return (nc >= maxdc - 1) ? 1 : nc + 1;
}

size_t nbl_ems_lds_bytes(int q, int maxdc, int nm, int nc)
{
	size_t doubles = (size_t)maxdc * q + (2 * (size_t)nbl_ems_layers(maxdc, nc) + 1) * q + (size_t)maxdc * nm;
	return doubles * 8 + (size_t)maxdc * nm * 4 + 16;
}

hipError_t nbl_launch_cn_ems(const NblGraphDev &g, const NblWork &w, const NblRun &r, hipStream_t st)
{
	const int layers = nbl_ems_layers(g.maxdc, r.nc);
	const size_t lds = nbl_ems_lds_bytes(g.q, g.maxdc, r.nm, r.nc);
	if (lds > NBL_MAX_LDS) return hipErrorInvalidValue; // (nbl_create refuses such shapes)
	NBL_DISPATCH_Q(g.q, return nbl_launch_checks(cn_ems_kernel<QQ>, (long long)r.B * g.M, 64, lds, st, g, w, r, layers))
}

hipError_t nbl_launch_unpad(const double *src, double *dst, const int *map, int rows, int q, hipStream_t st)
{
	long long total = (long long)rows * (q - 1);
	int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
	if (blocks < 1) blocks = 1;
	hipLaunchKernelGGL(unpad_kernel, dim3(blocks), dim3(256), 0, st, src, dst, map, rows, q);
	return hipGetLastError();
}
