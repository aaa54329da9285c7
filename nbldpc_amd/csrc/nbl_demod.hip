// nbldpc_amd/csrc/nbl_demod.hip -- the general soft demodulator: any constellation of M = 2^m points (m <= 8) against any field
// q = 2^p, any assignment of label bits to code bits (include/nbldpc.h, nbl_set_demodulator_ex).
//
// One wave per (codeword, code symbol), as demod_kernel has it.  The symbol's touched points are walked in ascending s; per point
//   1. the lanes compute the M distances d_s(c) into the wave's LDS region                      dist[c],  c < M
//   2. lane `pat` folds the foreign combinations of own pattern `pat` (ascending c) to the minimum  tab[pat], pat < 2^own
//   3. log-sum only, points with a foreign position: the lanes turn dist[c] into exp(-(d - dmin) / (2 sigma^2)) -- all M
//      exponentials side by side -- and lane `pat` adds its own terms in ascending c, then tab[pat] = dmin - 2 sigma^2 log(sum)
//   4. every lane adds (tab[0] - tab[pattern of a]) / (2 sigma^2) to its q / 64 values of a, held in registers
// The own pattern lists the own label positions in ascending position i, bit r = the r-th of them.  LDS per wave: M + 2^own <= 512
// doubles.  Every expression keeps the order the header defines; the library is compiled with -ffp-contract=off.
//
// PRIOR (nbl_decode_batch_samples_prior, the passes of nbl_decode_batch_samples_idd): between steps 1 and 2 lane c
// takes  (2 sigma^2) * (the priors of the claimed foreign label bits that are 1 in c, added in ascending position)  off its distance.
// The at most m prior values of a point are the same for the whole wave: codeword, point and the claim table tinv[s m + i] are made
// provably uniform, so they arrive as scalar loads, not as 64 lanes reading one address.  The instance without PRIOR is the kernel
// the prior-less calls have always launched.
//
// GAIN (nbl_decode_batch_samples_csi, the resident decodes under nbl_set_fading): step 1 measures the distance to
// the FADED point (hr cr - hi ci, hr ci + hi cr), (hr, hi) = gain[b][s].  The gain of a point is the same for the whole wave: codeword
// and point are made provably uniform, as for the priors, so it arrives as one scalar load.  The instances without GAIN are the
// kernels the gain-less calls have always launched.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nbldpc.h"
#include "nbl_device.h"
#include "nbl_kernels.h"

#define DSYNC() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")

// constellation index of (own pattern, foreign combination): label position i has weight 2^(m-1-i); both lists ascend in i, so the
// LAST listed position is the lowest bit of c and ascending f is ascending c for a fixed pattern
__device__ __forceinline__ int demod_index(const NblDemodPoint &pt, int m, int pat, int f)
{
	int c = 0, r = 0, u = 0;
	for (int i = 0; i < m; i++) {
		int bit;
		if (pt.own[i] >= 0) { bit = (pat >> r) & 1; r++; }
		else { bit = (f >> (m - pt.nown - 1 - u)) & 1; u++; }
		c |= bit << (m - 1 - i);
	}
	return c;
}

__device__ __forceinline__ int demod_pattern_of_index(const NblDemodPoint &pt, int m, int c)
{
	int pat = 0, r = 0;
	for (int i = 0; i < m; i++)
		if (pt.own[i] >= 0) { pat |= ((c >> (m - 1 - i)) & 1) << r; r++; }
	return pat;
}

__device__ __forceinline__ int demod_pattern_of_value(const NblDemodPoint &pt, int m, int a)
{
	int pat = 0, r = 0;
	for (int i = 0; i < m; i++)
		if (pt.own[i] >= 0) { pat |= ((a >> pt.own[i]) & 1) << r; r++; }
	return pat;
}

template <bool PRIOR, bool GAIN>
__global__ __launch_bounds__(256) void demod_general_kernel(const double *__restrict__ rx, int L, double sigma_n, int M, int m, int metric,
                                                            const double *__restrict__ cons, const NblDemodPoint *__restrict__ desc,
                                                            NblGraphDev g, NblWork w, int B, const double *__restrict__ prior,
                                                            const int *__restrict__ tinv, const double *__restrict__ gain)
{
	__shared__ double lds[4][512];
	const int lane = lane_id();
	const long long node = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (node >= (long long)B * g.N) return;
	const int b = (int)(node / g.N), n = (int)(node % g.N), q = g.q, p = g.p;
	double *dist = lds[threadIdx.x >> 6], *tab = dist + M;
	double *dst = w.Lch + ((size_t)b * g.N + n) * q;
	const double *r = rx + (size_t)b * L * 2;
	const NblDemodPoint *dn = desc + (size_t)n * (p + 1);
	const int nt = dn[0].s; // header entry: number of touched points
	const double two = 2 * sigma_n * sigma_n;

	double acc[4] = {0.0, 0.0, 0.0, 0.0};
	for (int k = 0; k < nt; k++) {
		const NblDemodPoint pt = dn[1 + k];
		const double re = r[2 * pt.s], im = r[2 * pt.s + 1];
		const int npat = 1 << pt.nown, nfor = 1 << (m - pt.nown);
		// PRIOR: pv[i] = prior of the code bit that claims foreign label position i of this point, cm bit i = there is one
		double pv[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
		int cm = 0;
		if constexpr (PRIOR) {
			int fm = 0;
#pragma unroll
			for (int i = 0; i < 8; i++)
				if (i < m && pt.own[i] < 0) fm |= 1 << i;
			fm = uniform(fm);
			const int *ti = tinv + (size_t)uniform(pt.s) * m;
			const double *pr = prior + (size_t)uniform(b) * g.N * p;
#pragma unroll
			for (int i = 0; i < 8; i++)
				if ((fm >> i) & 1) {
					const int gb = ti[i];
					if (gb >= 0) { pv[i] = pr[gb]; cm |= 1 << i; }
				}
		}
		double hr = 0.0, hi = 0.0;
		if constexpr (GAIN) {
			const double *gn = gain + ((size_t)uniform(b) * L + (size_t)uniform(pt.s)) * 2;
			hr = gn[0];
			hi = gn[1];
		}
		DSYNC(); // the previous point's table has been read by every lane
		for (int c = lane; c < M; c += 64) {
			double cr = cons[2 * c], ci = cons[2 * c + 1];
			if constexpr (GAIN) {
				const double pr = hr * cr - hi * ci, pi = hr * ci + hi * cr;
				cr = pr;
				ci = pi;
			}
			double d = (re - cr) * (re - cr) + (im - ci) * (im - ci);
			if constexpr (PRIOR) {
				double A = 0.0;
#pragma unroll
				for (int i = 0; i < 8; i++)
					if (((cm >> i) & 1) && ((c << i >> (m - 1)) & 1)) A = A + pv[i]; // (bit i of the label has weight 2^(m-1-i); cm is 0 from m up)
				d = d - two * A;
			}
			dist[c] = d;
		}
		DSYNC();
		for (int pat = lane; pat < npat; pat += 64) {
			double dm = dist[demod_index(pt, m, pat, 0)];
			for (int f = 1; f < nfor; f++) {
				const double d = dist[demod_index(pt, m, pat, f)];
				dm = d < dm ? d : dm;
			}
			tab[pat] = dm;
		}
		if (metric == NBL_DEMOD_LOGSUM && nfor > 1) {
			DSYNC();
			for (int c = lane; c < M; c += 64) {
				const double dm = tab[demod_pattern_of_index(pt, m, c)];
				dist[c] = exp(-(dist[c] - dm) / two);
			}
			DSYNC();
			for (int pat = lane; pat < npat; pat += 64) {
				double sum = 0.0;
				for (int f = 0; f < nfor; f++) sum = sum + dist[demod_index(pt, m, pat, f)];
				tab[pat] = tab[pat] - two * log(sum);
			}
		}
		DSYNC();
		const double t0 = tab[0];
#pragma unroll
		for (int i = 0; i < 4; i++) {
			const int a = lane + 64 * i;
			if (a < q) acc[i] = acc[i] + (t0 - tab[demod_pattern_of_value(pt, m, a)]) / two;
		}
	}
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const int a = lane + 64 * i;
		if (a < q) dst[a] = a ? acc[i] : 0.0;
	}
}

hipError_t nbl_launch_demod_general(const double *d_rx, int L, double sigma, int mod_order, int metric, const double *d_cons,
                                    const NblDemodPoint *d_desc, const NblGraphDev &g, const NblWork &w, int B, hipStream_t st,
                                    const double *d_prior, const int *d_tinv, const double *d_gain)
{
	int m = 0;
	while ((1 << m) < mod_order) m++;
	if (m < 1 || m > 8 || (1 << m) != mod_order || g.q > 256 || !d_cons || !d_desc) return hipErrorInvalidValue;
	long long nodes = (long long)B * g.N;
	dim3 grid((unsigned)((nodes + 3) / 4)), block(256);
	if (d_prior && !d_tinv) return hipErrorInvalidValue;
	if (d_prior && d_gain)
		demod_general_kernel<true, true><<<grid, block, 0, st>>>(d_rx, L, sigma, mod_order, m, metric, d_cons, d_desc, g, w, B, d_prior, d_tinv, d_gain);
	else if (d_gain)
		demod_general_kernel<false, true><<<grid, block, 0, st>>>(d_rx, L, sigma, mod_order, m, metric, d_cons, d_desc, g, w, B, nullptr, nullptr, d_gain);
	else if (d_prior)
		demod_general_kernel<true, false><<<grid, block, 0, st>>>(d_rx, L, sigma, mod_order, m, metric, d_cons, d_desc, g, w, B, d_prior, d_tinv, nullptr);
	else
		demod_general_kernel<false, false><<<grid, block, 0, st>>>(d_rx, L, sigma, mod_order, m, metric, d_cons, d_desc, g, w, B, nullptr, nullptr, nullptr);
	return hipGetLastError();
}
