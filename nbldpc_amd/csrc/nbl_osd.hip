// nbldpc_amd/csrc/nbl_osd.hip -- ordered-statistics decoding (the reference's OSD.h) on gfx950.
//
// osd_kernel: one workgroup per codeword that did not converge (converged codewords return at once).  Decoding_OSD_bit's steps:
//   1. inputs       bit LLRs L_bit[n p + k] = L_ch[n][2^k - 1] (OSD.h:23-31), reliabilities |L_bit| (flag 1) or |S| (flag 0, the
//                   factor-weighted posterior sum of osd_acc_kernel), base word DecideLLRVector(L_ch) (flag 1) or the last decisions
//   2. order        positions by reliability descending, ties by index ascending (OSD_permute, OSD.h:202-231; std::sort is not
//                   stable, so exact ties are the one known deviation): bitonic sort in LDS
//   3. elimination  H_GaussEliminate_bit (OSD.h:326-396) on bit-packed rows in LDS, with its pivot repair by the nearest row above and
//                   its rotation of order[0..num_temp] when no row has the bit.  The rotated order is the one used afterwards.
//   4. candidates   order 0, then flips of order[i] (i < MsgLen_bit), pairs, triples (OSD.h:133-181).  A candidate codeword is linear
//                   in its information bits, so it is c0 ^ g_i ^ g_j ^ g_l, with c0 the re-encoded base word and g_i the re-encoded unit
//                   vector of information position order[i] (OSD_Encode_bit, OSD.h:397-414).  Its distance is the sum of |L_bit| over the
//                   mismatching positions, added in ascending position order like compute_min_distance_bit (OSD.h:419-438) -- skipping the
//                   positions that do not mismatch adds nothing but exact zeros, so the sum is the reference's bit for bit.
//                   Flips of order[k .. MsgLen_bit-1] (k = N p - rows: the parity positions the CRC rows add) are skipped: the re-encode
//                   overwrites a parity position, so such a candidate is an earlier one again at an equal distance, and the reference only
//                   takes a candidate whose distance is STRICTLY below the running minimum.
//                   The reference keeps its running minimum in an int (NBLDPC.h:127: a winner's distance is truncated) and takes a
//                   candidate whose distance is below it, starting from 1000000: the winner is the first candidate in enumeration order
//                   whose distance has the smallest integer part, if that is below 1e6 -- a (floor(distance), enumeration rank) argmin
//                   over the workgroup.  None below 1e6: the base word stays.  The distance covers the first CodeLen*log(GFq)/log(2)
//                   positions, an int truncated from a double (compute_min_distance_bit): 575 of the 576 bits of the BDS code.
//   5. output       symbols sum_k bit[n p + k] 2^k (OSD.h:184-189) into w.out.
// osd_acc_kernel: S[b][n p + k] = factor * S + L_post[n][2^k - 1] after every iteration's variable-node pass (NBLDPC.cpp:687 / 820 / 989 /
// 1205); launched only for OSD post-processing with flag 0.
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#include "nbl_device.h"
#include "nbl_osd.h"

#define OSD_THREADS 512

struct OsdLds {
	uint64_t *H;      // [R][nw] rows of [CRC rows; H_bit], eliminated in place
	uint64_t *G;      // [k][nw] re-encoded unit vectors of the information positions
	double *absL;     // [n]
	double *key;      // [npow] reliabilities (sort keys)
	int *idx;         // [npow] positions (sorted with the keys; after the sort: the order of step 2)
	uint64_t *hd, *nz, *c0, *base, *info; // [nw] each: L > 0, L != 0, re-encoded base word, base word, information positions
	double *rd;       // [OSD_THREADS] reduction
	unsigned long long *rr;
	int *misc;        // [4]
};

// R rows of H plus k = n - R vectors of G: n rows of nw words in all, whatever R is
size_t nbl_osd_lds_bytes(int n, int R)
{
	(void)R;
	const int nw = (n + 63) / 64;
	int npow = 1;
	while (npow < n) npow <<= 1;
	return (size_t)n * nw * 8 + (size_t)n * 8 + (size_t)npow * 12 + (size_t)5 * nw * 8 + (size_t)OSD_THREADS * 16 + 16 + 64;
}

static __device__ __forceinline__ int getbit(const uint64_t *v, int pos) { return (int)((v[pos >> 6] >> (pos & 63)) & 1ull); }

// distance of the candidate with information flips f[0..cnt-1] (indices into order); mismatches summed in ascending position order
static __device__ __forceinline__ double cand_dist(const OsdLds &s, int nw, const int *f, int cnt)
{
	double acc = 0.0;
	for (int w = 0; w < nw; w++) {
		uint64_t c = s.c0[w];
		for (int t = 0; t < cnt; t++) c ^= s.G[(size_t)f[t] * nw + w];
		uint64_t m = (c ^ s.hd[w]) & s.nz[w];
		while (m) {
			const int b = __builtin_ctzll(m);
			acc = acc + s.absL[w * 64 + b];
			m &= m - 1;
		}
	}
	return acc;
}

// d: the integer part of a distance (the reference's int minimum)
static __device__ __forceinline__ void keep(double d, unsigned long long rank, double &bd, unsigned long long &br)
{
	if (d < bd || (d == bd && rank < br)) { bd = d; br = rank; }
}

// advance the pair (i, j), i < j < k, by `step` pairs in lexicographic order; i >= k - 1 afterwards = past the end
static __device__ __forceinline__ void pair_advance(int &i, int &j, int step, int k)
{
	j += step;
	while (i < k - 1 && j >= k) { i++; j = j - k + i + 1; }
}

__global__ __launch_bounds__(OSD_THREADS) void osd_kernel(NblGraphDev g, NblWork w, NblOsdDev o, int B)
{
	const int b = blockIdx.x;
	if (b >= B || w.done[b]) return;
	extern __shared__ __attribute__((aligned(16))) char smem[];
	const int tid = threadIdx.x, nt = blockDim.x;
	const int N = g.N, p = g.p, q = g.q, n = N * p, R = o.R, k = n - R, nw = (n + 63) / 64;
	int npow = 1;
	while (npow < n) npow <<= 1;
	OsdLds s;
	char *ptr = smem;
	s.H = (uint64_t *)ptr; ptr += (size_t)R * nw * 8;
	s.G = (uint64_t *)ptr; ptr += (size_t)k * nw * 8;
	s.absL = (double *)ptr; ptr += (size_t)n * 8;
	s.key = (double *)ptr; ptr += (size_t)npow * 8;
	s.hd = (uint64_t *)ptr; ptr += nw * 8;
	s.nz = (uint64_t *)ptr; ptr += nw * 8;
	s.c0 = (uint64_t *)ptr; ptr += nw * 8;
	s.base = (uint64_t *)ptr; ptr += nw * 8;
	s.info = (uint64_t *)ptr; ptr += nw * 8;
	s.rd = (double *)ptr; ptr += OSD_THREADS * 8;
	s.rr = (unsigned long long *)ptr; ptr += OSD_THREADS * 8;
	s.idx = (int *)ptr; ptr += (size_t)npow * 4;
	s.misc = (int *)ptr;

	const double *Lch = w.Lch + (size_t)b * N * q;
	int *out = w.out + (size_t)b * N;
	// ---- 1. inputs ----
	for (int i = tid; i < R * nw; i += nt) s.H[i] = o.H[i];
	for (int i = tid; i < nw; i += nt) { s.hd[i] = 0; s.nz[i] = 0; s.base[i] = 0; s.info[i] = 0; }
	__syncthreads();
	for (int i = tid; i < npow; i += nt) {
		if (i < n) {
			const double L = Lch[(size_t)(i / p) * q + (1 << (i % p))];
			s.absL[i] = fabs(L);
			const double rel = o.flag ? L : o.S[(size_t)b * n + i];
			s.key[i] = fabs(rel);
			if (L > 0) atomicOr((unsigned long long *)&s.hd[i >> 6], 1ull << (i & 63));
			if ((L > 0 || L < 0) && i < o.n_dist) atomicOr((unsigned long long *)&s.nz[i >> 6], 1ull << (i & 63));
		} else {
			s.key[i] = -1.0; // padding sorts last
		}
		s.idx[i] = i;
	}
	for (int sym = tid; sym < N; sym += nt) {
		int a = 0;
		if (o.flag) { // DecideLLRVector: first strict maximum above 0, else symbol 0
			double mx = 0.0;
			for (int x = 1; x < q; x++) {
				const double v = Lch[(size_t)sym * q + x];
				if (v > mx) { mx = v; a = x; }
			}
		} else {
			a = out[sym]; // the last iteration's decisions (DecodeOutput)
		}
		for (int j = 0; j < p; j++)
			if ((a >> j) & 1) atomicOr((unsigned long long *)&s.base[(sym * p + j) >> 6], 1ull << ((sym * p + j) & 63));
	}
	__syncthreads();
	// ---- 2. order: bitonic sort, "before" = larger key, then smaller index ----
	for (int size = 2; size <= npow; size <<= 1) {
		for (int stride = size >> 1; stride > 0; stride >>= 1) {
			for (int i = tid; i < npow; i += nt) {
				const int jx = i ^ stride;
				if (jx > i) {
					const bool asc = (i & size) == 0; // ascending in "before" order
					const double ka = s.key[i], kb = s.key[jx];
					const int ia = s.idx[i], ib = s.idx[jx];
					const bool b_first = kb > ka || (kb == ka && ib < ia);
					if (b_first == asc) { s.key[i] = kb; s.key[jx] = ka; s.idx[i] = ib; s.idx[jx] = ia; }
				}
			}
			__syncthreads();
		}
	}
	int *order = s.idx; // [n]
	// ---- 3. elimination (H_GaussEliminate_bit) ----
	bool ok = true;
	for (int row = R - 1; row >= 0 && ok; row--) {
		const int num_temp = row + n - R;
		int rotations = 0;
		int col;
		for (;;) {
			col = order[num_temp];
			if (getbit(s.H + (size_t)row * nw, col)) break;
			if (tid == 0) s.misc[0] = -1;
			__syncthreads();
			for (int r = tid; r < row; r += nt)
				if (getbit(s.H + (size_t)r * nw, col)) atomicMax(&s.misc[0], r); // nearest row above = the largest index below `row`
			__syncthreads();
			const int up = s.misc[0];
			if (up >= 0) {
				for (int x = tid; x < nw; x += nt) s.H[(size_t)row * nw + x] ^= s.H[(size_t)up * nw + x];
				__syncthreads();
				break;
			}
			// no row has the bit: order[0..num_temp] rotates right by one (the swap chain of OSD.h:362-368), and the row is redone
			if (++rotations > num_temp + 1) { ok = false; break; } // (not full rank: refused at creation, never reached)
			int v[NBL_OSD_MAX_BITS / OSD_THREADS];
#pragma unroll
			for (int u = 0; u < NBL_OSD_MAX_BITS / OSD_THREADS; u++) {
				const int x = tid + u * OSD_THREADS;
				v[u] = (x <= num_temp) ? order[x == 0 ? num_temp : x - 1] : 0;
			}
			__syncthreads();
#pragma unroll
			for (int u = 0; u < NBL_OSD_MAX_BITS / OSD_THREADS; u++) {
				const int x = tid + u * OSD_THREADS;
				if (x <= num_temp) order[x] = v[u];
			}
			__syncthreads();
		}
		if (!ok) break;
		// clear the pivot column in the rows above
		for (int r = tid; r < row; r += nt) {
			uint64_t *hr = s.H + (size_t)r * nw;
			if (getbit(hr, col)) {
				const uint64_t *hp = s.H + (size_t)row * nw;
				for (int x = 0; x < nw; x++) hr[x] ^= hp[x];
			}
		}
		__syncthreads();
	}
	if (ok) {
		// second pass (OSD.h:384-394): row i's pivot cleared from the rows below it
		for (int i = 0; i < R; i++) {
			const int pos = order[n - R + i];
			for (int r = i + 1 + tid; r < R; r += nt) {
				uint64_t *hr = s.H + (size_t)r * nw;
				if (getbit(hr, pos)) {
					const uint64_t *hp = s.H + (size_t)i * nw;
					for (int x = 0; x < nw; x++) hr[x] ^= hp[x];
				}
			}
			__syncthreads();
		}
	}
	// ---- 4. candidates ----
	double bd = 1e300;
	unsigned long long br = ~0ull;
	if (ok) {
		for (int i = tid; i < k; i += nt) atomicOr((unsigned long long *)&s.info[order[i] >> 6], 1ull << (order[i] & 63));
		__syncthreads();
		// c0: base word on the information positions, re-encoded parity bits (OSD_Encode_bit)
		for (int x = tid; x < nw; x += nt) s.c0[x] = s.base[x] & s.info[x];
		__syncthreads();
		for (int r = tid; r < R; r += nt) {
			const uint64_t *hr = s.H + (size_t)r * nw;
			int par = 0;
			for (int x = 0; x < nw; x++) par ^= __builtin_popcountll(hr[x] & s.info[x] & s.base[x]) & 1;
			const int pos = order[k + r];
			if (par) atomicOr((unsigned long long *)&s.c0[pos >> 6], 1ull << (pos & 63));
		}
		// g_i: unit vector of information position order[i], re-encoded
		for (int i = tid; i < k; i += nt) {
			uint64_t *gi = s.G + (size_t)i * nw;
			for (int x = 0; x < nw; x++) gi[x] = 0;
			const int pos = order[i];
			gi[pos >> 6] |= 1ull << (pos & 63);
			for (int r = 0; r < R; r++)
				if (getbit(s.H + (size_t)r * nw, pos)) { const int pp = order[k + r]; gi[pp >> 6] |= 1ull << (pp & 63); }
		}
		__syncthreads();
		const int ord = o.order < 0 ? 0 : (o.order > 3 ? 3 : o.order);
		const int kk = k; // information flips only (see the head of the file)
		int f[3];
		if (tid == 0) keep(floor(cand_dist(s, nw, f, 0)), 0ull, bd, br);
		if (ord >= 1)
			for (int i = tid; i < kk; i += nt) {
				f[0] = i;
				keep(floor(cand_dist(s, nw, f, 1)), (1ull << 60) | ((unsigned long long)i << 40), bd, br);
			}
		if (ord >= 2 && kk >= 2) {
			int i = 0, j = 1;
			pair_advance(i, j, tid, kk);
			for (; i < kk - 1; pair_advance(i, j, nt, kk)) {
				f[0] = i; f[1] = j;
				keep(floor(cand_dist(s, nw, f, 2)), (2ull << 60) | ((unsigned long long)i << 40) | ((unsigned long long)j << 20), bd, br);
			}
		}
		if (ord >= 3 && kk >= 3) {
			int i = 0, j = 1;
			pair_advance(i, j, tid, kk);
			for (; i < kk - 1; pair_advance(i, j, nt, kk)) {
				for (int l = j + 1; l < kk; l++) {
					f[0] = i; f[1] = j; f[2] = l;
					keep(floor(cand_dist(s, nw, f, 3)),
					     (3ull << 60) | ((unsigned long long)i << 40) | ((unsigned long long)j << 20) | (unsigned long long)l, bd, br);
				}
			}
		}
	}
	s.rd[tid] = bd;
	s.rr[tid] = br;
	__syncthreads();
	if (tid == 0) {
		for (int t = 1; t < nt; t++) keep(s.rd[t], s.rr[t], bd, br);
		s.rd[0] = bd;
		s.rr[0] = br;
	}
	__syncthreads();
	bd = s.rd[0];
	br = s.rr[0];
	// ---- 5. output: the winner if its distance is below 1e6, else the base word.  The reference copies a winner into
	// near_optimal_bit over the same truncated CodeLen_bit positions its distance covers (OSD.h:432-436); the positions from n_dist
	// on keep the base word's bits (set at OSD.h:31) ----
	const bool win = ok && bd < 1000000.0;
	int fl[3], cnt = 0;
	if (win) {
		cnt = (int)(br >> 60);
		fl[0] = (int)((br >> 40) & 0xfffff);
		fl[1] = (int)((br >> 20) & 0xfffff);
		fl[2] = (int)(br & 0xfffff);
	}
	for (int x = tid; x < nw; x += nt) {
		uint64_t c = s.c0[x];
		for (int t = 0; t < cnt; t++) c ^= s.G[(size_t)fl[t] * nw + x];
		const int lo = x * 64;
		const uint64_t keep_lo = o.n_dist >= lo + 64 ? ~0ull : (o.n_dist <= lo ? 0ull : ((1ull << (o.n_dist - lo)) - 1));
		s.info[x] = win ? ((c & keep_lo) | (s.base[x] & ~keep_lo)) : s.base[x]; // (info is not needed any more: it holds the result)
	}
	__syncthreads();
	for (int sym = tid; sym < N; sym += nt) {
		int a = 0;
		for (int j = p - 1; j >= 0; j--) a = 2 * a + getbit(s.info, sym * p + j);
		out[sym] = a;
	}
}

__global__ __launch_bounds__(256) void osd_acc_kernel(const double *__restrict__ post, double *__restrict__ S, int B, int N, int p, int q,
                                                      double factor, int first)
{
	const long long total = (long long)B * N * p;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
		const long long bn = i / p;
		const int k = (int)(i % p);
		const double prev = first ? 0.0 : S[i];
		S[i] = factor * prev + post[bn * q + (1 << k)];
	}
}

hipError_t nbl_launch_osd(const NblGraphDev &g, const NblWork &w, const NblOsdDev &o, int B, hipStream_t st)
{
	const size_t lds = nbl_osd_lds_bytes(g.N * g.p, o.R);
	if (lds > 64 * 1024) {
		// the attribute is a property of the kernel on each device: set once per device, under a lock (decoders may live on several
		// devices and host threads)
		static std::mutex mu;
		static std::vector<char> done;
		int dev = 0;
		hipError_t e = hipGetDevice(&dev);
		if (e != hipSuccess) return e;
		std::lock_guard<std::mutex> lock(mu);
		if ((int)done.size() <= dev) done.resize(dev + 1, 0);
		if (!done[dev]) {
			e = hipFuncSetAttribute((const void *)osd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NBL_OSD_MAX_LDS);
			if (e != hipSuccess) return e;
			done[dev] = 1;
		}
	}
	hipLaunchKernelGGL(osd_kernel, dim3(B), dim3(OSD_THREADS), lds, st, g, w, o, B);
	return hipGetLastError();
}

hipError_t nbl_launch_osd_acc(const double *post, double *S, int B, int N, int p, int q, double factor, int first, hipStream_t st)
{
	const long long total = (long long)B * N * p;
	long long blocks = (total + 255) / 256;
	if (blocks > 65536) blocks = 65536;
	hipLaunchKernelGGL(osd_acc_kernel, dim3((unsigned)blocks), dim3(256), 0, st, post, S, B, N, p, q, factor, first);
	return hipGetLastError();
}
