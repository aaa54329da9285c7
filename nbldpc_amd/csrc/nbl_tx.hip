// nbldpc_amd/csrc/nbl_tx.hip -- the transmit side of the reference's link chain and its error count on the device.
//
//   CComm::GenerateMessage  Comm.cpp:181-252   PN register bits, lane-interleaved (every message bit costs `parallel` clocks)
//   CComm::CRCEncode        Comm.cpp:506-561   CRC of the message bits (register starts at zero: linear)
//   CNBLDPC::Encode         NBLDPC.cpp:562-604 systematic encode + column exchanges (GF(q)-linear, hence GF(2)-linear on bits)
//   CComm::Encode/Puncture/Modulate  Comm.cpp:255-325  LSB-first unpacking, punctured bits dropped, MSB-first packing
//   CComm::Decode/Err       Comm.cpp:421-493   symbol / bit compares and CrcCheck of the decoded message
//
// PN bits -> CRC -> encoder -> code bits is ONE binary matrix T (N p rows, K p - crc_len columns) that nbl_set_transmitter builds
// on the host.  Four kernels:
//   tx_pn_kernel      the PN bits of every lane, packed 64 per word, from the register's period table
//   tx_encode_kernel  code bit (frame, row) = parity(T[row] & u[frame]): a thread owns one row and NBL_TX_F frames, so a word of T
//                     is loaded once for NBL_TX_F frames; T is stored word-major ([word][row]) and a wave's loads are contiguous
//   tx_pack_kernel    code bits -> code symbols (LSB first) and constellation indices (kept bits, MSB first)
//   tx_errcount_kernel one wave per frame: symbol compares, popcount of the bit XOR, CRC division as XOR of per-bit remainders
#include <hip/hip_runtime.h>
#include "nbl_kernels.h"

// bit j of lane b = seq[(phase(pn_state[b]) + (j + 1) * parallel - 1) mod period]: the register is clocked `parallel - 1` times,
// then once more with its output taken (Comm.cpp:199-202).  phase < 0: the register holds zeros and so does its output.
__global__ __launch_bounds__(256) void tx_pn_kernel(const uint16_t *__restrict__ pn_state, const int16_t *__restrict__ phase_of,
                                                    const uint8_t *__restrict__ seq, int period, int par_mod, int nb, int nw, int B,
                                                    unsigned long long *__restrict__ u)
{
	const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (tid >= (long long)B * nw) return;
	const int b = (int)(tid / nw), w = (int)(tid % nw);
	const int ph = phase_of[pn_state[b] & 2047];
	unsigned long long word = 0;
	if (ph >= 0) {
		// position of bit 64 w: (ph + (64 w + 1) par_mod - 1) mod period, then steps of par_mod
		int pos = (int)(((long long)ph + (long long)(64 * w + 1) * par_mod + period - 1) % period);
		const int n = nb - 64 * w < 64 ? nb - 64 * w : 64;
		for (int i = 0; i < n; i++) {
			word |= (unsigned long long)seq[pos] << i;
			pos += par_mod;
			if (pos >= period) pos -= period;
		}
	}
	u[tid] = word;
}

template <int F>
__global__ __launch_bounds__(256) void tx_encode_kernel(const unsigned long long *__restrict__ T, const unsigned long long *__restrict__ u,
                                                        int rows, int nw, int B, uint8_t *__restrict__ bits)
{
	extern __shared__ unsigned long long us[]; // [F][nw]
	const int f0 = blockIdx.x * F; // (frames on x: the grid's x extent is the large one)
	for (int i = threadIdx.x; i < F * nw; i += blockDim.x) {
		const int f = i / nw;
		us[i] = (f0 + f < B) ? u[(size_t)(f0 + f) * nw + (i - f * nw)] : 0ull;
	}
	__syncthreads();
	const int r = blockIdx.y * blockDim.x + threadIdx.x;
	if (r >= rows) return;
	unsigned long long acc[F];
#pragma unroll
	for (int f = 0; f < F; f++) acc[f] = 0;
	for (int w = 0; w < nw; w++) {
		const unsigned long long t = T[(size_t)w * rows + r];
#pragma unroll
		for (int f = 0; f < F; f++) acc[f] ^= t & us[f * nw + w];
	}
#pragma unroll
	for (int f = 0; f < F; f++)
		if (f0 + f < B) bits[(size_t)(f0 + f) * rows + r] = (uint8_t)(__builtin_popcountll(acc[f]) & 1);
}

// per frame N + L outputs: code symbol n = sum_j bit[n p + j] << j; index s = sum_k bit[keep[s mb + k]] << (mb - 1 - k)
__global__ __launch_bounds__(256) void tx_pack_kernel(const uint8_t *__restrict__ bits, const int *__restrict__ keep, int N, int p, int L,
                                                      int mb, int B, uint8_t *__restrict__ code, uint8_t *__restrict__ txi)
{
	const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	const int per = N + L;
	if (tid >= (long long)B * per) return;
	const int b = (int)(tid / per), i = (int)(tid % per);
	const uint8_t *fb = bits + (size_t)b * N * p;
	int v = 0;
	if (i < N) {
		for (int j = 0; j < p; j++) v |= fb[i * p + j] << j;
		code[(size_t)b * N + i] = (uint8_t)v;
	} else {
		const int s = i - N;
		for (int k = 0; k < mb; k++) v |= fb[keep[s * mb + k]] << (mb - 1 - k);
		txi[(size_t)b * L + s] = (uint8_t)v;
	}
}

// message symbols [B][K] -> message bits packed 64 per word (bit s p + k = bit k of symbol s), the input of tx_encode_kernel
// for the plain encoder
__global__ __launch_bounds__(256) void tx_msgbits_kernel(const int *__restrict__ msg, int K, int p, int nw, int B, unsigned long long *__restrict__ u)
{
	const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (tid >= (long long)B * nw) return;
	const int b = (int)(tid / nw), w = (int)(tid % nw);
	unsigned long long word = 0;
	for (int i = 0; i < 64; i++) {
		const int bit = 64 * w + i;
		if (bit >= K * p) break;
		word |= (unsigned long long)((msg[(size_t)b * K + bit / p] >> (bit % p)) & 1) << i;
	}
	u[tid] = word;
}

// TakeDecoded + Err of one frame (Comm.cpp:421-493): errSym, errBit over the K message symbols, CrcCheck(RX_MSG_BIT, K p, crc_len, 1)
// as the XOR of the remainders crc_col[bit] of the set bits; an all-zero word is no CRC pass; crc_len = 0 always passes.
__global__ __launch_bounds__(64) void tx_errcount_kernel(const int *__restrict__ dec, const uint8_t *__restrict__ code, const uint32_t *__restrict__ crc_col,
                                                         int N, int K, int p, int crc_len, int B, int *__restrict__ err_sym, int *__restrict__ err_bit,
                                                         uint8_t *__restrict__ crc_ok)
{
	const int b = blockIdx.x;
	if (b >= B) return;
	const int mask = (1 << p) - 1;
	int es = 0, eb = 0, ones = 0;
	uint32_t reg = 0;
	for (int s = threadIdx.x; s < K; s += 64) {
		const int d = dec[(size_t)b * N + s], t = code[(size_t)b * N + s];
		es += (d != t);
		eb += __builtin_popcount((d ^ t) & mask);
		const int rx = d & mask;
		ones += __builtin_popcount(rx);
		if (crc_len)
			for (int k = 0; k < p; k++)
				if ((rx >> k) & 1) reg ^= crc_col[s * p + k];
	}
	for (int o = 32; o > 0; o >>= 1) {
		es += __shfl_xor(es, o);
		eb += __shfl_xor(eb, o);
		ones += __shfl_xor(ones, o);
		reg ^= (uint32_t)__shfl_xor((int)reg, o);
	}
	if (threadIdx.x == 0) {
		err_sym[b] = es;
		err_bit[b] = eb;
		crc_ok[b] = (uint8_t)(crc_len == 0 ? 1 : (reg == 0 && ones != 0));
	}
}

hipError_t nbl_launch_tx_pn(const uint16_t *pn_state, const int16_t *phase_of, const uint8_t *seq, int period, int par_mod, int nb, int nw,
                            int B, unsigned long long *u, hipStream_t st)
{
	const long long total = (long long)B * nw;
	if (total == 0) return hipSuccess;
	tx_pn_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(pn_state, phase_of, seq, period, par_mod, nb, nw, B, u);
	return hipGetLastError();
}

hipError_t nbl_launch_tx_encode(const unsigned long long *T, const unsigned long long *u, int rows, int nw, int B, uint8_t *bits, hipStream_t st)
{
	if (B == 0 || rows == 0) return hipSuccess;
	const dim3 grid((unsigned)((B + NBL_TX_F - 1) / NBL_TX_F), (unsigned)((rows + 255) / 256));
	tx_encode_kernel<NBL_TX_F><<<grid, dim3(256), (size_t)NBL_TX_F * nw * 8, st>>>(T, u, rows, nw, B, bits);
	return hipGetLastError();
}

hipError_t nbl_launch_tx_pack(const uint8_t *bits, const int *keep, int N, int p, int L, int mb, int B, uint8_t *code, uint8_t *txi, hipStream_t st)
{
	const long long total = (long long)B * (N + L);
	if (total == 0) return hipSuccess;
	tx_pack_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(bits, keep, N, p, L, mb, B, code, txi);
	return hipGetLastError();
}

hipError_t nbl_launch_tx_msgbits(const int *msg, int K, int p, int nw, int B, unsigned long long *u, hipStream_t st)
{
	const long long total = (long long)B * nw;
	if (total == 0) return hipSuccess;
	tx_msgbits_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(msg, K, p, nw, B, u);
	return hipGetLastError();
}

hipError_t nbl_launch_tx_errcount(const int *dec, const uint8_t *code, const uint32_t *crc_col, int N, int K, int p, int crc_len, int B,
                                  int *err_sym, int *err_bit, uint8_t *crc_ok, hipStream_t st)
{
	if (B == 0) return hipSuccess;
	tx_errcount_kernel<<<dim3((unsigned)B), dim3(64), 0, st>>>(dec, code, crc_col, N, K, p, crc_len, B, err_sym, err_bit, crc_ok);
	return hipGetLastError();
}
