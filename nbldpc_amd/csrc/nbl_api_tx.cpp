// nbldpc_amd/csrc/nbl_api_tx.cpp -- the transmit side and the error count on the device (nbl_tx.hip): nbl_pn_advance,
// nbl_set_transmitter, nbl_transmit_batch, nbl_count_errors, nbl_encode_batch and the read-backs of what a slot holds.
#include <cstring>
#include "nbl_decoder.h"

// one clock of the PN register (Comm.cpp:241-252): shift, then regPN[0] = regPN[10] ^ regPN[3]; the output is regPN[10] after the shift
static inline unsigned pn_step(unsigned s) { return ((s << 1) & 2047u) | (((s >> 9) ^ (s >> 2)) & 1u); }

extern "C" void nbl_pn_advance(uint16_t *state, uint64_t clocks)
{
	if (!state) return;
	// the update is a map of an 11-bit state: square it repeatedly (2048-entry tables) and apply the tables of the set bits
	static const std::vector<std::vector<uint16_t>> pow2 = [] {
		std::vector<std::vector<uint16_t>> t(64, std::vector<uint16_t>(2048));
		for (unsigned s = 0; s < 2048; s++) t[0][s] = (uint16_t)pn_step(s);
		for (int k = 1; k < 64; k++)
			for (unsigned s = 0; s < 2048; s++) t[k][s] = t[k - 1][t[k - 1][s]];
		return t;
	}();
	unsigned s = *state & 2047u;
	for (int k = 0; k < 64; k++)
		if ((clocks >> k) & 1) s = pow2[k][s];
	*state = (uint16_t)s;
}

// tap masks of the CRC registers (Comm.cpp:513-533): bit j set for G[j], j = 0 .. len - 1
static uint32_t crc_tap_mask(int len, int type24)
{
	static const int t8[] = {0, 1, 3, 4, 7}, t16[] = {0, 5, 12}, t24a[] = {0, 1, 3, 4, 5, 6, 7, 10, 11, 14, 17, 18, 23}, t24b[] = {0, 1, 5, 6, 23};
	uint32_t m = 0;
	if (len == 8) for (int x : t8) m |= 1u << x;
	else if (len == 16) for (int x : t16) m |= 1u << x;
	else if (len == 24 && !type24) for (int x : t24a) m |= 1u << x;
	else if (len == 24) for (int x : t24b) m |= 1u << x;
	return m;
}

template <typename T> static nbl_status tx_upload(std::string &err, const std::vector<T> &h, DevBuf<T> &dst)
{
	if (nbl_status s = dst.grow(err, h.size() * sizeof(T) + 16)) return s;
	HIP_TRY_E(err, hipMemcpy(dst, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
	return NBL_OK;
}

extern "C" nbl_status nbl_set_transmitter(nbl_decoder *d, const nbl_tx_desc *tx)
{
	if (!d || !tx) return NBL_ERR_ARG;
	d->err.clear();
	const int N = d->g.N, M = d->g.M, q = d->g.q, p = d->g.p, K = N - M;
	if (!d->dm_order) { d->err = "nbl_set_transmitter: nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (d->h_cons.empty() || !d->d_cons) { d->err = "nbl_set_transmitter: the demodulator was set without constellation points (the channel needs them, also for BPSK)"; return NBL_ERR_ARG; }
	if (tx->mod_order != d->dm_order || tx->n_mod_sym != d->dm_L) { d->err = "nbl_set_transmitter: mod_order / n_mod_sym differ from the demodulator's"; return NBL_ERR_ARG; }
	if (tx->mod_order > 256) { d->err = "nbl_set_transmitter: mod_order above 256 is not supported (constellation indices are bytes)"; return NBL_ERR_UNSUPPORTED; }
	if (tx->crc_len != 0 && tx->crc_len != 8 && tx->crc_len != 16 && tx->crc_len != 24) { d->err = "nbl_set_transmitter: crc_len must be 0, 8, 16 or 24"; return NBL_ERR_ARG; }
	if (K <= 0) { d->err = "nbl_set_transmitter: the code has no message symbols"; return NBL_ERR_ARG; }
	if (tx->crc_len > K * p) { d->err = "nbl_set_transmitter: crc_len exceeds the message length K log2(q)"; return NBL_ERR_UNSUPPORTED; }
	if (tx->parallel < 1) { d->err = "nbl_set_transmitter: parallel < 1"; return NBL_ERR_ARG; }
	if (tx->n_punct < 0 || (tx->n_punct > 0 && !tx->punct)) { d->err = "nbl_set_transmitter: bad puncture list"; return NBL_ERR_ARG; }
	for (int i = 0; i < tx->n_punct; i++)
		if (tx->punct[i] < 0 || tx->punct[i] >= N || (i > 0 && tx->punct[i] <= tx->punct[i - 1])) { d->err = "nbl_set_transmitter: punctured positions must be ascending and below N"; return NBL_ERR_ARG; }
	const int mb = ilog2(tx->mod_order);
	// MOD_SYM_LEN = (N - n_punct) p / MOD_BIT_PER_SYM (Comm.cpp:105): the modulator consumes the first L mb kept bits
	if ((long long)tx->n_mod_sym * mb > (long long)(N - tx->n_punct) * p) { d->err = "nbl_set_transmitter: n_mod_sym needs more bits than the unpunctured code word has"; return NBL_ERR_ARG; }
	if (tx->random_msg && !tx->gen) { d->err = "nbl_set_transmitter: gen is NULL with random_msg != 0"; return NBL_ERR_ARG; }
	const int rows = N * p, nb = K * p - tx->crc_len, nw = (nb + 63) / 64, nwg = (K * p + 63) / 64;
	if (rows > 65536 || (size_t)rows * nwg * 8 > ((size_t)64 << 20)) { d->err = "nbl_set_transmitter: code too large for the transmit kernel (N log2(q) above 65536 bits or a matrix above 64 MiB)"; return NBL_ERR_UNSUPPORTED; }
	// H gen = 0 with the decoder's own graph and tables
	if (tx->gen) {
		for (size_t i = 0; i < (size_t)N * K; i++)
			if (tx->gen[i] >= q) { d->err = "nbl_set_transmitter: gen holds a value >= q"; return NBL_ERR_ARG; }
		for (int m = 0; m < M; m++)
			for (int k = 0; k < K; k++) {
				int acc = 0;
				for (int ce = d->h_coff[m]; ce < d->h_coff[m + 1]; ce++) acc ^= d->h_mul[(size_t)d->h_ch[ce] * q + tx->gen[(size_t)d->h_cvar[ce] * K + k]];
				if (acc) { d->err = "nbl_set_transmitter: H * gen != 0 (check " + std::to_string(m) + ", message symbol " + std::to_string(k) + ")"; return NBL_ERR_ARG; }
			}
	}
	HIP_TRY(d, hipSetDevice(d->device));
	if (d->stream2) HIP_TRY(d, hipStreamSynchronize(d->stream2));
	d->tx = nbl_decoder::Tx();
	nbl_decoder::Tx &t = d->tx;
	t.crc_len = tx->crc_len; t.random_msg = tx->random_msg; t.K = K; t.nb = nb; t.nw = nw; t.nwg = nwg; t.mb = mb;
	nbl_status st;
	if (tx->gen) {
		// G: code bit n p + j as a function of message bit k p + i = bit j of gen[n][k] * x^i, taken from gf_mul itself
		std::vector<unsigned long long> G((size_t)nwg * rows, 0ull);
		for (int n = 0; n < N; n++)
			for (int k = 0; k < K; k++) {
				const int h = tx->gen[(size_t)n * K + k];
				if (!h) continue;
				for (int i = 0; i < p; i++) {
					const int v = d->h_mul[(size_t)h * q + (1 << i)], c = k * p + i;
					for (int j = 0; j < p; j++)
						if ((v >> j) & 1) G[(size_t)(c >> 6) * rows + n * p + j] |= 1ull << (c & 63);
				}
			}
		// (without a CRC the PN bits are the message bits: one matrix serves both)
		if ((st = tx_upload(d->err, G, tx->crc_len == 0 ? t.T : t.G_crc))) { d->tx = nbl_decoder::Tx(); return st; }
		t.G = tx->crc_len == 0 ? t.T : t.G_crc;
		if (tx->crc_len != 0 && nb > 0) {
			// message bits = [u ; C u]: CRCEncode (type 0) of the unit vector e_i leaves, after the remaining nb - 1 - i zero inputs,
			// the register r_i; r_(nb-1) = taps, r_i = one zero-input clock of r_(i+1).  Parity bit c = register bit len - 1 - c.
			const int len = tx->crc_len;
			const uint32_t taps = crc_tap_mask(len, 0), keepm = (1u << len) - 1u;
			std::vector<uint32_t> r(nb);
			uint32_t reg = taps;
			for (int i = nb - 1; i >= 0; i--) {
				r[i] = reg;
				const uint32_t fb = (reg >> (len - 1)) & 1u;
				reg = ((reg << 1) & keepm) ^ (fb ? taps : 0u);
			}
			std::vector<unsigned long long> T((size_t)nw * rows, 0ull);
			auto gbit = [&](int row, int c) { return (G[(size_t)(c >> 6) * rows + row] >> (c & 63)) & 1ull; };
			for (int row = 0; row < rows; row++) {
				// columns of G at the parity positions, as a register-shaped mask: parity bit c <-> register bit len - 1 - c
				uint32_t pm = 0;
				for (int c = 0; c < len; c++)
					if (gbit(row, nb + c)) pm |= 1u << (len - 1 - c);
				for (int i = 0; i < nb; i++) {
					const unsigned long long b = gbit(row, i) ^ (unsigned long long)(__builtin_popcount(r[i] & pm) & 1);
					if (b) T[(size_t)(i >> 6) * rows + row] |= 1ull << (i & 63);
				}
			}
			if ((st = tx_upload(d->err, T, t.T))) { d->tx = nbl_decoder::Tx(); return st; }
		}
	}
	{ // kept code bits in modulator order (Puncture, Comm.cpp:290-308)
		std::vector<int> keep;
		int pi = 0;
		for (int n = 0; n < N; n++) {
			if (pi < tx->n_punct && tx->punct[pi] == n) { pi++; continue; }
			for (int j = 0; j < p; j++) keep.push_back(n * p + j);
		}
		keep.resize((size_t)tx->n_mod_sym * mb);
		if ((st = tx_upload(d->err, keep, t.keep))) { d->tx = nbl_decoder::Tx(); return st; }
	}
	{ // CrcCheck (type 1 for CRC-24) of the K p decoded message bits: remainder of bit i; the last bit enters register bit 0
		std::vector<uint32_t> col((size_t)K * p, 0u);
		if (tx->crc_len) {
			const int len = tx->crc_len;
			const uint32_t taps = crc_tap_mask(len, 1), keepm = (1u << len) - 1u;
			uint32_t reg = 1u;
			for (int i = K * p - 1; i >= 0; i--) {
				col[i] = reg;
				const uint32_t fb = (reg >> (len - 1)) & 1u;
				reg = ((reg << 1) & keepm) ^ (fb ? taps : 0u);
			}
		}
		if ((st = tx_upload(d->err, col, t.crc_col))) { d->tx = nbl_decoder::Tx(); return st; }
	}
	{ // the register's cycle from the reference's initial contents (Comm.cpp:58-74); a state off the cycle differs from one on it
	  // in regPN[10] only, which no output and no later state depends on
		std::vector<int16_t> phase(2048, -1);
		std::vector<uint8_t> seq;
		unsigned s0 = 0;
		static const int init[11] = {1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1};
		for (int i = 0; i < 11; i++) s0 |= (unsigned)init[i] << i;
		for (unsigned s = s0; phase[s] < 0; s = pn_step(s)) { phase[s] = (int16_t)seq.size(); seq.push_back((uint8_t)((s >> 9) & 1u)); }
		for (unsigned s = 0; s < 2048; s++)
			if (phase[s] < 0 && (s & 1023u)) {
				const unsigned tw = s ^ 1024u;
				if (phase[tw] >= 0) phase[s] = phase[tw];
				else { d->err = "nbl_set_transmitter: internal error, PN register state off its cycle"; d->tx = nbl_decoder::Tx(); return NBL_ERR_ARG; }
			}
		t.period = (int)seq.size();
		t.par_mod = tx->parallel % t.period;
		if ((st = tx_upload(d->err, phase, t.phase_of)) || (st = tx_upload(d->err, seq, t.seq))) { d->tx = nbl_decoder::Tx(); return st; }
	}
	t.on = true;
	return NBL_OK;
}

// per-call scratch and the slot's buffers of the channel thread
static nbl_status ensure_tx(nbl_decoder *d, int slot, int B, std::string &err)
{
	nbl_decoder::Tx &t = d->tx;
	const size_t rows = (size_t)d->g.N * d->g.p;
	// (every size grows with B alone: the rest is the geometry the transmitter was set with)
	nbl_status s;
	if ((s = t.pn.grow(err, (size_t)B * 2 + 16)) || (s = t.u.grow(err, (size_t)B * (t.nw > 0 ? t.nw : 1) * 8)) || (s = t.bits.grow(err, (size_t)B * rows)) ||
	    (s = t.code[slot].grow(err, (size_t)B * d->g.N)) || (s = t.txi[slot].grow(err, (size_t)B * d->dm_L)))
		return s;
	return NBL_OK;
}

extern "C" nbl_status nbl_transmit_batch(nbl_decoder *d, int32_t slot, const uint16_t *pn_state, const uint32_t *lane_state, double sigma, int32_t B)
{
	if (!d || !pn_state || !lane_state || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	d->err2.clear();
	if (!d->tx.on) { d->err2 = "nbl_transmit_batch: nbl_set_transmitter has not been called"; return NBL_ERR_ARG; }
	HIP_TRY_E(d->err2, hipSetDevice(d->device));
	if (!d->stream2) HIP_TRY_E(d->err2, hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
	nbl_decoder::Tx &t = d->tx;
	d->rxs_B[slot] = 0;
	t.tx_B[slot] = 0;
	nbl_status s = ensure_tx(d, slot, B, d->err2);
	if (s) return s;
	hipStream_t st = d->stream2;
	const int N = d->g.N, p = d->g.p, rows = N * p;
	if (t.random_msg && t.nb > 0) {
		HIP_TRY_E(d->err2, hipMemcpyAsync(t.pn, pn_state, (size_t)B * 2, hipMemcpyHostToDevice, st));
		HIP_TRY_E(d->err2, nbl_launch_tx_pn(t.pn, t.phase_of, t.seq, t.period, t.par_mod, t.nb, t.nw, B, t.u, st));
		HIP_TRY_E(d->err2, nbl_launch_tx_encode(t.T, t.u, rows, t.nw, B, t.bits, st));
	} else {
		HIP_TRY_E(d->err2, hipMemsetAsync(t.bits, 0, (size_t)B * rows, st)); // all-zero message and code word, encoder skipped (Comm.cpp:258-268)
	}
	HIP_TRY_E(d->err2, nbl_launch_tx_pack(t.bits, t.keep, N, p, d->dm_L, t.mb, B, t.code[slot], t.txi[slot], st));
	s = run_channel(d, nullptr, lane_state, sigma, B, st, d->d_rxs[slot], d->d_gains[slot], &d->slot_gain[slot], d->err2, t.txi[slot]);
	if (s == NBL_OK) { d->rxs_B[slot] = B; t.tx_B[slot] = B; }
	return s;
}

extern "C" nbl_status nbl_count_errors(nbl_decoder *d, int32_t slot, int32_t B, int32_t *err_sym, int32_t *err_bit, uint8_t *crc_ok)
{
	if (!d || B <= 0 || slot < 0 || slot > 1 || !err_sym || !err_bit || !crc_ok) return NBL_ERR_ARG;
	d->err.clear();
	nbl_decoder::Tx &t = d->tx;
	if (!t.on) { d->err = "nbl_count_errors: nbl_set_transmitter has not been called"; return NBL_ERR_ARG; }
	if (t.tx_B[slot] != B) { d->err = "nbl_count_errors: slot does not hold a transmitted batch of this size (nbl_transmit_batch first)"; return NBL_ERR_ARG; }
	if (t.dec_B[slot] != B) { d->err = "nbl_count_errors: slot does not hold the outputs of a decode of this size (nbl_decode_batch_resident first)"; return NBL_ERR_ARG; }
	HIP_TRY(d, hipSetDevice(d->device));
	if ((size_t)B > t.cnt_cap) { // (the three arrays lie cnt_cap entries apart: the capacity is kept beside the buffer)
		t.cnt_cap = 0;
		if (nbl_status s = t.cnt.grow(d->err, (size_t)B * 9 + 16)) return s;
		t.cnt_cap = B;
	}
	int *es = t.cnt, *eb = t.cnt.p + t.cnt_cap;
	uint8_t *ok = (uint8_t *)(t.cnt.p + 2 * t.cnt_cap);
	HIP_TRY(d, nbl_launch_tx_errcount(t.dec[slot], t.code[slot], t.crc_col, d->g.N, t.K, d->g.p, t.crc_len, B, es, eb, ok, d->stream));
	HIP_TRY(d, hipMemcpyAsync(err_sym, es, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipMemcpyAsync(err_bit, eb, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipMemcpyAsync(crc_ok, ok, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_encode_batch(nbl_decoder *d, const int32_t *msg, int32_t B, int32_t *code, int32_t *msg_out)
{
	if (!d || !msg || !code || B < 0) return NBL_ERR_ARG;
	d->err.clear();
	nbl_decoder::Tx &t = d->tx;
	if (!t.on || !t.G) { d->err = "nbl_encode_batch: nbl_set_transmitter has not been called with a generator"; return NBL_ERR_ARG; }
	if (B == 0) return NBL_OK;
	const int N = d->g.N, p = d->g.p, K = t.K, rows = N * p, q = d->g.q;
	for (size_t i = 0; i < (size_t)B * K; i++)
		if (msg[i] < 0 || msg[i] >= q) { d->err = "nbl_encode_batch: message symbol outside 0 .. q - 1"; return NBL_ERR_ARG; }
	HIP_TRY(d, hipSetDevice(d->device));
	const int chunk = B < 4096 ? B : 4096;
	nbl_status s;
	if ((s = t.e_msg.grow(d->err, (size_t)chunk * K * 4)) || (s = t.e_u.grow(d->err, (size_t)chunk * t.nwg * 8)) ||
	    (s = t.e_bits.grow(d->err, (size_t)chunk * rows)) || (s = t.e_code.grow(d->err, (size_t)chunk * N)))
		return s;
	std::vector<uint8_t> h((size_t)chunk * N);
	for (int b0 = 0; b0 < B; b0 += chunk) {
		const int n = B - b0 < chunk ? B - b0 : chunk;
		HIP_TRY(d, hipMemcpyAsync(t.e_msg, msg + (size_t)b0 * K, (size_t)n * K * 4, hipMemcpyHostToDevice, d->stream));
		HIP_TRY(d, nbl_launch_tx_msgbits(t.e_msg, K, p, t.nwg, n, t.e_u, d->stream));
		HIP_TRY(d, nbl_launch_tx_encode(t.G, t.e_u, rows, t.nwg, n, t.e_bits, d->stream));
		// (symbols only: the index output goes to the same buffer's tail-less twin with L = 0)
		HIP_TRY(d, nbl_launch_tx_pack(t.e_bits, t.keep, N, p, 0, t.mb, n, t.e_code, nullptr, d->stream));
		HIP_TRY(d, hipMemcpyAsync(h.data(), t.e_code, (size_t)n * N, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		for (int b = 0; b < n; b++) {
			for (int i = 0; i < N; i++) code[(size_t)(b0 + b) * N + i] = h[(size_t)b * N + i];
			if (msg_out) for (int i = 0; i < K; i++) msg_out[(size_t)(b0 + b) * K + i] = h[(size_t)b * N + i];
		}
	}
	return NBL_OK;
}

extern "C" nbl_status nbl_read_transmitted(nbl_decoder *d, int32_t slot, int32_t b0, int32_t n, int32_t *tx_msg, int32_t *tx_code, uint8_t *tx_index)
{
	if (!d || slot < 0 || slot > 1 || b0 < 0 || n < 0) return NBL_ERR_ARG;
	d->err.clear();
	nbl_decoder::Tx &t = d->tx;
	if (!t.on || t.tx_B[slot] <= 0 || (long long)b0 + n > t.tx_B[slot]) { d->err = "nbl_read_transmitted: the slot does not hold these lanes (nbl_transmit_batch first)"; return NBL_ERR_ARG; }
	if (n == 0) return NBL_OK;
	HIP_TRY(d, hipSetDevice(d->device));
	const int N = d->g.N, K = t.K, L = d->dm_L;
	if (tx_msg || tx_code) {
		std::vector<uint8_t> h((size_t)n * N);
		HIP_TRY(d, hipMemcpy(h.data(), t.code[slot] + (size_t)b0 * N, h.size(), hipMemcpyDeviceToHost));
		for (int b = 0; b < n; b++) {
			if (tx_code) for (int i = 0; i < N; i++) tx_code[(size_t)b * N + i] = h[(size_t)b * N + i];
			if (tx_msg) for (int i = 0; i < K; i++) tx_msg[(size_t)b * K + i] = h[(size_t)b * N + i];
		}
	}
	if (tx_index) HIP_TRY(d, hipMemcpy(tx_index, t.txi[slot] + (size_t)b0 * L, (size_t)n * L, hipMemcpyDeviceToHost));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): the received samples [n][L][2] a slot holds
extern "C" nbl_status nbl_debug_read_slot_rx(nbl_decoder *d, int32_t slot, int32_t b0, int32_t n, double *rx)
{
	if (!d || slot < 0 || slot > 1 || b0 < 0 || n <= 0 || !rx || b0 + n > d->rxs_B[slot]) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	HIP_TRY(d, hipMemcpy(rx, d->d_rxs[slot] + (size_t)b0 * d->dm_L * 2, (size_t)n * d->dm_L * 16, hipMemcpyDeviceToHost));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): put decoded words [B][N] where nbl_decode_batch_resident leaves a slot's outputs
extern "C" nbl_status nbl_debug_set_decoded(nbl_decoder *d, int32_t slot, const int32_t *sym, int32_t B)
{
	if (!d || slot < 0 || slot > 1 || !sym || B <= 0) return NBL_ERR_ARG;
	d->err.clear();
	if (!d->tx.on) { d->err = "nbl_debug_set_decoded: nbl_set_transmitter has not been called"; return NBL_ERR_ARG; }
	HIP_TRY(d, hipSetDevice(d->device));
	d->tx.dec_B[slot] = 0;
	if (nbl_status s = d->tx.dec[slot].grow(d->err, (size_t)B * d->g.N * 4)) return s;
	HIP_TRY(d, hipMemcpy(d->tx.dec[slot], sym, (size_t)B * d->g.N * 4, hipMemcpyHostToDevice));
	d->tx.dec_B[slot] = B;
	return NBL_OK;
}
