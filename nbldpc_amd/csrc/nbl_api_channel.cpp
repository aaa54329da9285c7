// nbldpc_amd/csrc/nbl_api_channel.cpp -- the channel on the device: CRand's lanes, AWGN and flat fading (nbl_noise.hip, nbl_fading.hip),
// the two resident slots of the pipelined link chain, nbl_set_fading and the channel diagnostics.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "nbl_decoder.h"

// ---- AWGN channel + CRand on the device ------------------------------------------------------------------

static uint32_t mod_pow(uint32_t a, uint64_t k, uint32_t m)
{
	uint64_t r = 1 % m, x = a % m;
	for (; k; k >>= 1) {
		if (k & 1) r = r * x % m;
		x = x * x % m;
	}
	return (uint32_t)r;
}

extern "C" void nbl_rand_advance(uint32_t state[3], uint64_t draws)
{
	state[0] = (uint32_t)((uint64_t)(state[0] % 61967u) * mod_pow(249, draws, 61967) % 61967u);
	state[1] = (uint32_t)((uint64_t)(state[1] % 63443u) * mod_pow(251, draws, 63443) % 63443u);
	state[2] = (uint32_t)((uint64_t)(state[2] % 63599u) * mod_pow(252, draws, 63599) % 63599u);
}

// A^(4 k) mod m for k < npos, [3][npos]: the state in front of position k of a frame, as a factor on the lane's state
static std::vector<uint32_t> jump_table(size_t npos)
{
	std::vector<uint32_t> jump(3 * npos);
	const uint32_t A[3] = {249, 251, 252}, M[3] = {61967, 63443, 63599};
	for (int g = 0; g < 3; g++) {
		uint64_t x = 1;
		const uint32_t a4 = mod_pow(A[g], 4, M[g]);
		for (size_t s = 0; s < npos; s++) { jump[g * npos + s] = (uint32_t)x; x = x * a4 % M[g]; }
	}
	return jump;
}

// nblk of the fading frame at the current L (0 without fading): the frame has nblk + L positions of four uniform draws
static int fading_blocks(const nbl_decoder *d)
{
	return d->fade_model == NBL_FADING_RAYLEIGH ? (d->dm_L + d->fade_coh - 1) / d->fade_coh : 0;
}

static nbl_status ensure_noise(nbl_decoder *d, int B, std::string &err)
{
	const size_t nblk = (size_t)fading_blocks(d);
	const size_t L = (size_t)d->dm_L + nblk; // positions per lane: the buffers below are per position
	if (nblk && (!d->d_jump_f || d->jump_f_pos != (int)L)) { // the table of the fading frame, beside the AWGN one
		d->d_jump_f.release();
		d->jump_f_pos = 0;
		const std::vector<uint32_t> jump = jump_table(L);
		if (nbl_status s = d->d_jump_f.grow(err, jump.size() * 4)) return s;
		HIP_TRY_E(err, hipMemcpy(d->d_jump_f, jump.data(), jump.size() * 4, hipMemcpyHostToDevice));
		d->jump_f_pos = (int)L;
	}
	if (!nblk && !d->d_jump) {
		const std::vector<uint32_t> jump = jump_table(L);
		if (nbl_status s = d->d_jump.grow(err, jump.size() * 4)) return s;
		HIP_TRY_E(err, hipMemcpy(d->d_jump, jump.data(), jump.size() * 4, hipMemcpyHostToDevice));
	}
	if ((size_t)B <= d->noise_cap && L <= d->noise_pos) return NBL_OK; // (capacity in lanes of noise_pos positions; nbl_set_demodulator resets it)
	nbl_decoder::Noise &x = d->noise;
	x = nbl_decoder::Noise(); // (every buffer of the old set is released)
	d->noise_cap = 0;
	d->noise_pos = 0;
	const size_t nval = (size_t)B * L * 4; // two functions per normal draw, two draws per symbol
	if (nval > 0xffffffffull) { err = "nbl_decode_batch_noise: batch * symbols too large for 32-bit value indices"; return NBL_ERR_ARG; }
	// about 16 % of the values are uncertain (5 % of the logarithms, 11 % of the cosines); room for 30 %
	const size_t cap = nval * 3 / 10 + 4096;
	nbl_status s;
	if ((s = x.state.grow(err, (size_t)B * 12)) || (s = x.txi.grow(err, (size_t)B * L)) || (s = x.fn.grow(err, nval * 8)) ||
	    (s = x.fidx.grow(err, cap * 4)) || (s = x.farg.grow(err, cap * 8)) || (s = x.fval.grow(err, cap * 8)) || (s = d->d_fcount.grow(err, 16)) ||
	    (s = x.h_farg.grow(err, cap * 8)) || (s = x.h_fval.grow(err, cap * 8)))
		return s;
	d->noise_cap = B;
	d->noise_pos = L;
	d->flag_cap = cap;
	return NBL_OK;
}

// Forms RX = TX + noise for B lanes in rx_buf (grown on demand) on stream `st`: the three kernels of nbl_noise.hip with the host's
// libm in between.  Returns with the samples complete in HBM.
// tx_index == NULL: the indices are already on the device, in d_txi_dev (nbl_transmit_batch).
// Under nbl_set_fading(RAYLEIGH) the generate kernel runs over the nblk + L positions of the fading frame and nbl_fading.hip's finish
// kernel forms RX = h * TX + noise, with the per-sample gains into gain_buf (grown on demand); *has_gain says which of the two ran.
nbl_status run_channel(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int B, hipStream_t st,
                       DevBuf<double> &rx_buf, DevBuf<double> &gain_buf, bool *has_gain, std::string &err, const uint8_t *d_txi_dev)
{
	*has_gain = false;
	if (!d->dm_order) { err = "nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (d->h_cons.empty() || !d->d_cons) { err = "the channel needs the constellation points (nbl_demod_desc.constellation), also for BPSK"; return NBL_ERR_ARG; }
	nbl_status s = ensure_noise(d, B, err);
	if (s) return s;
	const size_t L = d->dm_L;
	if (tx_index && d->dm_order < 256) { // an index beyond the constellation would read past d_cons in the finish kernel (8 bytes per step:
		// the modulation orders are powers of two, so "some byte >= order" is "some bit above the order's bits is set")
		const size_t n = (size_t)B * L;
		const uint8_t hi = (uint8_t)~(d->dm_order - 1);
		uint64_t m8 = 0, any = 0;
		for (int k = 0; k < 8; k++) m8 = (m8 << 8) | hi;
		size_t i = 0;
		for (; i + 8 <= n; i += 8) { uint64_t w8; memcpy(&w8, tx_index + i, 8); any |= w8 & m8; }
		for (; i < n; i++) any |= (uint64_t)(tx_index[i] & hi);
		if (any || (d->dm_order & (d->dm_order - 1))) {
			for (size_t k = 0; k < n; k++)
				if ((int)tx_index[k] >= d->dm_order) { err = "tx_index holds a value >= mod_order"; return NBL_ERR_ARG; }
		}
	}
	const size_t bytes = (size_t)B * L * 16;
	if ((s = rx_buf.grow(err, bytes))) return s;
	const int nblk = fading_blocks(d), npos = (int)L + nblk;
	if (nblk && (s = gain_buf.grow(err, bytes))) return s;
	nbl_decoder::Noise &x = d->noise;
	const bool timing = getenv("NBL_CHANNEL_TIMING") != nullptr;
	auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double t0 = now();
	double t1 = t0, t2 = t0, t3 = t0;
	HIP_TRY_E(err, hipMemcpyAsync(x.state, lane_state, (size_t)B * 12, hipMemcpyHostToDevice, st));
	if (tx_index) HIP_TRY_E(err, hipMemcpyAsync(x.txi, tx_index, (size_t)B * L, hipMemcpyHostToDevice, st));
	HIP_TRY_E(err, hipMemsetAsync(d->d_fcount, 0, 4, st));
	HIP_TRY_E(err, nbl_launch_noise_gen(x.state, nblk ? d->d_jump_f.p : d->d_jump.p, npos, B, x.fn, x.fidx, x.farg, d->d_fcount, (unsigned)d->flag_cap, st));
	unsigned nflag = 0;
	HIP_TRY_E(err, hipMemcpyAsync(&nflag, d->d_fcount, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY_E(err, hipStreamSynchronize(st));
	if (nflag > d->flag_cap) { err = "nbl_decode_batch_noise: more uncertain values than the list holds (30 % of all)"; return NBL_ERR_NOMEM; }
	d->last_flag_frac = (double)nflag / ((double)B * npos * 4);
	t1 = now();
	if (nflag) {
		HIP_TRY_E(err, hipMemcpyAsync(x.h_farg, x.farg, (size_t)nflag * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY_E(err, hipStreamSynchronize(st));
		t2 = now();
		// the host's own libm decides the uncertain values: log(1 - u1) or cos(2 pi u2), Rand.cpp:35
		int T = (int)std::thread::hardware_concurrency();
		if (const char *e = getenv("NBL_HOST_THREADS")) T = atoi(e);
		if (T > 16) T = 16;
		if (T < 1 || nflag < 4096) T = 1;
		auto work = [&](unsigned lo, unsigned hi) {
			// arguments of the logarithm are 1 - u1 in (0, 1]; arguments of the cosine are 2 pi u2 in [0, 2 pi): the list marks a
			// cosine argument by its sign bit (the kernel stores -x, and -0.0 for x = 0), so only the arguments travel
			for (unsigned k = lo; k < hi; k++) {
				const double a = x.h_farg[k];
				x.h_fval[k] = std::signbit(a) ? std::cos(-a) : std::log(a);
			}
		};
		if (T == 1) work(0, nflag);
		else {
			std::vector<std::thread> th;
			for (int t = 0; t < T; t++) th.emplace_back(work, (unsigned)((uint64_t)nflag * t / T), (unsigned)((uint64_t)nflag * (t + 1) / T));
			for (auto &x : th) x.join();
		}
		t3 = now();
		HIP_TRY_E(err, hipMemcpyAsync(x.fval, x.h_fval, (size_t)nflag * 8, hipMemcpyHostToDevice, st));
		HIP_TRY_E(err, nbl_launch_noise_patch(x.fn, x.fidx, x.fval, nflag, st));
	}
	if (nblk)
		HIP_TRY_E(err, nbl_launch_fading_finish(x.fn, tx_index ? x.txi.p : d_txi_dev, d->d_cons, sigma, (int)L, nblk, d->fade_coh, B, rx_buf, gain_buf, st));
	else
		HIP_TRY_E(err, nbl_launch_noise_finish(x.fn, tx_index ? x.txi.p : d_txi_dev, d->d_cons, sigma, (int)L, B, rx_buf, st));
	HIP_TRY_E(err, hipStreamSynchronize(st));
	*has_gain = nblk != 0;
	if (timing)
		fprintf(stderr, "[channel] B=%d: generate %.2f ms, list to host %.2f ms, host libm (%u values) %.2f ms, patch + finish %.2f ms\n", B,
		        (t1 - t0) * 1e3, (t2 - t1) * 1e3, nflag, (t3 - t2) * 1e3, (now() - t3) * 1e3);
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_noise(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B,
                                             int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	if (!d || !tx_index || !lane_state || !out_sym || B < 0 || !(sigma > 0)) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	if ((s = run_channel(d, tx_index, lane_state, sigma, B, d->stream, d->d_rx, d->d_gain, &d->rx_gain, d->err))) return s;
	HIP_TRY(d, launch_demod(d, d->d_rx, sigma, B, nullptr, d->rx_gain ? d->d_gain.p : nullptr));
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	return read_back(d, d->w.out, d->w.done, d->w.iters, B, out_sym, converged, iters, hipMemcpyDeviceToHost, d->stream, true);
}

// Two-phase form: the channel of batch k+1 (second stream, host libm) may run on another host thread while batch k is decoded.
extern "C" nbl_status nbl_channel_batch(nbl_decoder *d, int32_t slot, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B)
{
	if (!d || !tx_index || !lane_state || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	d->err2.clear();
	HIP_TRY_E(d->err2, hipSetDevice(d->device));
	if (!d->stream2) HIP_TRY_E(d->err2, hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
	d->rxs_B[slot] = 0;
	const nbl_status s = run_channel(d, tx_index, lane_state, sigma, B, d->stream2, d->d_rxs[slot], d->d_gains[slot], &d->slot_gain[slot],
	                                 d->err2);
	if (s == NBL_OK) d->rxs_B[slot] = B;
	return s;
}

// what the two resident decode calls refuse about their slot and outputs
nbl_status resident_check(nbl_decoder *d, int slot, int B, const int32_t *out_sym)
{
	if (!out_sym && !d->tx.on) { d->err = "nbl_decode_batch_resident: out_sym may only be NULL once nbl_set_transmitter has been called"; return NBL_ERR_ARG; }
	if (d->rxs_B[slot] != B) { d->err = "nbl_decode_batch_resident: slot does not hold the samples of a batch of this size (nbl_channel_batch first)"; return NBL_ERR_ARG; }
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_resident(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	if (!d || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	if (nbl_status rs = resident_check(d, slot, B, out_sym)) return rs;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	HIP_TRY(d, launch_demod(d, d->d_rxs[slot], sigma, B, nullptr, d->slot_gain[slot] ? d->d_gains[slot].p : nullptr));
	if (d->tx.on) d->tx.dec_B[slot] = 0;
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	if (out_sym) HIP_TRY(d, hipMemcpyAsync(out_sym, d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (d->tx.on) { // the slot keeps its outputs for nbl_count_errors
		if ((s = d->tx.dec[slot].grow(d->err, (size_t)B * d->g.N * 4))) return s;
		HIP_TRY(d, hipMemcpyAsync(d->tx.dec[slot], d->w.out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToDevice, d->stream));
	}
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->w.done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->w.iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	if (d->tx.on) d->tx.dec_B[slot] = B;
	return NBL_OK;
}

// ---- flat fading (include/nbldpc.h) ---------------------------------------------------------------------------

extern "C" nbl_status nbl_set_fading(nbl_decoder *d, const nbl_fading_desc *f)
{
	if (!d) return NBL_ERR_ARG;
	if (!f || f->model == NBL_FADING_NONE) { d->fade_model = NBL_FADING_NONE; d->fade_coh = 1; return NBL_OK; }
	if (f->model != NBL_FADING_RAYLEIGH) {
		d->err = "nbl_set_fading: unknown model " + std::to_string(f->model) + " (NBL_FADING_NONE = 0, NBL_FADING_RAYLEIGH = 1)";
		return NBL_ERR_ARG;
	}
	if (f->coherence < 1) {
		d->err = "nbl_set_fading: coherence must be at least 1, got " + std::to_string(f->coherence);
		return NBL_ERR_ARG;
	}
	d->fade_model = f->model;
	d->fade_coh = f->coherence;
	return NBL_OK;
}

extern "C" uint64_t nbl_channel_draws(const nbl_decoder *d)
{
	return d ? 4ull * (uint64_t)fading_blocks(d) + 4ull * (uint64_t)d->dm_L : 0;
}

extern "C" nbl_status nbl_read_gains(nbl_decoder *d, int32_t slot, int32_t b0, int32_t n, double *gain)
{
	if (!d || slot < 0 || slot > 1 || b0 < 0 || n < 0 || (n > 0 && !gain)) return NBL_ERR_ARG;
	d->err.clear();
	if (d->rxs_B[slot] <= 0 || !d->slot_gain[slot]) { d->err = "nbl_read_gains: the slot holds no gains (its samples were not formed under nbl_set_fading)"; return NBL_ERR_ARG; }
	if ((long long)b0 + n > d->rxs_B[slot]) { d->err = "nbl_read_gains: the slot does not hold these lanes"; return NBL_ERR_ARG; }
	if (n == 0) return NBL_OK;
	HIP_TRY(d, hipSetDevice(d->device));
	HIP_TRY(d, hipMemcpy(gain, d->d_gains[slot] + (size_t)b0 * d->dm_L * 2, (size_t)n * d->dm_L * 16, hipMemcpyDeviceToHost));
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): run the channel alone and return the received samples [B][L][2] and the
// fraction of log / cos values that went to the host's libm.
extern "C" nbl_status nbl_debug_channel(nbl_decoder *d, const uint8_t *tx_index, const uint32_t *lane_state, double sigma, int32_t B,
                                        double *rx_out, double *flag_frac)
{
	if (!d || !tx_index || !lane_state || !rx_out || B <= 0) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = run_channel(d, tx_index, lane_state, sigma, B, d->stream, d->d_rx, d->d_gain, &d->rx_gain, d->err);
	if (s) return s;
	HIP_TRY(d, hipMemcpyAsync(rx_out, d->d_rx, (size_t)B * d->dm_L * 16, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	if (flag_frac) *flag_frac = d->last_flag_frac;
	return NBL_OK;
}
